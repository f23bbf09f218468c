// pt_shade.h — what happens at a surface hit, one definition per step.
//
// The steps of __closesthit__radiance (devicePrograms.cu:343-514) after pt_device.h found the hit:
// surface, light pick, NEE shadow ray and contribution, lit / occluder table lookups, continuation.
// The megakernel's path_segment (pt_render.hip), the wavefront shading kernels (pt_wavefront.hip) and
// the table builders (pt_lit.hip) all call these, so kernels that must agree on a quantity bit for
// bit run the same expression.  -ffp-contract=off; every expression keeps the oracle's association
// order (oracle/pt_oracle.c is the independent side and shares nothing with this file).
#pragma once
#include "pt_device.h"
#include "pt_lit.h"

namespace pt {

// Surface reconstruction at a hit: GetNormal / GetSurfacePos (devicePrograms.cu:83-129),
// back-face flip (:379-382), SampleTextures + normal mapping (:392-409), BuildTangentSpace
// (:168-212).  The texture ids are used as given (the reference's hasNormalTexture /
// hasMetalRoughTexture = HasAlbedoTex() flag bug, OptixRenderer.cpp:535,540, is not kept).
struct SurfaceHit {
    f3 pos, ng;
    bool ng_back;  // ng points against the stored winding's normal e1 x e2 (the skip table's side 1)
    Frame fr;
    f3 wo;        // shading space
    f3 albedo;
    float metallic, roughness;
};

__device__ __forceinline__ void apply_textures(const DevScene& S, int ti, float u, float v, const float4 M1,
                                               const float4 M2, f3& albedo, float& metallic, float& roughness,
                                               f3& Ns) {
    const int at = __float_as_int(M1.z), nt = __float_as_int(M1.w), mt = __float_as_int(M2.x);
    float x, y;
    tri_texcoord(S, ti, u, v, x, y);
    f3 ntex = mk(0.0f, 0.0f, 0.0f);
    if (at >= 0) {
        const float4 c = tex_sample(S, at, x, y, true);
        albedo = albedo * mk(c.x, c.y, c.z);
    }
    if (nt >= 0) {
        const float4 c = tex_sample(S, nt, x, y, false);
        ntex = mk(c.x, c.y, c.z);
    }
    if (mt >= 0) {
        const float4 c = tex_sample(S, mt, x, y, false);
        metallic = c.x;
        roughness = c.y;
    }
    if (ntex.x != 0.0f || ntex.y != 0.0f || ntex.z != 0.0f) {  // normal mapping in the a8 frame of Ns
        f3 d1 = cross(Ns, mk(0.0f, 0.0f, 1.0f));
        f3 d2 = cross(Ns, mk(0.0f, 1.0f, 0.0f));
        f3 T0 = (length(d1) > length(d2)) ? d1 : d2;
        T0 = normalize(T0);
        const f3 B0 = cross(T0, Ns);
        const f3 tn = mk(ntex.x * 2.0f - 1.0f, ntex.y * 2.0f - 1.0f, ntex.z * 2.0f - 1.0f);
        Ns = normalize(mk((T0.x * tn.x + B0.x * tn.y) + Ns.x * tn.z, (T0.y * tn.x + B0.y * tn.y) + Ns.y * tn.z,
                          (T0.z * tn.x + B0.z * tn.y) + Ns.z * tn.z));
    }
}

// TEX: the scene has textures (kernels are instantiated both ways so untextured scenes keep
// the texture code out of their register budget).
template <bool TEX>
__device__ __forceinline__ void reconstruct(const DevScene& S, const Hit& h, f3 d, SurfaceHit& s) {
    const int ti = h.tri;
    const float4 A = S.isect[3 * ti];
    const float4 S0 = S.shade[4 * ti], S1 = S.shade[4 * ti + 1], S2 = S.shade[4 * ti + 2], S3 = S.shade[4 * ti + 3];
    // the edges again from the vertices: e = v - v0 is the one fp32 subtraction k_gather stored in
    // isect, so Ng is bit-identical, and the hit costs five gathers instead of seven
    const float4 E1 = make_float4(S0.x - A.x, S0.y - A.y, S0.z - A.z, 0.0f);
    const float4 E2 = make_float4(S1.x - A.x, S1.y - A.y, S1.z - A.z, 0.0f);
    const int mi = __float_as_int(S3.w);
    const float4 M0 = S.mats[kMatStride * mi], M1 = S.mats[kMatStride * mi + 1];
    f3 wo_w = normalize(-d);
    f3 v0 = mk(A.x, A.y, A.z), v1 = mk(S0.x, S0.y, S0.z), v2 = mk(S1.x, S1.y, S1.z);
    f3 n0 = mk(S0.w, S1.w, S2.x), n1 = mk(S2.y, S2.z, S2.w), n2 = mk(S3.x, S3.y, S3.z);
    f3 Ng = cross(mk(E1.x, E1.y, E1.z), mk(E2.x, E2.y, E2.z));
    const float u = h.u, v = h.v;
    float w = 1.0f - u - v;
    f3 Ns = mk(w * n0.x + u * n1.x + v * n2.x, w * n0.y + u * n1.y + v * n2.y, w * n0.z + u * n1.z + v * n2.z);
    if (M1.y != kNormalNone) {  // has normals: normalize(modelMatrix * vec4(Ns, 0))
        if (TEX && M1.y == kNormalObject) {  // mat4_mul_vec4's order, row by row
            const float4 R0 = S.mats[kMatStride * mi + 3], R1 = S.mats[kMatStride * mi + 4],
                         R2 = S.mats[kMatStride * mi + 5];
            Ns = mk(mat_row_dir(R0, Ns), mat_row_dir(R1, Ns), mat_row_dir(R2, Ns));
        }
        Ns = normalize(Ns);
    }
    const bool ng_flip = dot(wo_w, Ng) < 0.0f;
    if (ng_flip) Ng = -Ng;
    Ng = normalize(Ng);
    if (dot(Ng, Ns) < 0.0f) Ns = -Ns;
    Ns = normalize(Ns);
    if (h.back) {
        Ns = Ns * -1.0f;
        Ng = Ng * -1.0f;
    }
    s.pos = mk(w * v0.x + u * v1.x + v * v2.x, w * v0.y + u * v1.y + v * v2.y, w * v0.z + u * v1.z + v * v2.z);
    s.ng = Ng;
    s.ng_back = ng_flip != h.back;  // negation and normalize are exact in the sign
    s.albedo = mk(M0.x, M0.y, M0.z);
    s.metallic = M0.w;
    s.roughness = M1.x;
    if (TEX) {
        const float4 M2 = S.mats[kMatStride * mi + 2];
        if (M2.y != 0.0f) apply_textures(S, ti, u, v, M1, M2, s.albedo, s.metallic, s.roughness, Ns);
    }
    f3 c1 = cross(Ns, mk(0.0f, 0.0f, 1.0f));
    f3 c2 = cross(Ns, mk(0.0f, 1.0f, 0.0f));
    f3 T = (length(c1) > length(c2)) ? c1 : c2;
    T = normalize(T);
    s.fr.t = T;
    s.fr.b = cross(T, Ns);
    s.fr.n = Ns;
    s.wo = to_local(s.fr, wo_w);
}

// The reference's debug print of one bounce of the debug path (devicePrograms.cu:428-437:
// position, albedo, shading and geometry normal, roughness, metallic, at bounceCounter), plus
// the hit triangle's global index, the throughput entering the bounce and the radiance so far.
// Record layout: ptamd.h pt_debug_bounce.
__device__ __forceinline__ void debug_record(const DevLaunch& L, int bounce, int prim, const SurfaceHit& sf, f3 beta,
                                             f3 radiance) {
    if (bounce < 1 || bounce > kDebugMaxBounces) return;
    float* r = L.debug + (size_t)(bounce - 1) * kDebugRecordFloats;
    const float v[kDebugRecordFloats] = {__int_as_float(bounce), __int_as_float(prim),
                                         sf.pos.x, sf.pos.y, sf.pos.z, sf.albedo.x, sf.albedo.y, sf.albedo.z,
                                         sf.fr.n.x, sf.fr.n.y, sf.fr.n.z, sf.ng.x, sf.ng.y, sf.ng.z,
                                         sf.roughness, sf.metallic, beta.x, beta.y, beta.z,
                                         radiance.x, radiance.y, radiance.z};
    for (int k = 0; k < kDebugRecordFloats; ++k) r[k] = v[k];
}

// ---- next-event estimation (devicePrograms.cu:446-472) -----------------------------------------
// light choice: Lighting::GetRandomPointLight (LightMethods.h:25-40)
__device__ __forceinline__ float pick_light(const DevLaunch& L, uint32_t& seed, int& li) {
    li = 0;
    if (L.n_lights == 1) return 1.0f;
    if (L.n_lights <= 0) return 0.0f;
    float r = rnd(seed);
    li = (int)(r * (float)L.n_lights);
    if (li >= L.n_lights) li = L.n_lights - 1;
    return 1.0f / (float)L.n_lights;
}
// What pick_light returned for a launch with lights, for a kernel that runs after the pick (k_shade_nee).
__device__ __forceinline__ float light_pdf(const DevLaunch& L) {
    return L.n_lights == 1 ? 1.0f : 1.0f / (float)L.n_lights;
}

// From the point to the light, not normalised: the shadow ray's extent and the lit table's side test.
__device__ __forceinline__ f3 light_vec(const DevLight& lt, f3 pos) { return mk(lt.px, lt.py, lt.pz) - pos; }
// The light's direction in the shading frame.
__device__ __forceinline__ f3 light_local(const SurfaceHit& sf, const DevLight& lt) {
    return to_local(sf.fr, normalize(light_vec(lt, sf.pos)));
}
// How far a ray's origin leaves the surface along +-Ng: the shadow ray's and the continuation's, so a
// continuation that leaves on Ng's side starts at the shadow ray's origin (k_shade_fused kShareOrigin).
__device__ __forceinline__ f3 origin_offset(f3 ng) { return 1e-3f * ng; }
// The shadow ray of a point with geometric normal ng towards a light at pos + ldir.
__device__ __forceinline__ void shadow_ray(f3 pos, f3 ng, f3 ldir, f3& o, f3& dir, float& tmax) {
    o = pos + origin_offset(ng);
    dir = normalize(ldir);
    tmax = length(ldir);
}
// f |cos| of the light's direction lds, and the unoccluded light's contribution through it.  The squared
// distance is a step of its own: k_shade_nee takes it before the layered walk and the rest after it.
__device__ __forceinline__ f3 nee_spectrum(f3 f, f3 lds) { return f * abs_dot(lds, mk(0.0f, 0.0f, 1.0f)); }
__device__ __forceinline__ float light_dist2(const DevLight& lt, f3 pos) {
    const f3 dd = pos - mk(lt.px, lt.py, lt.pz);
    return dd.x * dd.x + dd.y * dd.y + dd.z * dd.z;
}
__device__ __forceinline__ f3 nee_contrib(f3 beta, f3 spectrum, const DevLight& lt, float d2, float P) {
    const f3 Li = mk(lt.cr, lt.cg, lt.cb) / d2;
    return ((beta * spectrum) * Li) / (P * 1.0f);
}

// continuation (devicePrograms.cu:501-509) + loop test of SamplePath (:646)
__device__ __forceinline__ bool continue_path(const SurfaceHit& sf, const BSample& bs, f3& beta, f3& o, f3& d,
                                              int next_bounce, int max_bounces) {
    float ac = abs_dot(bs.dir, mk(0.0f, 0.0f, 1.0f));
    beta = beta * mk(bs.color.x * ac / bs.pdf, bs.color.y * ac / bs.pdf, bs.color.z * ac / bs.pdf);
    f3 off = origin_offset(sf.ng);
    if (dot(bs.dir, mk(0.0f, 0.0f, 1.0f)) < 0.0f) off = -off;
    o = sf.pos + off;
    d = normalize(to_world(sf.fr, bs.dir));
    return next_bounce < max_bounces && length(beta) > 0.00001f;
}

// ---- lit table and occluder candidates (pt_lit.h, pt_lit.hip) ----------------------------------
// The hit's cell (-1: a triangle without cells) and the (light, cell) bit.  A set bit answers the NEE
// visibility test of a hit whose shadow origin is offset to the light's side (lit_side): unoccluded,
// no shadow ray.  occ_entry: the occluder candidate of such a ray the bit left open, -1 or a triangle.
__device__ __forceinline__ int lit_cell(const DevLaunch& L, const Hit& h) {
    const uint32_t w = L.lit_tri[h.tri];
    const int k = lit_level(w);
    return k == kLitNoCells ? -1 : (int)(lit_first(w) + lit_cell_index(k, h.u, h.v));
}
__device__ __forceinline__ bool lit_bit(const DevLaunch& L, int li, int cell) {
    return (L.lit_bits[(size_t)li * L.lit_words + ((uint32_t)cell >> 5)] >> (cell & 31)) & 1u;
}
__device__ __forceinline__ bool lit_side(int cell, f3 ldir, const SurfaceHit& sf) {
    return cell >= 0 && dot(ldir, sf.ng) > kLitDelta;
}
__device__ __forceinline__ int occ_entry(const DevLaunch& L, int li, int cell) {
    return L.occ_tab[li * (int)L.lit_cells + cell];
}

}  // namespace pt
