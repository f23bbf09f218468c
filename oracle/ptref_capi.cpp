/*
 * ptref_capi.cpp — C entry points over the REFERENCE's own headers.  TEST INFRASTRUCTURE ONLY.
 *
 * Built by oracle/Makefile into oracle/_ref/libptref.so and libptref_om.so (both git-ignored)
 * when the reference tree is present; tests/test_oracle_vs_reference.py loads them to pin
 * oracle/pt_oracle.c bit for bit against the code it restates.  This file holds no reference
 * text: it includes PBRT/Conductor.h, PBRT/GlossyDiffuse.h and Renderer/Camera.h by path at
 * build time (the Makefile's -I flags) and only calls what they define.
 *
 * Every ref_bsdf_* call hands the reference what orc_bsdf_* hand the oracle: a zeroed
 * Surface / BSDFSample, identity shading matrices, normal +z, TransportMode::Radiance and both
 * lobes on.  Signatures follow pt_oracle.h.
 *
 * Must be compiled with clang++: the reference writes vec2(rnd(seed), rnd(seed)), its PTX
 * draws left to right, and clang evaluates arguments left to right where g++ goes right to
 * left.  ref_disk_concentric exists so the test can prove which one built the library.
 */
#include "PBRT/Conductor.h"
#include "PBRT/GlossyDiffuse.h"

#include "Camera.h"

#include <cstring>

namespace {

RadianceRayData g_ray_record;  /* zero-initialised: isDebugRay = false */

Surface make_surface(const float albedo[3], float roughness, const float wo[3]) {
    Surface s;
    std::memset(&s, 0, sizeof s);
    s.ShadingToWorld = glm::mat3(1.0f);
    s.WorldToShading = glm::mat3(1.0f);
    s.gNormal = glm::vec3(0.0f, 0.0f, 1.0f);
    s.sNormal = glm::vec3(0.0f, 0.0f, 1.0f);
    s.outgoingRay = glm::vec3(wo[0], wo[1], wo[2]);
    s.roughness = roughness;
    s.albedo = glm::vec3(albedo[0], albedo[1], albedo[2]);
    return s;
}

glm::vec3 v3(const float* p) { return glm::vec3(p[0], p[1], p[2]); }

}  // namespace

/* The payload words IsDebugRay() unpacks (RayData.h): one zeroed record, packed by the
 * reference's own packPointer. */
uint32_t optixGetPayload_0() {
    uint32_t i0, i1;
    packPointer(&g_ray_record, i0, i1);
    return i0;
}
uint32_t optixGetPayload_1() {
    uint32_t i0, i1;
    packPointer(&g_ray_record, i0, i1);
    return i1;
}

extern "C" {

enum { REF_LAMBERT = 0, REF_CONDUCTOR = 1, REF_DIELECTRIC = 2, REF_LAYERED = 3 };

uint32_t ref_tea16(uint32_t v0, uint32_t v1) { return RandomOptix::tea<16>(v0, v1); }

void ref_rnd_seq(uint32_t seed, int32_t n, float* out, uint32_t* seed_out) {
    unsigned int s = seed;
    for (int32_t i = 0; i < n; ++i) out[i] = RandomOptix::rnd(s);
    if (seed_out) *seed_out = s;
}

/* build self-check: the two draws inside one constructor call (LambertDiffuse.h:40) */
void ref_disk_concentric(uint32_t* seed, float out[2]) {
    unsigned int s = *seed;
    glm::vec2 d = PBRT::LambertDiffuse::SampleUniformDiskConcentric(s);
    *seed = s;
    out[0] = d.x;
    out[1] = d.y;
}

/* out: color[3], pdf, direction[3], flags (bit0 refl, bit1 trans, bit2 specular, bit3 glossy) */
int32_t ref_bsdf_sample(int32_t model, uint32_t* seed, const float albedo[3], float roughness, const float wo[3],
                        float out[8]) {
    using namespace PBRT;
    Surface surface = make_surface(albedo, roughness, wo);
    BSDFSample b;
    std::memset(&b, 0, sizeof b);
    unsigned int s = *seed;
    bool ok;
    switch (model) {
        case REF_LAMBERT: ok = LambertDiffuse::Sample_f(s, surface, v3(wo), b, true); break;
        case REF_CONDUCTOR: ok = Conductor::Sample_f(s, surface.albedo, roughness, v3(wo), b); break;
        case REF_DIELECTRIC:
            ok = Dielectric::Sample_f(s, surface, v3(wo), b, Dielectric::TransportMode::Radiance, true, true);
            break;
        default: ok = GlossyDiffuse::Sample_f(s, surface, b); break;
    }
    *seed = s;
    out[0] = b.color.x; out[1] = b.color.y; out[2] = b.color.z; out[3] = b.pdf;
    out[4] = b.direction.x; out[5] = b.direction.y; out[6] = b.direction.z;
    out[7] = (float)((b.reflection ? 1 : 0) | (b.transmission ? 2 : 0) | (b.specular ? 4 : 0) | (b.glossy ? 8 : 0));
    return ok ? 1 : 0;
}

void ref_bsdf_eval(int32_t model, uint32_t* seed, const float albedo[3], float roughness, const float wo[3],
                   const float wi[3], float out[3]) {
    using namespace PBRT;
    Surface surface = make_surface(albedo, roughness, wo);
    unsigned int s = *seed;
    glm::vec3 r;
    switch (model) {
        case REF_LAMBERT: r = LambertDiffuse::f(surface, v3(wo), v3(wi)); break;
        case REF_CONDUCTOR: r = Conductor::f(surface.albedo, roughness, v3(wo), v3(wi)); break;
        case REF_DIELECTRIC: r = Dielectric::f(surface, v3(wo), v3(wi), Dielectric::TransportMode::Radiance); break;
        default: r = GlossyDiffuse::f(s, surface, v3(wi)); break;
    }
    *seed = s;
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}

/* Lambert and Dielectric have a PDF of their own.  The reference has no Conductor::PDF: its
 * Sample_f forms the density in line (Conductor.h:166) from Microfacet::PDF_Isotropic, and
 * that expression is evaluated here at the half vector of wo and wi faced to +z, the point
 * orc_bsdf_pdf evaluates.  Layered has no PDF at all and gives 0, as orc_bsdf_pdf does. */
float ref_bsdf_pdf(int32_t model, float roughness, const float wo3[3], const float wi3[3]) {
    using namespace PBRT;
    const float zero3[3] = {0.0f, 0.0f, 0.0f};
    Surface surface = make_surface(zero3, roughness, wo3);
    glm::vec3 wo = v3(wo3), wi = v3(wi3);
    if (model == REF_LAMBERT) return LambertDiffuse::PDF(surface, wo, wi, true);
    if (model == REF_DIELECTRIC) return Dielectric::PDF(surface, wo, wi, true, true);
    if (model == REF_CONDUCTOR) {
        float alpha = Surface::GetAlpha(roughness);
        if (!SpherGeom::SameHemisphere(wo, wi) || Surface::IsEffectifvelySmooth(alpha)) return 0.0f;
        glm::vec3 wm = wo + wi;
        if (LengthSqr(wm) == 0) return 0.0f;
        wm = glm::normalize(wm);
        if (wm.z < 0) wm = -wm;
        return Microfacet::PDF_Isotropic(wo, wm, alpha) / (4 * AbsDot(wo, wm));
    }
    return 0.0f;
}

/* Batched forms: case k has its own model-independent inputs; seeds are advanced in place. */
void ref_bsdf_sample_n(int32_t model, int32_t n, uint32_t* seeds, const float* albedo3, const float* roughness,
                       const float* wo3, float* out8, int32_t* ok) {
    for (int32_t k = 0; k < n; ++k)
        ok[k] = ref_bsdf_sample(model, seeds + k, albedo3 + 3 * (size_t)k, roughness[k], wo3 + 3 * (size_t)k,
                                out8 + 8 * (size_t)k);
}
void ref_bsdf_eval_n(int32_t model, int32_t n, uint32_t* seeds, const float* albedo3, const float* roughness,
                     const float* wo3, const float* wi3, float* out3) {
    for (int32_t k = 0; k < n; ++k)
        ref_bsdf_eval(model, seeds + k, albedo3 + 3 * (size_t)k, roughness[k], wo3 + 3 * (size_t)k,
                      wi3 + 3 * (size_t)k, out3 + 3 * (size_t)k);
}
void ref_bsdf_pdf_n(int32_t model, int32_t n, const float* roughness, const float* wo3, const float* wi3,
                    float* out) {
    for (int32_t k = 0; k < n; ++k)
        out[k] = ref_bsdf_pdf(model, roughness[k], wo3 + 3 * (size_t)k, wi3 + 3 * (size_t)k);
}

/* Camera.cpp and GlmHelperMethods.cpp as they are; position, inverse view and inverse
 * projection formed as OptixRenderer::SetCamera forms them (OptixRenderer.cpp:662-668). */
void ref_camera_from_blender(const float blender_pos[3], const float blender_rot_deg[3], float fov_deg,
                             int32_t width, int32_t height, float pos[3], float inv_view[16],
                             float inv_proj[16]) {
    Camera camera;
    camera.SetHorizontalFOV(fov_deg);
    camera.SetBlenderPosition(v3(blender_pos));
    camera.SetBlenderRotation(v3(blender_rot_deg));
    glm::ivec2 size(width, height);
    const float aspect = size.x / float(size.y);
    glm::vec3 p = camera.position;
    glm::mat4 iv = glm::inverse(camera.GetViewMatrix());
    glm::mat4 ip = glm::inverse(camera.GetProjectionMatrix(aspect));
    pos[0] = p.x; pos[1] = p.y; pos[2] = p.z;
    std::memcpy(inv_view, &iv[0][0], 16 * sizeof(float));
    std::memcpy(inv_proj, &ip[0][0], 16 * sizeof(float));
}

}  /* extern "C" */
