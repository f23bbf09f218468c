// pt_capi_bake.cpp — the host half of a scene: validation, the retained copy and the bake.  Calls no HIP
// runtime function, so tests/scene_ingest_check.cpp links it host-only.
#include "pt_renderer.h"

using namespace pt;

namespace {

// glm mat4 * vec4 for the host-side pre-transform (GetVertices, devicePrograms.cu:77-81)
void xform4(const float* m, const float v[4], float out[4]) { mat4_mul_vec4(m, v, out); }

}  // namespace

namespace pt {

int ingest_scene(const pt_scene* scene, GeomHost& G_out, std::vector<float4>& mats_out, std::vector<int4>& texinfo_out,
                 size_t* ntexel_out, bool* any_tex_out, std::string* err) {
    auto reject = [&](const char* msg) {  // the outputs are written only at the end
        *err = msg;
        return (int)PT_ERR_INVALID;
    };
    // ---- host: world-space triangle soup in original (mesh-concatenated) order ----
    size_t ntri = 0;
    for (int m = 0; m < scene->n_meshes; ++m) {
        const pt_mesh& me = scene->meshes[m];
        if (me.n_triangles < 0 || me.n_vertices < 0) return reject("pt_create: negative counts");
        if (me.n_triangles > 0 && (!me.vertices || !me.indices))
            return reject("pt_create: mesh without vertices/indices");
        ntri += (size_t)me.n_triangles;
    }
    if (ntri > (size_t)0x3fffffff) return reject("pt_create: too many triangles");
    // textures (CreateTextures, OptixRenderer.cpp:562-612): one RGBA8 texel pool + (offset, w, h)
    const int ntex = scene->n_textures;
    if (ntex < 0 || (ntex > 0 && !scene->textures)) return reject("pt_create: invalid textures");
    std::vector<int4> texinfo((size_t)std::max(1, ntex));
    size_t ntexel = 0;
    for (int k = 0; k < ntex; ++k) {
        const pt_texture& tx = scene->textures[k];
        if (tx.width <= 0 || tx.height <= 0 || !tx.rgba8) return reject("pt_create: invalid texture");
        texinfo[(size_t)k] = make_int4((int)ntexel, tx.width, tx.height, 0);
        ntexel += (size_t)tx.width * (size_t)tx.height;
    }
    if (ntexel > (size_t)0x7fffffff) return reject("pt_create: textures too large");
    bool any_tex = false;
    for (int m = 0; m < scene->n_meshes; ++m) {
        const pt_mesh& me = scene->meshes[m];
        for (int id : {me.albedo_tex, me.normal_tex, me.metal_rough_tex}) {
            if (id < -1 || id >= ntex) return reject("pt_create: texture id out of range");
            any_tex = any_tex || id >= 0;
        }
    }
    std::vector<float4> mats((size_t)kMatStride * (size_t)std::max(1, scene->n_meshes));
    GeomHost G;
    G.voff.push_back(0);
    G.tidx.reserve(ntri);
    if (any_tex) G.uvs.reserve(2 * ntri);
    for (int m = 0; m < scene->n_meshes; ++m) {
        const pt_mesh& me = scene->meshes[m];
        auto ibits = [](int v) {
            float f;
            std::memcpy(&f, &v, 4);
            return f;
        };
        const bool textured = me.albedo_tex >= 0 || me.normal_tex >= 0 || me.metal_rough_tex >= 0;
        mats[kMatStride * m] = make_float4(me.albedo[0], me.albedo[1], me.albedo[2], me.metallic);
        mats[kMatStride * m + 1] =
            make_float4(me.roughness, kNormalNone, ibits(me.albedo_tex), ibits(me.normal_tex));  // .y: normal_rows
        mats[kMatStride * m + 2] = make_float4(ibits(me.metal_rough_tex), textured ? 1.0f : 0.0f, 0.0f, 0.0f);
        // retained: object-space vertices and normals, the matrix, global vertex indices
        const int voff = G.voff.back(), nv = me.vertices ? me.n_vertices : 0;
        if ((size_t)voff + (size_t)nv > (size_t)0x7fffffff) return reject("pt_create: too many vertices");
        for (int v = 0; v < nv; ++v) {
            G.verts.push_back(make_float4(me.vertices[3 * v], me.vertices[3 * v + 1], me.vertices[3 * v + 2], 0.0f));
            G.norms.push_back(me.normals
                                  ? make_float4(me.normals[3 * v], me.normals[3 * v + 1], me.normals[3 * v + 2], 0.0f)
                                  : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        }
        G.voff.push_back(voff + nv);
        G.has_normals.push_back(me.normals ? 1 : 0);
        G.alpha.push_back(me.albedo_tex >= 0 ? 1 : 0);
        G.model.insert(G.model.end(), me.model_matrix, me.model_matrix + 16);
        G.normal_rows(m, &mats[(size_t)kMatStride * (size_t)m]);
        for (int i = 0; i < me.n_triangles; ++i) {
            float uv[6] = {0, 0, 0, 0, 0, 0};  // Mesh::texCoord, zeros when absent (Mesh.cpp:50-53)
            int gi[3];
            for (int k = 0; k < 3; ++k) {
                int vi = me.indices[3 * i + k];
                if (vi < 0 || vi >= me.n_vertices) return reject("pt_create: index out of range");
                if (me.texcoords) {
                    uv[2 * k] = me.texcoords[2 * vi];
                    uv[2 * k + 1] = me.texcoords[2 * vi + 1];
                }
                gi[k] = voff + vi;
            }
            G.tidx.push_back(make_int4(gi[0], gi[1], gi[2], m));
            if (any_tex) {
                G.uvs.push_back(make_float4(uv[0], uv[1], uv[2], uv[3]));
                G.uvs.push_back(make_float4(uv[4], uv[5], 0.0f, 0.0f));
            }
        }
    }
    G_out = std::move(G);
    mats_out = std::move(mats);
    texinfo_out = std::move(texinfo);
    *ntexel_out = ntexel;
    *any_tex_out = any_tex;
    return PT_OK;
}

// The bake: world-space triangle soup in original order (modelMatrix * vec4(v, 1); normals with
// w = 0) with its w tags, and the centroid bounds.  pt_create and the rebuild path of
// pt_commit_geometry both call it; k_rebake (pt_refit.hip) runs the same arithmetic per triangle.
void bake_scene(const GeomHost& G, std::vector<float4>& tri, std::vector<float4>& nrm, float cmin[3], float cmax[3]) {
    const size_t ntri = G.tidx.size(), nv = G.verts.size();
    tri.resize(3 * ntri);
    nrm.resize(3 * ntri);
    std::vector<float> wv(3 * nv), wn(3 * nv, 0.0f);
    for (int m = 0; m < G.n_meshes(); ++m) {
        const float* M = &G.model[16 * (size_t)m];
        for (int v = G.voff[(size_t)m]; v < G.voff[(size_t)m + 1]; ++v) {
            const float4 p = G.verts[(size_t)v];
            float in4[4] = {p.x, p.y, p.z, 1.0f}, o4[4];
            xform4(M, in4, o4);
            wv[3 * (size_t)v] = o4[0];
            wv[3 * (size_t)v + 1] = o4[1];
            wv[3 * (size_t)v + 2] = o4[2];
            const int mode = G.normal_mode(m);
            if (mode != 0) {
                const float4 q = G.norms[(size_t)v];
                float n4[4] = {q.x, q.y, q.z, 0.0f};
                o4[0] = q.x, o4[1] = q.y, o4[2] = q.z;  // kNormalObject: reconstruct applies the matrix
                if (mode == 1) xform4(M, n4, o4);
                wn[3 * (size_t)v] = o4[0];
                wn[3 * (size_t)v + 1] = o4[1];
                wn[3 * (size_t)v + 2] = o4[2];
            }
        }
    }
    for (int a = 0; a < 3; ++a) {
        cmin[a] = INFINITY;
        cmax[a] = -INFINITY;
    }
    for (size_t t = 0; t < ntri; ++t) {
        const int4 id = G.tidx[t];
        const int vi3[3] = {id.x, id.y, id.z}, m = id.w;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 3; ++k) {
            const size_t vi = (size_t)vi3[k];
            float wbits;
            // w tags: v0 = original triangle index, v1 = mesh, v2 = alpha cut-out flag
            int tag = (k == 0) ? (int)t : (k == 1 ? m : G.alpha[(size_t)m]);
            std::memcpy(&wbits, &tag, 4);
            tri[3 * t + k] = make_float4(wv[3 * vi], wv[3 * vi + 1], wv[3 * vi + 2], wbits);
            nrm[3 * t + k] = make_float4(wn[3 * vi], wn[3 * vi + 1], wn[3 * vi + 2], 0.0f);
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], wv[3 * vi + a]);
                hi[a] = std::max(hi[a], wv[3 * vi + a]);
            }
        }
        for (int a = 0; a < 3; ++a) {
            float c = 0.5f * (lo[a] + hi[a]);
            cmin[a] = std::min(cmin[a], c);
            cmax[a] = std::max(cmax[a], c);
        }
    }
}

}  // namespace pt
