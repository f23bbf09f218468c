// Host check of the part of pt_create that reads the caller's memory (pt_capi_bake.cpp:
// ingest_scene, GeomHost::normal_mode, bake_scene).  Compiled host-only; no GPU.
//
//   scene_ingest_check rejections | normal_mode | bake
//
// Prints one line per failed check and "checks=<n> bad=<m>"; exits 1 when m > 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pt_renderer.h"

using namespace pt;

namespace {

int g_checks = 0, g_bad = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++g_checks;                                                      \
        if (!(cond)) {                                                   \
            ++g_bad;                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
        }                                                                \
    } while (0)

// A mesh that owns its arrays; c() is the view pt_create takes.
struct Mesh {
    std::vector<float> v, n, uv;
    std::vector<int32_t> idx;
    float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int albedo_tex = -1, normal_tex = -1, mr_tex = -1;
    pt_mesh c() const {
        pt_mesh m{};
        m.vertices = v.empty() ? nullptr : v.data();
        m.normals = n.empty() ? nullptr : n.data();
        m.texcoords = uv.empty() ? nullptr : uv.data();
        m.indices = idx.empty() ? nullptr : idx.data();
        m.n_vertices = (int32_t)(v.size() / 3);
        m.n_triangles = (int32_t)(idx.size() / 3);
        std::memcpy(m.model_matrix, M, sizeof M);
        m.albedo[0] = 0.5f, m.albedo[1] = 0.25f, m.albedo[2] = 0.75f;
        m.metallic = 0.0f;
        m.roughness = 0.5f;
        m.albedo_tex = albedo_tex;
        m.normal_tex = normal_tex;
        m.metal_rough_tex = mr_tex;
        return m;
    }
};

// column-major matrix from rows (the fourth row is 0 0 0 1)
void set_rows(float* M, const float r0[4], const float r1[4], const float r2[4]) {
    const float* rows[3] = {r0, r1, r2};
    for (int c = 0; c < 4; ++c) {
        for (int r = 0; r < 3; ++r) M[4 * c + r] = rows[r][c];
        M[4 * c + 3] = c == 3 ? 1.0f : 0.0f;
    }
}

// a quad of two triangles (small integers and halves) with per-vertex axis normals
Mesh quad(float z, bool normals) {
    Mesh m;
    m.v = {-1.0f, -0.5f, z, 2.0f, -0.5f, z, 2.0f, 1.5f, z, -1.0f, 1.5f, z};
    if (normals) m.n = {0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, -1};
    m.idx = {0, 1, 2, 0, 2, 3};
    return m;
}

struct Ingested {
    GeomHost G;
    std::vector<float4> mats;
    std::vector<int4> texinfo;
    size_t ntexel = 0;
    bool any_tex = false;
    std::string err;
    int rc = 0;
};

Ingested ingest(const std::vector<Mesh>& meshes, const std::vector<pt_texture>& tex = {}) {
    std::vector<pt_mesh> cm;
    for (const Mesh& m : meshes) cm.push_back(m.c());
    pt_scene sc{};
    sc.meshes = cm.empty() ? nullptr : cm.data();
    sc.n_meshes = (int32_t)cm.size();
    sc.textures = tex.empty() ? nullptr : tex.data();
    sc.n_textures = (int32_t)tex.size();
    Ingested o;
    o.rc = ingest_scene(&sc, o.G, o.mats, o.texinfo, &o.ntexel, &o.any_tex, &o.err);
    return o;
}

// The status and the message of a rejected scene, and that no output was touched.
void expect_rejected(std::vector<pt_mesh> cm, int n_textures, const pt_texture* tex, const char* msg) {
    pt_scene sc{};
    sc.meshes = cm.data();
    sc.n_meshes = (int32_t)cm.size();
    sc.textures = tex;
    sc.n_textures = n_textures;
    GeomHost G;
    G.voff = {7, 8};
    G.alpha = {3};
    std::vector<float4> mats(5, make_float4(1, 2, 3, 4));
    std::vector<int4> texinfo(2, make_int4(9, 9, 9, 9));
    size_t ntexel = 1234;
    bool any_tex = true;
    std::string err;
    const int rc = ingest_scene(&sc, G, mats, texinfo, &ntexel, &any_tex, &err);
    CHECK(rc == PT_ERR_INVALID);
    CHECK(err == msg);
    CHECK(G.voff.size() == 2 && G.voff[0] == 7 && G.voff[1] == 8 && G.alpha.size() == 1 && G.alpha[0] == 3);
    CHECK(G.verts.empty() && G.norms.empty() && G.tidx.empty() && G.model.empty() && G.has_normals.empty() && G.uvs.empty());
    CHECK(mats.size() == 5 && mats[4].w == 4.0f);
    CHECK(texinfo.size() == 2 && texinfo[1].x == 9);
    CHECK(ntexel == 1234 && any_tex);
}

void check_rejections() {
    const uint32_t texel = 0xff00ff00u;
    const pt_texture tex{&texel, 1, 1};
    // three meshes, the fault in the last: the first two have been read by then
    const Mesh a = quad(0.0f, true), b = quad(1.0f, false), c = quad(2.0f, true);
    const std::vector<pt_mesh> good = {a.c(), b.c(), c.c()};
    {
        std::vector<pt_mesh> s = good;
        s[2].n_triangles = -1;
        expect_rejected(s, 0, nullptr, "pt_create: negative counts");
        s = good;
        s[2].n_vertices = -1;
        expect_rejected(s, 0, nullptr, "pt_create: negative counts");
    }
    {
        Mesh bad = c;
        bad.idx[4] = 4;  // == n_vertices
        expect_rejected({a.c(), b.c(), bad.c()}, 0, nullptr, "pt_create: index out of range");
        bad.idx[4] = -1;
        expect_rejected({a.c(), b.c(), bad.c()}, 0, nullptr, "pt_create: index out of range");
    }
    {
        std::vector<pt_mesh> s = good;
        s[2].albedo_tex = 1;  // == n_textures
        expect_rejected(s, 1, &tex, "pt_create: texture id out of range");
        s = good;
        s[2].metal_rough_tex = 0;  // == n_textures of a scene without textures
        expect_rejected(s, 0, nullptr, "pt_create: texture id out of range");
    }
    {
        std::vector<pt_mesh> s = good;
        s[2].indices = nullptr;
        expect_rejected(s, 0, nullptr, "pt_create: mesh without vertices/indices");
    }
    {  // one mesh
        std::vector<pt_mesh> s = {a.c()};
        s[0].n_triangles = -2;
        expect_rejected(s, 0, nullptr, "pt_create: negative counts");
    }
}

void check_normal_mode() {
    const float s2 = std::sqrt(0.5f);
    const float I0[4] = {1, 0, 0, 0}, I1[4] = {0, 1, 0, 0}, I2[4] = {0, 0, 1, 0};
    const float P0[4] = {0, 0, -1, 0}, P1[4] = {1, 0, 0, 0}, P2[4] = {0, -1, 0, 0};  // signed axis permutation
    const float T0[4] = {1, 0, 0, 3}, T1[4] = {0, 1, 0, -2}, T2[4] = {0, 0, 1, 5};   // pure translation
    const float R0[4] = {s2, -s2, 0, 0}, R1[4] = {s2, s2, 0, 0};                      // 45 degrees about z
    const float S0[4] = {2 * s2, -3 * s2, 0, 1}, S1[4] = {2 * s2, 3 * s2, 0, 0}, S2[4] = {0, 0, 0.5f, 0};  // R * diag(2,3,.5)
    struct Case {
        const float *r0, *r1, *r2;
        bool normals;
        int mode;
    };
    const Case first[3] = {{I0, I1, I2, false, 0}, {I0, I1, I2, true, 1}, {P0, P1, P2, true, 1}};
    const Case second[3] = {{T0, T1, T2, true, 1}, {R0, R1, I2, true, 2}, {S0, S1, S2, true, 2}};
    for (const Case* cases : {first, second}) {
        std::vector<Mesh> meshes;
        for (int k = 0; k < 3; ++k) {
            meshes.push_back(quad((float)k, cases[k].normals));
            set_rows(meshes.back().M, cases[k].r0, cases[k].r1, cases[k].r2);
        }
        const Ingested o = ingest(meshes);
        CHECK(o.rc == PT_OK && o.err.empty());
        CHECK(o.G.n_meshes() == 3 && o.mats.size() == 3 * (size_t)kMatStride);
        for (int k = 0; k < 3 && o.rc == PT_OK; ++k) {
            CHECK(o.G.normal_mode(k) == cases[k].mode);
            const float4* rec = &o.mats[(size_t)kMatStride * (size_t)k];
            CHECK(rec[1].y == (float)cases[k].mode);
            const float* rows[3] = {cases[k].r0, cases[k].r1, cases[k].r2};
            for (int r = 0; r < 3; ++r)
                CHECK(rec[3 + r].x == rows[r][0] && rec[3 + r].y == rows[r][1] && rec[3 + r].z == rows[r][2] &&
                      rec[3 + r].w == rows[r][3]);
        }
    }
}

int bits(float f) {
    int i;
    std::memcpy(&i, &f, 4);
    return i;
}

// bake_scene against positions, normals, tags and centroid bounds computed here in double (every
// product and sum of the scenes below is exact in fp32, so the order of operations cannot matter)
void check_baked(const std::vector<Mesh>& meshes, const Ingested& o) {
    std::vector<float4> tri, nrm;
    float cmin[3], cmax[3];
    bake_scene(o.G, tri, nrm, cmin, cmax);
    size_t ntri = 0;
    for (const Mesh& m : meshes) ntri += m.idx.size() / 3;
    CHECK(tri.size() == 3 * ntri && nrm.size() == 3 * ntri && o.G.tidx.size() == ntri);
    if (tri.size() != 3 * ntri || nrm.size() != 3 * ntri) return;
    double emin[3] = {INFINITY, INFINITY, INFINITY}, emax[3] = {-INFINITY, -INFINITY, -INFINITY};
    size_t t = 0;
    for (size_t mi = 0; mi < meshes.size(); ++mi) {
        const Mesh& m = meshes[mi];
        const int mode = o.G.normal_mode((int)mi);
        for (size_t i = 0; i < m.idx.size() / 3; ++i, ++t) {
            double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int k = 0; k < 3; ++k) {
                const int vi = m.idx[3 * i + (size_t)k];
                const float4 p = tri[3 * t + (size_t)k], q = nrm[3 * t + (size_t)k];
                const float got[3] = {p.x, p.y, p.z}, gotn[3] = {q.x, q.y, q.z};
                for (int r = 0; r < 3; ++r) {
                    double w = m.M[12 + r], wn = 0.0;
                    for (int c = 0; c < 3; ++c) {
                        w += (double)m.M[4 * c + r] * (double)m.v[3 * (size_t)vi + (size_t)c];
                        if (mode != 0) wn += (double)m.M[4 * c + r] * (double)m.n[3 * (size_t)vi + (size_t)c];
                    }
                    if (mode == 2) wn = m.n[3 * (size_t)vi + (size_t)r];  // left in object space
                    CHECK((double)got[r] == w);
                    CHECK((double)gotn[r] == wn);
                    lo[r] = std::min(lo[r], w);
                    hi[r] = std::max(hi[r], w);
                }
                const int tag = k == 0 ? (int)t : (k == 1 ? (int)mi : (m.albedo_tex >= 0 ? 1 : 0));
                CHECK(bits(p.w) == tag);
                CHECK(q.w == 0.0f);
            }
            for (int r = 0; r < 3; ++r) {
                emin[r] = std::min(emin[r], 0.5 * (lo[r] + hi[r]));
                emax[r] = std::max(emax[r], 0.5 * (lo[r] + hi[r]));
            }
        }
    }
    for (int r = 0; r < 3; ++r) CHECK((double)cmin[r] == emin[r] && (double)cmax[r] == emax[r]);
}

void check_bake() {
    {  // no meshes
        const Ingested o = ingest({});
        CHECK(o.rc == PT_OK && o.G.n_meshes() == 0 && o.G.voff.size() == 1 && o.mats.size() == (size_t)kMatStride);
        CHECK(!o.any_tex && o.ntexel == 0 && o.G.uvs.empty());
        check_baked({}, o);
    }
    {  // one mesh whose matrix keeps its normals in object space: a permutation scaled by 2
        Mesh m = quad(0.5f, true);
        const float r0[4] = {0, 2, 0, -3}, r1[4] = {0, 0, -2, 4}, r2[4] = {2, 0, 0, 1};
        set_rows(m.M, r0, r1, r2);
        const Ingested o = ingest({m});
        CHECK(o.rc == PT_OK && o.G.normal_mode(0) == 2 && !o.any_tex);
        check_baked({m}, o);
    }
    {  // three meshes: a signed permutation with normals; one without vertices; a textured one without normals
        Mesh a = quad(-1.5f, true);
        const float a0[4] = {0, 0, -1, 2}, a1[4] = {1, 0, 0, -7}, a2[4] = {0, -1, 0, 3};
        set_rows(a.M, a0, a1, a2);
        a.v.insert(a.v.end(), {0.5f, 3.0f, -2.0f});  // 5 vertices, 3 triangles
        a.n.insert(a.n.end(), {0, -1, 0});
        a.idx.insert(a.idx.end(), {4, 0, 2});
        Mesh b;  // no vertices, no triangles
        Mesh c = quad(2.0f, false);
        const float c0[4] = {-1, 0, 0, 0}, c1[4] = {0, 0, 1, 5}, c2[4] = {0, 1, 0, -4};
        set_rows(c.M, c0, c1, c2);
        c.uv = {0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 1.0f, 0.0f, 1.0f};
        c.albedo_tex = 1;
        const uint32_t texels[6] = {1, 2, 3, 4, 5, 6};
        const std::vector<pt_texture> tex = {{texels, 2, 1}, {texels + 2, 2, 2}};
        const Ingested o = ingest({a, b, c}, tex);
        CHECK(o.rc == PT_OK && o.any_tex && o.ntexel == 6);
        CHECK(o.texinfo.size() == 2 && o.texinfo[0].x == 0 && o.texinfo[1].x == 2 && o.texinfo[1].y == 2 && o.texinfo[1].z == 2);
        CHECK(o.G.voff == std::vector<int>({0, 5, 5, 9}));
        CHECK(o.G.has_normals == std::vector<int>({1, 0, 0}) && o.G.alpha == std::vector<int>({0, 0, 1}));
        CHECK(o.G.normal_mode(0) == 1 && o.G.normal_mode(1) == 0 && o.G.normal_mode(2) == 0);
        CHECK(o.G.tidx.size() == 5 && o.G.tidx[3].x == 5 && o.G.tidx[3].z == 7 && o.G.tidx[3].w == 2);
        CHECK(o.G.uvs.size() == 10 && o.G.uvs[0].x == 0.0f && o.G.uvs[0].z == 0.0f);  // mesh a: zeros
        CHECK(o.G.uvs[6].z == 1.0f && o.G.uvs[6].w == 0.0f && o.G.uvs[7].x == 1.0f && o.G.uvs[7].y == 1.0f);
        CHECK(bits(o.mats[(size_t)kMatStride * 2 + 1].z) == 1 && o.mats[(size_t)kMatStride * 2 + 2].y == 1.0f);
        check_baked({a, b, c}, o);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "rejections") check_rejections();
    else if (what == "normal_mode") check_normal_mode();
    else if (what == "bake") check_bake();
    else {
        std::printf("usage: scene_ingest_check rejections|normal_mode|bake\n");
        return 2;
    }
    std::printf("checks=%d bad=%d\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
