// Compile-and-link check of the feature-buffer and denoiser methods of include/OptixRenderer.hpp
// (Aov, AovPrim, Denoise, DenoiseInfo) against stand-in types shaped like the reference's, as
// facade_geometry_check.cpp does for the geometry updates.  Without a GPU the constructor must
// throw (exit code 2, "no HIP device"); with one, the triangle must cover some pixels and not
// others, an all-ones image must come back all ones, the miss pixels of the filtered mean must
// equal the mean's, and the three calls must have rendered the G-buffer once.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "OptixRenderer.hpp"

namespace stand_in {
struct vec2 { float x, y; };
struct vec3 { float x, y, z; };
struct ivec2 { int x, y; };
struct ivec3 { int x, y, z; };
struct mat4 {
    float c[4][4];
    const float* operator[](int i) const { return c[i]; }
};
inline mat4 identity() {
    mat4 m{};
    for (int i = 0; i < 4; ++i) m.c[i][i] = 1.0f;
    return m;
}
struct Mesh {
    std::vector<vec3> vertecies, normal;
    std::vector<vec2> texCoord;
    std::vector<ivec3> index;
    vec3 albedo{0.5f, 0.5f, 0.5f};
    float metallic = 0.0f, roughness = 0.5f;
    int albedoTex = -1, normalTex = -1, metalRoughTex = -1;
    mat4 GetModelMatrix() const { return identity(); }
};
struct Texture {
    uint32_t* pixel = nullptr;
    ivec2 resolution{-1, -1};
};
struct Model {
    std::vector<std::unique_ptr<Mesh>> meshes;
    std::vector<std::unique_ptr<Texture>> textures;
};
struct PointLight {
    vec3 position, color;
};
struct Camera {
    vec3 position{0, 0, 3};
    mat4 GetViewMatrix() const {
        mat4 m = identity();
        m.c[3][2] = -3.0f;
        return m;
    }
    mat4 GetProjectionMatrix(float aspect) const {
        mat4 m{};
        m.c[0][0] = 1.0f / aspect;
        m.c[1][1] = 1.0f;
        m.c[2][2] = -1.002f;
        m.c[2][3] = -1.0f;
        m.c[3][2] = -0.2002f;
        return m;
    }
};
}  // namespace stand_in

int main() {
    using namespace stand_in;
    Model model;
    auto m = std::make_unique<Mesh>();
    m->vertecies = {{-1, -1, 0}, {1, -1, 0}, {0, 1, 0}};
    m->normal = {{0, 0, 1}, {0, 0, 1}, {0, 0, 1}};
    m->index = {{0, 1, 2}};
    model.meshes.push_back(std::move(m));
    try {
        ptamd::OptixRendererT<Model> r("ignored.ptx", &model, PT_MAT_LAMBERT);
        ivec2 size{16, 12};
        const size_t n = 16 * 12;
        r.Resize(size);
        Camera cam;
        r.SetCamera(&cam);
        std::vector<PointLight> lights = {{{0, 0, 2}, {1, 1, 1}}};
        r.SetLights(&lights);
        r.SetMaxBounces(2);
        std::vector<vec3> mean(n), filtered(n), ones(n, vec3{1, 1, 1}), ones_out(n);
        r.RenderAccumulate(4, 1, mean.data());
        const std::vector<int32_t> prim = r.AovPrim();
        const std::vector<float> depth = r.Aov(PT_AOV_DEPTH);
        r.Denoise(filtered.data(), 0.25f);
        pt_denoise_options opt = ptamd::OptixRendererT<Model>::DenoiseDefaults();
        opt.iterations = 3;
        r.Denoise(ones.data(), ones_out.data(), &opt);
        const pt_denoise_info info = r.DenoiseInfo();
        size_t hits = 0;
        bool miss_kept = true, depth_ok = true;
        for (size_t i = 0; i < n; ++i) {
            if (prim[i] >= 0) ++hits;
            else miss_kept = miss_kept && std::memcmp(&mean[i], &filtered[i], sizeof(vec3)) == 0;
            depth_ok = depth_ok && (prim[i] >= 0 ? depth[i] > 0.0f : depth[i] == 0.0f);
        }
        const bool ones_kept = std::memcmp(ones.data(), ones_out.data(), sizeof(vec3) * n) == 0;
        const bool info_ok = info.gbuffer_renders == 1 && info.hit_pixels == hits && info.iterations == 3;
        std::printf("hits=%zu of %zu miss kept=%d depth=%d ones kept=%d info=%d\n", hits, n, miss_kept ? 1 : 0,
                    depth_ok ? 1 : 0, ones_kept ? 1 : 0, info_ok ? 1 : 0);
        return (hits > 0 && hits < n && miss_kept && depth_ok && ones_kept && info_ok) ? 0 : 3;
    } catch (const std::exception& e) {
        std::printf("threw: %s\n", e.what());
        return 2;
    }
}
