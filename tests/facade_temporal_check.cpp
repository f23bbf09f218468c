// Compile-and-link check of the temporal-filter methods of include/OptixRenderer.hpp
// (TemporalDefaults, DenoiseTemporal, TemporalReset, TemporalState, TemporalInfo) against stand-in
// types shaped like the reference's, as facade_denoise_check.cpp does for the denoiser.  Without a
// GPU the constructor must throw (exit code 2, "no HIP device"); with one, a first call must start
// every hit pixel at length 1, a second call from the same camera must take up history at all of
// them, a reset must start them again, and the miss pixels must come back as they went in.
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
        std::vector<vec3> mean(n), filtered(n), half(n, vec3{0.5f, 0.5f, 0.5f}), half_out(n);
        r.RenderAccumulate(4, 1, mean.data());
        r.DenoiseTemporal(filtered.data(), 0.25f);
        const pt_temporal_info first = r.TemporalInfo();
        const std::vector<float> len1 = r.TemporalState(PT_TEMPORAL_HISTORY_LENGTH);
        pt_temporal_options topt = ptamd::OptixRendererT<Model>::TemporalDefaults();
        topt.max_history = 8;
        pt_denoise_options opt = ptamd::OptixRendererT<Model>::DenoiseDefaults();
        opt.iterations = 3;
        r.DenoiseTemporal(half.data(), half_out.data(), &topt, &opt);
        const pt_temporal_info second = r.TemporalInfo();
        const std::vector<float> moments = r.TemporalState(PT_TEMPORAL_MOMENTS);
        r.TemporalReset();
        const bool dropped = r.TemporalInfo().history_valid == 0;
        r.DenoiseTemporal(half.data(), half_out.data());
        const pt_temporal_info third = r.TemporalInfo();
        const std::vector<int32_t> prim = r.AovPrim();
        size_t hits = 0;
        bool miss_kept = true, len_ok = true;
        for (size_t i = 0; i < n; ++i) {
            if (prim[i] >= 0) ++hits;
            else miss_kept = miss_kept && std::memcmp(&mean[i], &filtered[i], sizeof(vec3)) == 0;
            len_ok = len_ok && len1[i] == (prim[i] >= 0 ? 1.0f : 0.0f);
        }
        const bool first_ok = first.calls == 1 && first.history_valid == 1 && first.reprojected_pixels == 0 &&
                              first.reset_pixels == hits;
        const bool second_ok = second.calls == 2 && second.reprojected_pixels == hits && second.reset_pixels == 0;
        const bool third_ok = dropped && third.calls == 3 && third.reprojected_pixels == 0 && third.reset_pixels == hits;
        std::printf("hits=%zu of %zu miss kept=%d lengths=%d first=%d second=%d third=%d moments=%zu\n", hits, n,
                    miss_kept ? 1 : 0, len_ok ? 1 : 0, first_ok ? 1 : 0, second_ok ? 1 : 0, third_ok ? 1 : 0, moments.size());
        return (hits > 0 && hits < n && miss_kept && len_ok && first_ok && second_ok && third_ok && moments.size() == 2 * n)
                   ? 0
                   : 3;
    } catch (const std::exception& e) {
        std::printf("threw: %s\n", e.what());
        return 2;
    }
}
