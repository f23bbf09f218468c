// Compile-and-link check of the adaptive-sampling methods of include/OptixRenderer.hpp
// (AdaptiveDefaults, RenderAdaptive, AdaptiveSamples, AdaptiveInfo, DenoiseAdaptive) against stand-in
// types shaped like the reference's, as facade_denoise_check.cpp does for the denoiser.  Without a
// GPU the constructor must throw (exit code 2, "no HIP device"); with one, a triangle in front of a
// black background: every count is a multiple of the round within [min, max], the tiles that see
// only the background stop at min_samples, the mean times the count is the sum, and the counts add
// up to what the info reports.
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
        ivec2 size{40, 24};
        const size_t n = 40 * 24;
        r.Resize(size);
        Camera cam;
        r.SetCamera(&cam);
        std::vector<PointLight> lights = {{{0, 0, 2}, {1, 1, 1}}, {{1, 1, 2}, {1, 1, 1}}};
        r.SetLights(&lights);
        r.SetMaxBounces(2);
        pt_adaptive_options opt = ptamd::OptixRendererT<Model>::AdaptiveDefaults();
        const bool defaults_ok = opt.round_frames == 16 && opt.min_samples == 16 && opt.max_samples == 1024;
        opt.round_frames = 4;
        opt.min_samples = 6;  // rounded up to 8
        opt.max_samples = 24;
        opt.threshold = 0.02f;
        std::vector<vec3> mean(n), sum(n), filtered(n);
        r.RenderAdaptive(1, mean.data(), &opt);
        const std::vector<uint32_t> count = r.AdaptiveSamples();
        r.DownloadMean(sum.data(), 1);
        r.DenoiseAdaptive(filtered.data());
        const pt_adaptive_info info = r.AdaptiveInfo();
        uint64_t total = 0;
        uint32_t lo = ~0u, hi = 0;
        bool counts_ok = true, mean_ok = true;
        for (size_t i = 0; i < n; ++i) {
            total += count[i];
            lo = count[i] < lo ? count[i] : lo;
            hi = count[i] > hi ? count[i] : hi;
            counts_ok = counts_ok && count[i] % 4 == 0 && count[i] >= 8 && count[i] <= 24;
            mean_ok = mean_ok && mean[i].x == sum[i].x / (float)count[i];
        }
        const bool corner_ok = count[0] == 8 && mean[0].x == 0.0f;  // the background: no variance
        const bool info_ok = info.samples == total && info.tiles == 15 && info.rounds >= 2 && info.rounds <= 6 &&
                             info.samples_uniform == (uint64_t)n * hi && info.tiles_stopped >= 1;
        std::printf("samples=%llu of %llu counts %u..%u defaults=%d counts=%d mean=%d corner=%d info=%d\n",
                    (unsigned long long)total, (unsigned long long)info.samples_uniform, lo, hi, defaults_ok ? 1 : 0,
                    counts_ok ? 1 : 0, mean_ok ? 1 : 0, corner_ok ? 1 : 0, info_ok ? 1 : 0);
        return (defaults_ok && counts_ok && mean_ok && corner_ok && info_ok) ? 0 : 3;
    } catch (const std::exception& e) {
        std::printf("threw: %s\n", e.what());
        return 2;
    }
}
