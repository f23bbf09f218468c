// Compile-and-link check of the motion-vector surface of include/OptixRenderer.hpp (Motion,
// pt_temporal_options.motion_vectors, the new pt_temporal_info fields) against stand-in types shaped
// like the reference's, as facade_temporal_check.cpp does for the temporal filter.  Without a GPU
// the constructor must throw (exit code 2, "no HIP device"); with one: a first call with the option
// on has no history, a second without a commit runs the plain kernel, and after the triangle is
// slid by 0.1 in its plane a third runs the motion kernel, counts every hit pixel as moved, takes up
// history and reports where each point was.
#include <cmath>
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
        using R = ptamd::OptixRendererT<Model>;
        R r("ignored.ptx", &model, PT_MAT_LAMBERT);
        ivec2 size{16, 12};
        const size_t n = 16 * 12;
        r.Resize(size);
        Camera cam;
        r.SetCamera(&cam);
        std::vector<PointLight> lights = {{{0, 0, 2}, {1, 1, 1}}};
        r.SetLights(&lights);
        r.SetMaxBounces(2);
        std::vector<vec3> half(n, vec3{0.5f, 0.5f, 0.5f}), out(n);
        pt_temporal_options topt = R::TemporalDefaults();
        const bool default_off = topt.motion_vectors == 0;
        topt.motion_vectors = 1;
        r.DenoiseTemporal(half.data(), out.data(), &topt);
        const pt_temporal_info first = r.TemporalInfo();
        r.DenoiseTemporal(half.data(), out.data(), &topt);
        const pt_temporal_info second = r.TemporalInfo();
        mat4 slide = identity();
        slide.c[3][0] = 0.1f;
        r.SetMeshTransform(0, slide);
        r.CommitGeometry();
        r.DenoiseTemporal(half.data(), out.data(), &topt);
        const pt_temporal_info third = r.TemporalInfo();
        const std::vector<int32_t> prim = r.AovPrim();
        const std::vector<float> pos = r.Aov(PT_AOV_POSITION), bary = r.Motion(PT_MOTION_BARYCENTRIC),
                                 pp = r.Motion(PT_MOTION_PREV_POSITION), screen = r.Motion(PT_MOTION_SCREEN);
        size_t hits = 0;
        bool where_ok = pp.size() == 3 * n && screen.size() == 3 * n && bary.size() == 2 * n;
        for (size_t i = 0; where_ok && i < n; ++i) {
            if (prim[i] >= 0) {
                ++hits;
                where_ok = std::fabs(pp[3 * i] - (pos[3 * i] - 0.1f)) < 1e-5f && pp[3 * i + 1] == pos[3 * i + 1] &&
                           screen[3 * i + 2] == 1.0f && screen[3 * i] < 0.0f && bary[2 * i] >= 0.0f && bary[2 * i + 1] >= 0.0f;
            } else {
                where_ok = pp[3 * i] == 0.0f && screen[3 * i + 2] == 0.0f && bary[2 * i] == 0.0f;
            }
        }
        const bool first_ok = first.motion_used == 0 && first.moved_pixels == 0 && first.snapshot_ms > 0.0;
        const bool second_ok = second.motion_used == 0 && second.snapshot_ms == 0.0 && second.reset_pixels == 0;
        const bool third_ok = third.motion_used == 1 && third.moved_pixels == hits && third.reprojected_pixels + third.reset_pixels == hits &&
                              third.reprojected_pixels > 0 && third.snapshot_ms > 0.0;
        std::printf("hits=%zu of %zu default off=%d first=%d second=%d third=%d (moved=%llu reprojected=%llu) where=%d\n", hits, n,
                    default_off ? 1 : 0, first_ok ? 1 : 0, second_ok ? 1 : 0, third_ok ? 1 : 0,
                    (unsigned long long)third.moved_pixels, (unsigned long long)third.reprojected_pixels, where_ok ? 1 : 0);
        return (hits > 0 && hits < n && default_off && first_ok && second_ok && third_ok && where_ok) ? 0 : 3;
    } catch (const std::exception& e) {
        std::printf("threw: %s\n", e.what());
        return 2;
    }
}
