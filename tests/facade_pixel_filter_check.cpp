// Compile-and-link check of the anti-aliasing methods of include/OptixRenderer.hpp (SetPixelFilter,
// PixelFilter) against stand-in types shaped like the reference's, as facade_adaptive_check.cpp does
// for adaptive sampling.  Without a GPU the constructor must throw (exit code 2, "no HIP device");
// with one, a triangle in front of a black background: the setting reads back resolved, 16 frames
// under supersample 4 differ from 16 pixel-centre frames only along the triangle's edges (the
// background corner stays black), a tent-filtered mean is finite, and back at the default the render
// has the bits it had before.
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
        const pt_pixel_filter d = r.PixelFilter();
        const bool default_ok = d.supersample == 1 && d.kind == PT_FILTER_BOX && d.radius == 0.5f;
        std::vector<vec3> plain(n), aa(n), tent(n), restored(n);
        r.RenderAccumulate(16, 1, plain.data());
        r.SetPixelFilter(4);
        r.RenderAccumulate(16, 1, aa.data());
        r.SetPixelFilter(4, PT_FILTER_TENT);
        const pt_pixel_filter t = r.PixelFilter();
        const bool resolved_ok = t.supersample == 4 && t.kind == PT_FILTER_TENT && t.radius == 1.0f;
        r.RenderAccumulate(16, 1, tent.data());
        r.SetPixelFilter();
        r.RenderAccumulate(16, 1, restored.data());
        size_t differ = 0;
        bool finite_ok = true;
        for (size_t i = 0; i < n; ++i) {
            differ += std::memcmp(&plain[i], &aa[i], sizeof(vec3)) != 0 ? 1 : 0;
            finite_ok = finite_ok && tent[i].x == tent[i].x && tent[i].x >= 0.0f && tent[i].x < 1e6f;
        }
        const bool edges_ok = differ > 0 && differ < n / 2;
        const bool corner_ok = plain[0].x == 0.0f && aa[0].x == 0.0f && tent[0].x == 0.0f;
        const bool restored_ok = std::memcmp(plain.data(), restored.data(), n * sizeof(vec3)) == 0;
        std::printf("differ=%zu default=%d resolved=%d edges=%d finite=%d corner=%d restored=%d\n", differ,
                    default_ok ? 1 : 0, resolved_ok ? 1 : 0, edges_ok ? 1 : 0, finite_ok ? 1 : 0, corner_ok ? 1 : 0,
                    restored_ok ? 1 : 0);
        return (default_ok && resolved_ok && edges_ok && finite_ok && corner_ok && restored_ok) ? 0 : 3;
    } catch (const std::exception& e) {
        std::printf("threw: %s\n", e.what());
        return 2;
    }
}
