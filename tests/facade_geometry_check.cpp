// Compile-and-link check of the geometry-update methods of include/OptixRenderer.hpp
// (SetMeshTransform, UpdateMeshVertices, CommitGeometry) against stand-in types shaped like the
// reference's, as facade_compile_check.cpp does for the rest.  Without a GPU the constructor must
// throw (exit code 2, "no HIP device"); with one, a moved triangle must change the image, and a
// refit and a rebuild of the same move must give the same image.
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
        ivec2 size{8, 8};
        r.Resize(size);
        Camera cam;
        r.SetCamera(&cam);
        std::vector<PointLight> lights = {{{0, 0, 2}, {1, 1, 1}}};
        r.SetLights(&lights);
        r.SetMaxBounces(2);
        std::vector<vec3> before(64), staged(64), refit(64), rebuilt(64), squashed(64);
        r.RenderAccumulate(2, 1, before.data());
        mat4 move = identity();
        move.c[3][0] = 0.4f;  // translate along x
        r.SetMeshTransform(0, move);
        r.RenderAccumulate(2, 1, staged.data());  // staged only: the old geometry renders
        r.CommitGeometry();
        r.RenderAccumulate(2, 1, refit.data());
        r.SetMeshTransform(0, move);
        r.CommitGeometry(true);
        r.RenderAccumulate(2, 1, rebuilt.data());
        std::vector<vec3> verts = {{-1, -0.5f, 0}, {1, -0.5f, 0}, {0, 0.5f, 0}};
        r.UpdateMeshVertices(0, verts, std::vector<vec3>());  // keeps the normals
        r.CommitGeometry();
        r.RenderAccumulate(2, 1, squashed.data());
        const size_t bytes = sizeof(vec3) * before.size();
        const bool staged_same = std::memcmp(before.data(), staged.data(), bytes) == 0;
        const bool moved = std::memcmp(before.data(), refit.data(), bytes) != 0;
        const bool same = std::memcmp(refit.data(), rebuilt.data(), bytes) == 0;
        const bool reshaped = std::memcmp(rebuilt.data(), squashed.data(), bytes) != 0;
        std::printf("staged unchanged=%d moved=%d refit==rebuild=%d reshaped=%d\n", staged_same ? 1 : 0, moved ? 1 : 0,
                    same ? 1 : 0, reshaped ? 1 : 0);
        return (staged_same && moved && same && reshaped) ? 0 : 3;
    } catch (const std::exception& e) {
        std::printf("threw: %s\n", e.what());
        return 2;
    }
}
