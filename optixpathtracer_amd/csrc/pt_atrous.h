// pt_atrous.h — what the image-space kernels of pt_aov.hip (G-buffer, a-trous filter) and
// pt_temporal.hip (temporal reprojection, variance-guided a-trous) share: the pixel tiling and the
// small exact functions that DESIGN.md §10 and §11 name.  Device code only.
#pragma once
#include "pt_internal.h"

namespace pt {
namespace {

constexpr int kBlock = 256;
constexpr int kTile = 16;  // pixels per workgroup side

__device__ __forceinline__ void tile_pixel(int& x, int& y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = blockIdx.x * kTile + (wave & 1) * 8 + (lane & 7);
    y = blockIdx.y * kTile + (wave >> 1) * 8 + (lane >> 3);
}

__device__ __forceinline__ void store3(float* p, size_t i, f3 v) {
    p[3 * i] = v.x;
    p[3 * i + 1] = v.y;
    p[3 * i + 2] = v.z;
}

// a_p = max(albedo[p], floor) per channel
__device__ __forceinline__ f3 albedo_floor(float4 a, float floor) {
    return mk(a.x < floor ? floor : a.x, a.y < floor ? floor : a.y, a.z < floor ? floor : a.z);
}

__device__ __forceinline__ float d2(float4 q, float4 p) {
    const float x = q.x - p.x, y = q.y - p.y, z = q.z - p.z;
    return (x * x + y * y) + z * z;
}

__device__ __forceinline__ float b3(int i) {  // h = [1/16, 1/4, 3/8, 1/4, 1/16]
    return i == 2 ? 0.375f : (i == 1 || i == 3) ? 0.25f : 0.0625f;
}

inline dim3 tile_grid(int w, int h) { return dim3((unsigned)((w + kTile - 1) / kTile), (unsigned)((h + kTile - 1) / kTile)); }

}  // namespace
}  // namespace pt
