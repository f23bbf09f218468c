// pt_filter.hip — the filtered accumulation of pt_set_pixel_filter (pt_capi_filter.cpp).
//
// k_accum_filtered<R>: k_accum for a launch whose pixel filter is wider than the box.  The sample
// of frame F sits in cell c = F mod ss^2 of its pixel, and the frame's filtered image is, per output
// pixel (X, Y) in fp32 without contraction,
//     g = 0;  for j = -R..R: for i = -R..R:  g = g + (wy[j] * wx[i]) * L_F(clamp(X + i), clamp(Y + j))
// with the cell's normalised weights wx, wy (L.ss_taps: 2 R + 1 along x, then 2 R + 1 along y) and
// the border replicated.  Every tap is evaluated, zero weights too, so a sample that is not finite
// reaches its whole footprint.  The frames of the batch are then added in ascending frame order,
// in k_accum's three forms: into the fp32 sum, into the fp64 sum (with its fp32 rounding stored), or
// each frame's 0.0f + g to its own image (frame_stride).
// One workgroup of four waves per 16x16 output pixels.  Per frame the tile and its halo, (16 + 2 R)^2
// radiance records, are staged in LDS; the two LDS buffers alternate, and the next frame's records
// are already on their way to registers while this frame's taps are summed, so a frame costs one
// barrier.  The cell, and with it the tap rows' address, is the same for the whole workgroup.  It is
// a gather: no atomics, and the order of the additions is the one above.  tests/pixel_filter_ref.py
// restates it in numpy.
#include "pt_internal.h"

namespace pt {

namespace {

constexpr int kTileF = 16;  // output pixels along a workgroup's side
constexpr int kBlockF = kTileF * kTileF;

template <int R>
__global__ __launch_bounds__(kBlockF) void k_accum_filtered(const float4* __restrict__ rad, DevLaunch L, int nf) {
    constexpr int K = 2 * R + 1, T = kTileF + 2 * R, N = T * T;
    static_assert(N > kBlockF && N <= 2 * kBlockF, "every thread stages one record, some a second one");
    __shared__ float4 tile[2][N];
    const int W = L.width, H = L.height;
    const size_t P = (size_t)W * (size_t)H;
    const int tid = (int)threadIdx.x, lx = tid & (kTileF - 1), ly = tid / kTileF;
    const int x0 = (int)blockIdx.x * kTileF, y0 = (int)blockIdx.y * kTileF;
    const int X = x0 + lx, Y = y0 + ly;
    const bool in = X < W && Y < H;  // the others only stage records
    // the records this thread stages: slots tid and (where the tile has it) tid + kBlockF of the tile,
    // each from its clamped image pixel
    const auto source = [&](int slot) {
        const int ty = slot / T, tx = slot - ty * T;
        return min(max(y0 - R + ty, 0), H - 1) * W + min(max(x0 - R + tx, 0), W - 1);
    };
    const bool two = tid + kBlockF < N;
    const int src0 = source(tid), src1 = two ? source(tid + kBlockF) : src0;
    float4 next0 = rad[src0], next1 = rad[src1];
    const size_t idx = in ? ((size_t)Y * (size_t)W + (size_t)X) * 3 : 0;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (in && !L.frame_stride) {
        if (L.accum64) {
            dx = L.accum64[idx], dy = L.accum64[idx + 1], dz = L.accum64[idx + 2];
        } else {
            sx = L.accum[idx], sy = L.accum[idx + 1], sz = L.accum[idx + 2];
        }
    }
    const uint32_t cell_mask = (uint32_t)(L.ss * L.ss - 1);
    for (int f = 0; f < nf; ++f) {
        float4* buf = tile[f & 1];
        buf[tid] = next0;
        if (two) buf[tid + kBlockF] = next1;
        if (f + 1 < nf) {
            const float4* nr = rad + (size_t)(f + 1) * P;
            next0 = nr[src0];
            next1 = nr[src1];
        }
        // the only barrier of the frame: the buffer written next was last read before this one
        __syncthreads();
        const float* taps = L.ss_taps + (size_t)((L.frame_base + (uint32_t)f) & cell_mask) * (2 * K);  // wave-uniform
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const float w = taps[K + j] * taps[i];  // wy[j] * wx[i]
                const float4 l = buf[(ly + j) * T + (lx + i)];
                gx = gx + w * l.x;
                gy = gy + w * l.y;
                gz = gz + w * l.z;
            }
        }
        if (L.frame_stride) {  // render-ahead: each frame its own image, a one-frame sum into zeros
            if (in) {
                float* o = L.accum + (size_t)f * L.frame_stride + idx;
                o[0] = 0.0f + gx;
                o[1] = 0.0f + gy;
                o[2] = 0.0f + gz;
            }
        } else if (L.accum64) {
            dx += (double)gx;
            dy += (double)gy;
            dz += (double)gz;
        } else {  // frames in order: the sequential accumulation
            sx += gx;
            sy += gy;
            sz += gz;
        }
    }
    if (!in || L.frame_stride) return;
    if (L.accum64) {
        L.accum64[idx] = dx;
        L.accum64[idx + 1] = dy;
        L.accum64[idx + 2] = dz;
        sx = (float)dx, sy = (float)dy, sz = (float)dz;
    }
    L.accum[idx] = sx;
    L.accum[idx + 1] = sy;
    L.accum[idx + 2] = sz;
}

}  // namespace

hipError_t accum_filtered(const float4* radiance, const DevLaunch& L, int nf, hipStream_t stream) {
    if (L.ss_R < 1 || L.ss_R > kFilterMaxR || L.ss < 1 || L.pixel_map || L.row0 != 0 || L.height != L.image_height)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((L.width + kTileF - 1) / kTileF), (unsigned)((L.height + kTileF - 1) / kTileF));
    if (L.ss_R == 1)
        hipLaunchKernelGGL(k_accum_filtered<1>, grid, dim3(kBlockF), 0, stream, radiance, L, nf);
    else
        hipLaunchKernelGGL(k_accum_filtered<2>, grid, dim3(kBlockF), 0, stream, radiance, L, nf);
    return hipGetLastError();
}

}  // namespace pt
