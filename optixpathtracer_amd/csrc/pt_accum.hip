// pt_accum.hip — the last stage of a wavefront batch: the batch's frames added to the destination
// (accum_batch), and the fp64 sum's rounding to fp32 (accum_f64_to_f32).
//
// PixelSum is the one definition of the destination's three forms, and with it of the fp32 order
// that makes the image equal the sequential reference accumulation bit for bit:
//   the fp32 sum      s = accum[pixel];  s += g for the frames in ascending order;  accum[pixel] = s
//   the fp64 sum      the same in fp64 on accum64 with d += (double)g, and accum[pixel] = (float)d
//   per-frame images  frame f's 0.0f + g alone to accum + f * frame_stride (the render-ahead ring): a
//                     one-frame sum into zeros
// Three kernels feed it, one per way a frame's g of a pixel comes about:
// k_accum: g = L[f * P + pixel], the path's radiance.
// k_accum_filtered<R>: a launch whose pixel filter is wider than the box.  The sample of frame F sits
// in cell c = F mod ss^2 of its pixel, and the frame's filtered image is, per output pixel (X, Y) in
// fp32 without contraction,
//     g = 0;  for j = -R..R: for i = -R..R:  g = g + (wy[j] * wx[i]) * L_F(clamp(X + i), clamp(Y + j))
// with the cell's normalised weights wx, wy (L.ss_taps: 2 R + 1 along x, then 2 R + 1 along y) and
// the border replicated.  Every tap is evaluated, zero weights too, so a sample that is not finite
// reaches its whole footprint.
// One workgroup of four waves per 16x16 output pixels.  Per frame the tile and its halo, (16 + 2 R)^2
// radiance records, are staged in LDS; the two LDS buffers alternate, and the next frame's records
// are already on their way to registers while this frame's taps are summed, so a frame costs one
// barrier.  The cell, and with it the tap rows' address, is the same for the whole workgroup.  It is
// a gather: no atomics, and the order of the additions is the one above.  tests/pixel_filter_ref.py
// restates it in numpy.
// k_accum_adaptive: a mapped launch (DevLaunch::pixel_map, pt_render_adaptive).  One thread per
// mapped pixel: g = L[f * n_pixels + p] into the fp32 sum of image pixel pixel_map[p], and each
// frame's fp32 luminance, widened to fp64, into the pixel's moments S1 and S2 (tests/adaptive_ref.py).
#include "pt_internal.h"

namespace pt {

namespace {

constexpr int kBlockAcc = 256;
constexpr int kTileF = 16;  // k_accum_filtered: output pixels along a workgroup's side
constexpr int kBlockF = kTileF * kTileF;

// The running sum of the pixel whose RGB starts at float idx of the destination, in the launch's
// form (wave-uniform).  live = false: a thread without a pixel, which loads and stores nothing.
struct PixelSum {
    const DevLaunch& L;
    const size_t idx;
    const bool live;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    double dx = 0.0, dy = 0.0, dz = 0.0;
    __device__ __forceinline__ PixelSum(const DevLaunch& launch, size_t i, bool lv = true) : L(launch), idx(i), live(lv) {
        if (!live || L.frame_stride) return;
        if (L.accum64) {  // pt_set_accum_fp64: the frames' fp32 radiance summed in fp64
            dx = L.accum64[idx], dy = L.accum64[idx + 1], dz = L.accum64[idx + 2];
        } else {
            sx = L.accum[idx], sy = L.accum[idx + 1], sz = L.accum[idx + 2];
        }
    }
    // frame f of the batch, in ascending order: the sequential accumulation
    __device__ __forceinline__ void add(int f, float gx, float gy, float gz) {
        if (L.frame_stride) {  // render-ahead: each frame its own 1-spp image
            if (live) {
                float* o = L.accum + (size_t)f * L.frame_stride + idx;
                o[0] = 0.0f + gx;
                o[1] = 0.0f + gy;
                o[2] = 0.0f + gz;
            }
        } else if (L.accum64) {
            dx += (double)gx;
            dy += (double)gy;
            dz += (double)gz;
        } else {
            sx += gx;
            sy += gy;
            sz += gz;
        }
    }
    __device__ __forceinline__ void store() {
        if (!live || L.frame_stride) return;
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
};

__global__ __launch_bounds__(kBlockAcc) void k_accum(const float4* __restrict__ rad, DevLaunch L, int nf) {
    const int P = L.width * L.height;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        PixelSum sum(L, (size_t)p * 3);
        for (int f = 0; f < nf; ++f) {
            const float4 l = rad[(size_t)f * P + p];
            sum.add(f, l.x, l.y, l.z);
        }
        sum.store();
    }
}

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
    PixelSum sum(L, in ? ((size_t)Y * (size_t)W + (size_t)X) * 3 : 0, in);
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
        sum.add(f, gx, gy, gz);
    }
    sum.store();
}

__global__ __launch_bounds__(kBlockAcc) void k_accum_adaptive(const float4* __restrict__ rad, DevLaunch L, int nf) {
    const int P = launch_pixels(L);
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= P) return;
    const int ip = L.pixel_map[p];
    PixelSum sum(L, (size_t)ip * 3);
    double s1 = L.adapt_moments[2 * (size_t)ip], s2 = L.adapt_moments[2 * (size_t)ip + 1];
    for (int f = 0; f < nf; ++f) {
        const float4 l = rad[(size_t)f * P + p];
        sum.add(f, l.x, l.y, l.z);
        const double y = (double)luminance(l);
        s1 += y;
        s2 += y * y;
    }
    sum.store();
    L.adapt_moments[2 * (size_t)ip] = s1;
    L.adapt_moments[2 * (size_t)ip + 1] = s2;
    L.adapt_n[ip] += (uint32_t)nf;
}

__global__ __launch_bounds__(kBlockAcc) void k_f64_to_f32(const double* __restrict__ a, float* __restrict__ b, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        b[i] = (float)a[i];
}

// Grid covering `items` slots, one per thread.
inline dim3 item_grid(int items) { return dim3((unsigned)std::max(1, (items + kBlockAcc - 1) / kBlockAcc)); }

}  // namespace

hipError_t accum_batch(const float4* radiance, const DevLaunch& L, int nf, hipStream_t stream) {
    if (L.pixel_map) {  // a mapped launch adds into the fp32 sum alone
        if (L.accum64 || L.frame_stride || L.ss_taps) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_accum_adaptive, item_grid(L.n_pixels), dim3(kBlockAcc), 0, stream, radiance, L, nf);
    } else if (L.ss_taps) {  // a pixel filter wider than the box gathers across a whole image
        if (L.ss_R < 1 || L.ss_R > kFilterMaxR || L.ss < 1 || L.row0 != 0 || L.height != L.image_height)
            return hipErrorInvalidValue;
        const dim3 grid((unsigned)((L.width + kTileF - 1) / kTileF), (unsigned)((L.height + kTileF - 1) / kTileF));
        if (L.ss_R == 1)
            hipLaunchKernelGGL(k_accum_filtered<1>, grid, dim3(kBlockF), 0, stream, radiance, L, nf);
        else
            hipLaunchKernelGGL(k_accum_filtered<2>, grid, dim3(kBlockF), 0, stream, radiance, L, nf);
    } else {
        hipLaunchKernelGGL(k_accum, item_grid(L.width * L.height), dim3(kBlockAcc), 0, stream, radiance, L, nf);
    }
    return hipGetLastError();
}

hipError_t accum_f64_to_f32(const double* sum64, float* sum32, size_t n, hipStream_t stream) {
    const unsigned blocks = (unsigned)std::min<size_t>((n + kBlockAcc - 1) / kBlockAcc, 8192);
    hipLaunchKernelGGL(k_f64_to_f32, dim3(std::max(1u, blocks)), dim3(kBlockAcc), 0, stream, sum64, sum32, n);
    return hipGetLastError();
}

}  // namespace pt
