// pt_atrous.h — what the image-space kernels of pt_aov.hip (G-buffer, a-trous filter) and
// pt_temporal.hip (temporal reprojection, variance-guided a-trous) share: the pixel tiling, the
// small exact functions that DESIGN.md §10 and §11 name, and the one a-trous iteration that both
// filters run.  Device code only.
//
// k_filter / k_filter_rows: one iteration, one thread per pixel, ping-pong float4 colour buffers, no
// atomics.  Every load is a 16-byte record: the colour and the two guide records (normal | valid,
// position | depth).  The steps 1, 2 and 4 stage a 16x16 tile and its halo in LDS, the steps 8 and
// 16 a tile of rows one step apart, larger steps load every tap from global memory (measured:
// DESIGN.md §10).  What a tap weighs and what is stored is the term F's, a type of the including
// file bound at compile time (ColourTerm in pt_aov.hip, LuminanceTerm in pt_temporal.hip): the
// kernel's argument F::Params with its AtrousParams F::base(P); F(cp), the result of a pixel that is
// not filtered; begin, tap and finish around the taps of one that is; store<LAST>.
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

// The records of pixel (gx, gy) from three streams, for an LDS tile; zeros outside the image (a
// guide's w = 0: no tap there).
__device__ __forceinline__ void stage(const float4* a, const float4* b, const float4* c, int w, int h, int gx, int gy,
                                      float4& sa, float4& sb, float4& sc) {
    float4 ra = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb = ra, rc = ra;
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
        const size_t g = (size_t)gy * (size_t)w + (size_t)gx;
        ra = a[g];
        rb = b[g];
        rc = c[g];
    }
    sa = ra;
    sb = rb;
    sc = rc;
}

// A term's store: c_{i+1}[p] = out | lane, or after the last iteration the remodulated out in the W*H*3 output.
template <bool LAST>
__device__ __forceinline__ void filter_store(const AtrousParams& A, size_t p, bool valid, f3 out, float lane) {
    if (LAST) {
        if (valid && A.demodulate) out = out * albedo_floor(A.ga[p], A.floor);
        store3(A.out, p, out);
    } else {
        A.cout[p] = make_float4(out.x, out.y, out.z, lane);
    }
}

// LAST: the remodulated result goes to the W*H*3 output instead of the next colour buffer.
// LSTEP > 0: the step is LSTEP, and the workgroup's tile with its halo of 2 * LSTEP pixels, (16 +
// 4 LSTEP)^2 records of 48 B, is staged in LDS first; LSTEP = 0: any step, every tap a global load.
template <class F, bool LAST, int LSTEP>
__global__ __launch_bounds__(kBlock) void k_filter(typename F::Params P) {
    const AtrousParams& A = F::base(P);
    constexpr bool LDS = LSTEP > 0;
    constexpr int side = kTile + 4 * LSTEP, kRecords = LDS ? side * side : 1;
    __shared__ float4 sc[kRecords], sn[kRecords], sp[kRecords];
    int x, y;
    tile_pixel(x, y);
    const int s = LDS ? LSTEP : A.step;
    const int ox = blockIdx.x * kTile - 2 * s, oy = blockIdx.y * kTile - 2 * s;
    if (LDS) {
        for (int i = threadIdx.x; i < side * side; i += kBlock)
            stage(A.cin, A.gn, A.gp, A.w, A.h, ox + i % side, oy + i / side, sc[i], sn[i], sp[i]);
        __syncthreads();
    }
    if (x >= A.w || y >= A.h) return;
    const size_t p = (size_t)y * (size_t)A.w + (size_t)x;
    const int lp = LDS ? (y - oy) * side + (x - ox) : 0;
    const float4 cp = LDS ? sc[lp] : A.cin[p], np = LDS ? sn[lp] : A.gn[p], pp = LDS ? sp[lp] : A.gp[p];
    const bool valid = np.w != 0.0f;
    F f(cp);
    if (valid) {
        f.begin(P, p, cp);
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + dx * s, qy = y + dy * s;
                const float k = b3(dy + 2) * b3(dx + 2);
                float4 cq, nq, pq;
                if (LDS) {
                    const int lq = (qy - oy) * side + (qx - ox);
                    nq = sn[lq];
                    if (nq.w == 0.0f) continue;
                    cq = sc[lq];
                    pq = sp[lq];
                } else {
                    if (qx < 0 || qx >= A.w || qy < 0 || qy >= A.h) continue;
                    const size_t q = (size_t)qy * (size_t)A.w + (size_t)qx;
                    nq = A.gn[q];
                    if (nq.w == 0.0f) continue;
                    cq = A.cin[q];
                    pq = A.gp[q];
                }
                f.tap(k, dx == 0 && dy == 0, cq, nq, pq, cp, np, pp, A);
            }
        }
        f.finish();
    }
    f.template store<LAST>(P, p, valid);
}

// The same iteration for the steps 8 and 16, where a square tile's halo outgrows the LDS: a
// workgroup takes 32 columns of 8 rows that lie `STEP` apart (thread = column + 32 * row), so the
// vertical taps are the neighbouring rows of its tile: (32 + 4 STEP) x 12 records.  blockIdx.y
// counts STEP row phases within each band of 8 * STEP image rows.
template <class F, bool LAST, int STEP>
__global__ __launch_bounds__(kBlock) void k_filter_rows(typename F::Params P) {
    const AtrousParams& A = F::base(P);
    constexpr int kCols = 32, kRows = 8, side = kCols + 4 * STEP, kRecords = side * (kRows + 4);
    __shared__ float4 sc[kRecords], sn[kRecords], sp[kRecords];
    const int ox = blockIdx.x * kCols - 2 * STEP;
    const int y0 = ((int)blockIdx.y / STEP) * (kRows * STEP) + (int)blockIdx.y % STEP;  // tile row 0
    for (int i = threadIdx.x; i < kRecords; i += kBlock)
        stage(A.cin, A.gn, A.gp, A.w, A.h, ox + i % side, y0 + (i / side - 2) * STEP, sc[i], sn[i], sp[i]);
    __syncthreads();
    const int col = threadIdx.x % kCols, row = threadIdx.x / kCols;
    const int x = blockIdx.x * kCols + col, y = y0 + row * STEP;
    if (x >= A.w || y >= A.h) return;
    const size_t p = (size_t)y * (size_t)A.w + (size_t)x;
    const int lp = (row + 2) * side + (x - ox);
    const float4 cp = sc[lp], np = sn[lp], pp = sp[lp];
    const bool valid = np.w != 0.0f;
    F f(cp);
    if (valid) {
        f.begin(P, p, cp);
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int lq = lp + dy * side + dx * STEP;
                const float4 nq = sn[lq];
                if (nq.w == 0.0f) continue;
                f.tap(b3(dy + 2) * b3(dx + 2), dx == 0 && dy == 0, sc[lq], nq, sp[lq], cp, np, pp, A);
            }
        }
        f.finish();
    }
    f.template store<LAST>(P, p, valid);
}

// One iteration of term F: the kernel of A.step, staged in LDS up to min(lds_max_step, kAtrousLdsMaxStep).
template <class F, bool LAST>
hipError_t filter_launch(const typename F::Params& P, int lds_max_step, hipStream_t stream) {
    const AtrousParams& A = F::base(P);
    const dim3 grid = tile_grid(A.w, A.h);
    const int lstep = A.step <= std::min(lds_max_step, kAtrousLdsMaxStep) ? A.step : 0;
    // k_filter_rows: 32 columns per workgroup; per band of 8 * step rows, one workgroup per row phase
    const dim3 rows((unsigned)((A.w + 31) / 32), (unsigned)((A.h + 8 * A.step - 1) / (8 * A.step) * A.step));
    switch (lstep) {
        case 1: hipLaunchKernelGGL((k_filter<F, LAST, 1>), grid, dim3(kBlock), 0, stream, P); break;
        case 2: hipLaunchKernelGGL((k_filter<F, LAST, 2>), grid, dim3(kBlock), 0, stream, P); break;
        case 4: hipLaunchKernelGGL((k_filter<F, LAST, 4>), grid, dim3(kBlock), 0, stream, P); break;
        case 8: hipLaunchKernelGGL((k_filter_rows<F, LAST, 8>), rows, dim3(kBlock), 0, stream, P); break;
        case 16: hipLaunchKernelGGL((k_filter_rows<F, LAST, 16>), rows, dim3(kBlock), 0, stream, P); break;
        default: hipLaunchKernelGGL((k_filter<F, LAST, 0>), grid, dim3(kBlock), 0, stream, P); break;
    }
    return hipGetLastError();
}

template <class F>
hipError_t filter_iteration(const typename F::Params& P, bool last, int lds_max_step, hipStream_t stream) {
    return last ? filter_launch<F, true>(P, lds_max_step, stream) : filter_launch<F, false>(P, lds_max_step, stream);
}

}  // namespace
}  // namespace pt
