// pt_adaptive.hip — the kernels of pt_render_adaptive (pt_capi_adaptive.cpp): rounds
// of frames over the pixels of the 8x8 tiles that have not converged yet.  A round's batches end in
// the mapped accumulate, k_accum_adaptive (pt_accum.hip), which keeps the sum, the moments S1 and S2
// and the sample counts; here are the estimate, the compaction and the resolve.
//
// k_adapt_error: one wave64 per tile, one lane per pixel (lane = 8 * row + column in the tile).  The
// pixel's relative standard error e in fp64, then the tile's sum of e by a six-step butterfly: step k
// adds the lanes whose index differs in bit k, so the tree is the same whatever the hardware does and
// every lane ends with the same bits (fp64 + is commutative).  Lanes outside the image add 0.
// k_adapt_fill: after an exclusive scan (hipCUB) of the active tiles' pixel counts, each active
// tile's wave writes its pixels' image indices in raster order at the tile's offset, and the last
// tile's wave the total.
// k_adapt_resolve: mean = sum / (float)n.
// The arithmetic is the specification of §12 (-ffp-contract=off, IEEE fp64 division and square root);
// tests/adaptive_ref.py restates it in numpy.
#include <hipcub/hipcub.hpp>

#include "pt_internal.h"

namespace pt {

namespace {

constexpr int kBlockAd = 256;
constexpr int kTile = 8;  // pixels along a tile's side: 64 pixels, one wave

// a < b ? b : a -- a NaN in `a` stays (fmax would drop it), so a pixel whose moments are not finite
// keeps its tile rendering
__device__ __forceinline__ double max_keep_nan(double a, double b) { return a < b ? b : a; }

// This wave's tile and this lane's pixel of it: false when the wave is past the last tile.
__device__ __forceinline__ bool wave_tile(const AdaptiveBuffers& A, int& tile, int& x, int& y) {
    const int lane = (int)(threadIdx.x & 63);
    tile = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (tile >= A.tiles_x * A.tiles_y) return false;
    const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
    x = tx * kTile + (lane & 7);
    y = ty * kTile + (lane >> 3);
    return true;
}

__global__ __launch_bounds__(kBlockAd) void k_adapt_error(AdaptiveBuffers A, float threshold, uint32_t min_samples,
                                                          uint32_t max_samples, float luminance_floor) {
    int tile, x, y;
    if (!wave_tile(A, tile, x, y)) return;               // wave-uniform
    if (A.tile_state[tile] != kTileActive) return;       // not rendered in this round: its figures stay
    const bool in = x < A.w && y < A.h;
    const int ip = y * A.w + x;
    double e = 0.0;
    uint32_t n = 0;
    if (in) {
        n = A.n[ip];
        const double dn = (double)n;
        const double s1 = A.moments[2 * (size_t)ip], s2 = A.moments[2 * (size_t)ip + 1];
        const double m = s1 / dn;
        const double v = max_keep_nan(s2 / dn - m * m, 0.0) / dn;
        e = sqrt(v) / max_keep_nan(m, (double)luminance_floor);
        A.err[ip] = (float)e;
    }
    double sum = e;
    for (int k = 0; k < 6; ++k) sum += __shfl_xor(sum, 1 << k, 64);
    const int cnt = min(kTile, A.w - (x - (int)(threadIdx.x & 7))) * min(kTile, A.h - (y - (int)((threadIdx.x & 63) >> 3)));
    const double te = sum / (double)cnt;
    if ((threadIdx.x & 63) == 0) {  // lane 0 is the tile's pixel (0, 0), always in the image
        A.tile_err[tile] = (float)te;
        A.tile_rounds[tile] += 1;
        int state = kTileActive;
        if (te <= (double)threshold && n >= min_samples) state = kTileStopped;
        else if (n >= max_samples) state = kTileFull;
        A.tile_state[tile] = state;
    }
}

// cnt[t] = the pixels tile t adds to the next round's list: its in-image pixels while it is active.
__global__ __launch_bounds__(kBlockAd) void k_adapt_count(AdaptiveBuffers A) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= A.tiles_x * A.tiles_y) return;
    const int ty = t / A.tiles_x, tx = t - ty * A.tiles_x;
    const int c = min(kTile, A.w - tx * kTile) * min(kTile, A.h - ty * kTile);
    A.tile_cnt[t] = A.tile_state[t] == kTileActive ? c : 0;
}

__global__ __launch_bounds__(kBlockAd) void k_adapt_fill(AdaptiveBuffers A) {
    int tile, x, y;
    if (!wave_tile(A, tile, x, y)) return;  // wave-uniform
    const int lane = (int)(threadIdx.x & 63);
    const int off = A.tile_off[tile], c = A.tile_cnt[tile];
    if (tile == A.tiles_x * A.tiles_y - 1 && lane == 0) *A.count = off + c;
    if (c == 0 || x >= A.w || y >= A.h) return;
    const int tw = min(kTile, A.w - (x - (lane & 7)));  // the tile's width in the image
    A.pixel_map[off + (lane >> 3) * tw + (lane & 7)] = y * A.w + x;
}

__global__ __launch_bounds__(kBlockAd) void k_adapt_resolve(const float* __restrict__ sum, const uint32_t* __restrict__ n,
                                                            float* __restrict__ mean, int pixels) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= pixels) return;
    const float fn = (float)n[p];
    mean[3 * (size_t)p] = sum[3 * (size_t)p] / fn;
    mean[3 * (size_t)p + 1] = sum[3 * (size_t)p + 1] / fn;
    mean[3 * (size_t)p + 2] = sum[3 * (size_t)p + 2] / fn;
}

inline dim3 grid_for(int items) { return dim3((unsigned)std::max(1, (items + kBlockAd - 1) / kBlockAd)); }

}  // namespace

hipError_t adaptive_scan_bytes(int tiles, size_t* bytes) {
    *bytes = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const int*)nullptr, (int*)nullptr, tiles);
}

hipError_t adaptive_estimate(const AdaptiveBuffers& A, float threshold, uint32_t min_samples, uint32_t max_samples,
                             float luminance_floor, hipStream_t stream) {
    const int tiles = A.tiles_x * A.tiles_y;
    hipLaunchKernelGGL(k_adapt_error, grid_for(tiles * 64), dim3(kBlockAd), 0, stream, A, threshold, min_samples,
                       max_samples, luminance_floor);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return adaptive_compact(A, stream);
}

hipError_t adaptive_compact(const AdaptiveBuffers& A, hipStream_t stream) {
    const int tiles = A.tiles_x * A.tiles_y;
    hipLaunchKernelGGL(k_adapt_count, grid_for(tiles), dim3(kBlockAd), 0, stream, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = A.scan_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(A.scan_tmp, bytes, A.tile_cnt, A.tile_off, tiles, stream)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_adapt_fill, grid_for(tiles * 64), dim3(kBlockAd), 0, stream, A);
    return hipGetLastError();
}

hipError_t adaptive_resolve(const float* sum, const uint32_t* n, float* mean, int pixels, hipStream_t stream) {
    hipLaunchKernelGGL(k_adapt_resolve, grid_for(pixels), dim3(kBlockAd), 0, stream, sum, n, mean, pixels);
    return hipGetLastError();
}

}  // namespace pt
