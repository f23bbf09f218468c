// pt_render.hip — render kernels for gfx950 (replaces optixLaunch of __raygen__renderFrame,
// Renderer/OptiX/OptixRenderer.cpp:617-647, and the per-spp GL accumulation of
// Renderer/OptixView.cpp:212-255).
//
// k_render_mega<MODE>: one thread per pixel; a 256-thread workgroup covers a 16x16 pixel
// tile, each wave64 an 8x8 quadrant (primary-ray coherence inside the wave).  The thread
// loads its fp32 sum, adds the radiance of frame ids frame_base .. frame_base+n_frames-1
// in order (identical rounding to sequential per-frame accumulation), and stores it once:
// no per-spp HBM round trip of the 24.9 MB colour buffer.  The BVH4 traversal stack lives
// in LDS (32 entries x 256 threads = 32 KB per workgroup).
#include "pt_internal.h"
#include "pt_shade.h"

namespace pt {

namespace {

constexpr int kBlock = 256;
// LDS traversal stack entries per lane (PT_MK_STACK, pt_device.h; the megakernel is
// VGPR-limited, not LDS-limited).
constexpr int kStack = PT_MK_STACK;
// Minimum waves per SIMD the register allocator must allow (caps VGPRs at 512/N).
#ifndef PT_MK_WAVES
#define PT_MK_WAVES 1
#endif

// Path state of one camera sample (RadianceRayData, RayData.h:5-21).
struct PathState {
    f3 o, d, beta, radiance;
    uint32_t seed;
    int bounce;
    bool end;
};

__device__ __forceinline__ void path_start(PathState& p, f3 o, f3 d, uint32_t seed) {  // SamplePath :626-635
    p.o = o;
    p.d = d;
    p.beta = mk(1.0f, 1.0f, 1.0f);
    p.radiance = mk(0.0f, 0.0f, 0.0f);
    p.seed = seed;
    p.bounce = 0;
    p.end = false;
}

// loop test of SamplePath (devicePrograms.cu:646)
__device__ __forceinline__ bool path_alive(const DevLaunch& L, const PathState& p) {
    return !p.end && p.bounce < L.max_bounces && length(p.beta) > 0.00001f;
}

// One iteration of SamplePath's loop: TraceRadiance + __closesthit__radiance
// (devicePrograms.cu:343-514) or __miss__radiance (:576-583), in the steps of pt_shade.h.
template <int MODE, bool STATS, int DEPTH, bool TEX>
__device__ __forceinline__ void path_segment(const DevScene& S, const DevLaunch& L, PathState& p, int* stk,
                                             int stride, TravStats& ts, bool debug_path) {
    Hit h;
    bool hit = traverse<kRayClosest, STATS, DEPTH, TEX>(S, p.o, p.d, 0.0f, 100.0f, h, stk, stride, ts);
    if (!hit) {
        p.beta = mk(0, 0, 0);
        p.bounce = 100;
        return;
    }
    p.bounce++;
    if (p.bounce > L.max_bounces) {
        p.end = true;
        return;
    }
    SurfaceHit sf;
    reconstruct<TEX>(S, h, p.d, sf);
    if (debug_path) debug_record(L, p.bounce, __float_as_int(S.isect[3 * h.tri].w), sf, p.beta, p.radiance);
    const bool conductor = rnd(p.seed) < sf.metallic;  // :400
    int li;
    const float P = pick_light(L, p.seed, li);
    if (P > 0.0f) {  // NEE (:446-472)
        const DevLight lt = L.lights[li];
        f3 so, sdir;
        float stmax;
        shadow_ray(sf.pos, sf.ng, light_vec(lt, sf.pos), so, sdir, stmax);
        Hit sh;
        bool occluded = traverse<kRayAny, STATS, DEPTH, TEX>(S, so, sdir, 0.0f, stmax, sh, stk, stride, ts);
        f3 lds = light_local(sf, lt);
        if (!occluded) {
            f3 f = bsdf_f<MODE>(p.seed, sf.albedo, sf.roughness, conductor, sf.wo, lds);
            f3 spectrum = nee_spectrum(f, lds);
            if (!is_zero(spectrum))
                p.radiance = p.radiance + nee_contrib(p.beta, spectrum, lt, light_dist2(lt, sf.pos), P);
        }
    }
    BSample bs;
    // the last segment's sampled direction is never traced (SamplePath's loop test, :646):
    // skipping the sample leaves every traced value unchanged
    if (p.bounce >= L.max_bounces || !bsdf_sample<MODE>(p.seed, sf.albedo, sf.roughness, conductor, sf.wo, bs)) {
        p.end = true;
        return;
    }
    continue_path(sf, bs, p.beta, p.o, p.d, p.bounce, L.max_bounces);  // path_alive holds its loop test
}

// The wave's path segments (counted with or without STATS) and its traversal statistics.  A function
// with the sum first: written out in the kernel, or summed after the flush, the same operations cost
// the Conductor and Dielectric kernels 4 VGPRs and a wave per SIMD (profiles/shade_steps_isa.txt).
template <bool STATS>
__device__ __forceinline__ void flush_segments(const DevLaunch& L, uint32_t segs, const TravStats& ts, int lane) {
    const unsigned long long a = wave_sum_u64(segs);
    flush_trav_stats<STATS>(L.counters, ts);
    if (lane == 0 && L.counters) atomicAdd(&L.counters[kCtrSegments], a);
}

template <int MODE, bool STATS, bool TEX>
__global__ __launch_bounds__(kBlock, PT_MK_WAVES) void k_render_mega(DevScene S, DevLaunch L) {
    __shared__ int stack[kStack * kBlock];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    int* stk = stack + threadIdx.x;
    uint32_t segs = 0;
    TravStats ts;
    if (x < L.width && y < L.height && L.n_frames > 0) {
        f3 co, cd;
        camera_ray(L, x, y, co, cd);
        const size_t idx = ((size_t)y * (size_t)L.width + (size_t)x) * 3;
        float sx = L.accum[idx], sy = L.accum[idx + 1], sz = L.accum[idx + 2];
        const uint32_t pix = (uint32_t)(L.width * y + x);
        // Path regeneration: a lane whose path ends starts its next frame at once instead of
        // idling until the wave's longest path of the frame finishes.  Each lane still adds
        // its frames in order, so the sum is bit-identical to the sequential accumulation.
        uint32_t f = 0;
        PathState p;
        path_start(p, co, cd, tea16(pix, L.frame_base));  // devicePrograms.cu:631
        const bool debug_pixel = L.debug_pixel == (int)pix;
        while (true) {
            if (path_alive(L, p)) {
                path_segment<MODE, STATS, kStack, TEX>(S, L, p, stk, kBlock, ts,
                                                       debug_pixel && L.frame_base + f == L.debug_frame);
                segs++;
                continue;
            }
            sx += p.radiance.x;
            sy += p.radiance.y;
            sz += p.radiance.z;
            if (++f == L.n_frames) break;
            path_start(p, co, cd, tea16(pix, L.frame_base + f));
        }
        L.accum[idx] = sx;
        L.accum[idx + 1] = sy;
        L.accum[idx + 2] = sz;
    }
    flush_segments<STATS>(L, segs, ts, lane);
}

template <bool TEX>
__global__ __launch_bounds__(kBlock) void k_trace(DevScene S, const float* rays, int n, int* prim, float* th,
                                                  float* uh, float* vh, int* back, int any_hit) {
    __shared__ int stack[kStack * kBlock];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = rays + 8 * (size_t)i;
    f3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    Hit h;
    TravStats ts;
    int* stk = stack + threadIdx.x;
    bool hit = any_hit ? traverse<true, false, kStack, TEX>(S, o, d, r[6], r[7], h, stk, kBlock, ts)
                       : traverse<false, false, kStack, TEX>(S, o, d, r[6], r[7], h, stk, kBlock, ts);
    // any-hit: the occluder's original index (an any-hit traversal records only its leaf slot)
    prim[i] = hit ? (any_hit ? __float_as_int(S.isect[3 * h.tri].w) : h.orig) : -1;
    th[i] = hit && !any_hit ? h.t : 0.0f;
    uh[i] = hit && !any_hit ? h.u : 0.0f;
    vh[i] = hit && !any_hit ? h.v : 0.0f;
    back[i] = hit && !any_hit ? (h.back ? 1 : 0) : 0;
}

template <int MODE>
hipError_t launch_mega(const DevScene& S, const DevLaunch& L, bool stats, hipStream_t stream) {
    dim3 grid((unsigned)((L.width + 15) / 16), (unsigned)((L.height + 15) / 16));
    with_flag(S.texinfo != nullptr, [&](auto tx) {
        with_flag(stats, [&](auto st) {
            hipLaunchKernelGGL((k_render_mega<MODE, st(), tx()>), grid, dim3(kBlock), 0, stream, S, L);
        });
    });
    return hipGetLastError();
}

}  // namespace

hipError_t launch_render(int kernel, int mode, bool stats, const DevScene& S, const DevLaunch& L,
                         hipStream_t stream) {
    (void)kernel;
    switch (mode) {
        case kModeLambert: return launch_mega<kModeLambert>(S, L, stats, stream);
        case kModeConductor: return launch_mega<kModeConductor>(S, L, stats, stream);
        case kModeDielectric: return launch_mega<kModeDielectric>(S, L, stats, stream);
        case kModeLayered: return launch_mega<kModeLayered>(S, L, stats, stream);
        default: return launch_mega<kModeDefault>(S, L, stats, stream);
    }
}

hipError_t launch_trace(const DevScene& S, const float* d_rays, int n, int* d_prim, float* d_thit, float* d_u,
                        float* d_v, int* d_back, int any_hit, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    with_flag(S.texinfo != nullptr, [&](auto tx) {
        hipLaunchKernelGGL(k_trace<tx()>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, S, d_rays,
                           n, d_prim, d_thit, d_u, d_v, d_back, any_hit);
    });
    return hipGetLastError();
}

}  // namespace pt
