// pt_wavefront.hip — wavefront path tracer for gfx950 (PT_KERNEL_WAVEFRONT).
//
// The reference runs one OptiX thread per pixel that loops over bounces
// (SamplePath, devicePrograms.cu:625-664).  Here each bounce of a frame is a sequence of
// persistent, grid-stride kernels over SoA queues in HBM, so the traversal kernels carry
// only a ray (low VGPR count -> high occupancy) and the BSDF code runs in its own kernel:
//
//   k_camera            : path q = f * P + pixel for the nf frames of the batch; camera ray ->
//                         queue 0, state init (with sub-pixel cells, pt_set_pixel_filter: the ray and
//                         the seed of the frame's cell of the pixel, DevLaunch::ss_cells)
//   per bounce b:
//     k_extend          : closest hit of queue b (BVH4 traversal, LDS stack) -> hit records
//                         (fused modes: bounce 0 only; later bounces ride in k_trace_pair)
//     fused modes (Lambert / Conductor / Dielectric: BRDF eval draws no random numbers):
//       k_shade_fused   : surface, metallic coin, light pick, f*|cos|, BSDF sample; NEE
//                         contribution + shadow ray -> shadow queue (only if f != 0);
//                         continuation ray -> queue b+1 (wave-ballot compaction)
//       k_trace_pair    : one launch tracing the shadow rays of bounce b (any hit; unoccluded ->
//                         L[path] += contribution) and the extension rays of bounce b+1
//                         (closest hit), which start at the same hit points
//     RNG-coupled modes (Default / Layered: GlossyDiffuse::f consumes the path seed only
//     when the light is visible, GlossyDiffuse.h:230-343):
//       k_shade_a       : surface, coin, light pick -> shadow ray queue; item -> bucketed
//                         sample queue (and NEE queue at bounce 0, from the visibility table)
//       k_shadow_vis    : any-hit -> vis[shadow ray]; k_nee_compact: visible -> NEE queue
//       k_shade_nee     : f (may draw), NEE, over the bucketed NEE queue
//       k_shade_smp     : BSDF sample -> queue b+1, over the bucketed sample queue
//   accum_batch         : the batch's frames added to the destination in frame order, the same fp32
//                         order as the sequential reference accumulation (pt_accum.hip: k_accum, or
//                         the filtered or the mapped accumulate in its place)
//
// Every kernel reads queue lengths from device memory written by an earlier launch (kernel
// boundaries order the hand-off), so a whole batch of frames is enqueued without host round trips.
#include <type_traits>
#include <unordered_map>

#include "pt_internal.h"
#include "pt_resource.h"
#include "pt_shade.h"
#include "pt_skip.h"

namespace pt {

namespace {

constexpr int kBlockWF = 256;
// Trace kernels (k_extend, k_trace_pair, k_shadow_vis): workgroup size.  Every workgroup holds its
// own copy of the staged top BVH levels in LDS, so fewer, larger workgroups per CU leave room for
// more staged nodes at the same waves per SIMD: 512 threads with 100 nodes / 768 with 150 lost
// 2.9 / 7.0 % Lambert and 1.7 / 3.8 % Dielectric, Sponza-class +0.6 %.
#ifndef PT_TRACE_BLOCK
#define PT_TRACE_BLOCK 256
#endif
constexpr int kBlockTrace = PT_TRACE_BLOCK;
// LDS traversal stack entries per lane (PT_WF_STACK, pt_device.h): 11 KB per workgroup.
constexpr int kStack = PT_WF_STACK;
// Top BVH4 levels staged in LDS per trace workgroup (nodes 0 .. kLdsNodes-1, breadth-first: 49 =
// the three top levels (21) and 28 of the fourth, 6.1 KB).  With the 11-KB stack and the 9-KB
// triangle batches (below) a workgroup takes 26.1 KB, so a CU holds 6 workgroups, the 6 waves per
// SIMD the kernels' 80 VGPRs allow (v39, DESIGN.md §5: Lambert +2.4 %, Conductor +7.7 %,
// Dielectric +4.5 % over 5 waves with 14 entries and 57 nodes; the kernels wait on memory in
// more than half their cycles, and a sixth wave covers more of it).  Earlier sweeps at 5 waves
// (v34 tree): 0 / 21 / 41 / 85 nodes with a 16-entry stack -8.6 / -1.2 / 0 / -7.5 % Lambert.
#ifndef PT_LDS_NODES
#define PT_LDS_NODES 49
#endif
constexpr int kLdsNodes = PT_LDS_NODES;
// Wide trace workgroups (round 6): on one wavefront stream (Lambert, Default, Layered) the untextured
// trace kernels run 768-thread workgroups, two per CU, each staging 150 top nodes (levels 0-3 and 65
// of level 4) in LDS instead of six 256-thread workgroups with 49 each: the same 6 waves per SIMD,
// three times the staged nodes per workgroup.  Lambert +2.5 %, Default +0.6 %, Sponza-class +1.0 %;
// beside a second stream's shading kernels (Conductor, Dielectric) the 256-thread workgroups stay
// (Dielectric 3404 on two streams vs 3362 with wide workgroups on one).
#ifndef PT_TRACE_BLOCK_WIDE
#define PT_TRACE_BLOCK_WIDE 768
#endif
#ifndef PT_LDS_NODES_WIDE
#define PT_LDS_NODES_WIDE 150
#endif
constexpr int kBlockTraceWide = PT_TRACE_BLOCK_WIDE;
template <int BLK>
constexpr int lds_nodes_of() { return BLK == kBlockTrace ? kLdsNodes : PT_LDS_NODES_WIDE; }
// wave-batched triangle tests (pt_device.h wave_tri_batch): 2.25 KB of LDS per wave
// Trace kernels: 6 waves per SIMD (80 VGPRs, 3 spilled in cold paths)
#ifndef PT_WF_WAVES
#define PT_WF_WAVES 6
#endif
// the textured variants: 6 waves as well since round 6 (4 before; the textured atrium, config 5t,
// +1.6 % at 6, ±0 at 5, profiles/r06_ab/r06m_ab_tex_c5t.log).  They take the wide workgroups on
// one-stream calls like the untextured ones (+0.7 % config 5t, +1.0 % on the small textured scene,
// profiles/r06_ab/r06n_ab_widetex_*.log).
#ifndef PT_WF_WAVES_TEX
#define PT_WF_WAVES_TEX 6
#endif
constexpr int wf_waves(bool tex) { return tex ? PT_WF_WAVES_TEX : PT_WF_WAVES; }

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Look-ahead cancellation.  pt_render renders up to 64 frames ahead of
// the caller on speculation (pt_capi.cpp render_frame_image); when the camera or any other
// render state changes, those frames are useless and the next call must not wait behind them.
// The host publishes a new cancel epoch in pinned host memory (cancel_look_ahead); a batch
// enqueued under an older epoch then stops: every wave of the shading kernels checks at its
// start and returns, and the trace kernels stop refilling (trace_range), so what is still
// enqueued of the batch drains in launch gaps.  The host word is read over PCIe by few lanes
// (`relay`: the first lane of one block in 64, or of one wave per trace workgroup now and
// then), which raise the device word cancel_seen with an atomic max; everyone else polls that
// word with agent-scope loads (sc1: L2-served, MI355X_MICROARCH "visibility").  Epochs only
// grow, so a stale read never cancels a batch enqueued after the cancel.  A cancelled batch's
// queues stay consistent (every counted entry is written), its ring slot is discarded, and the
// next batch starts from zeroed counters.
__device__ __forceinline__ bool wf_cancel_poll(const WFState& W, bool relay) {
    if (relay) {
        const unsigned h = __hip_atomic_load(W.cancel_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_fetch_max(W.cancel_seen, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned v = __hip_atomic_load(W.cancel_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __builtin_amdgcn_readfirstlane(v) > W.cancel_epoch;  // wave-uniform
}
// Entry check of the shading and setup kernels: the wave returns when its batch is cancelled
// (a barrier later in the kernel waits only on the surviving waves of the workgroup).
__device__ __forceinline__ bool wf_cancelled(const WFState& W) {
    if (!W.cancel_seen) return false;  // not a speculative batch (kernel argument: uniform)
    return wf_cancel_poll(W, (blockIdx.x & 63) == 0 && threadIdx.x == 0);
}

// pt_set_debug_hold (tests only): the first kernel of a held speculative
// batch.  One lane waits until the host cancels the batch (a newer epoch in the pinned cancel
// word, relayed into cancel_seen as wf_cancel_poll does), releases the hold (the pinned release
// word), or 10 s of the 100-MHz wall clock pass, with an iteration bound behind that.  Every later
// kernel of the batch is queued behind it, so a test can move the camera while the batch is
// provably in flight, whatever the speed of the GPU.
__global__ void k_hold(WFState W) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    for (int it = 0; it < (1 << 22); ++it) {
        const unsigned h = __hip_atomic_load(W.cancel_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (h > W.cancel_epoch) {
            __hip_atomic_fetch_max(W.cancel_seen, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (__hip_atomic_load(W.hold_release, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;
        if (wall_clock64() - t0 > 1000000000ull) return;
        __builtin_amdgcn_s_sleep(64);
    }
}

// Hit record of a finished extension ray: (path, u, v, tri | back << 31), or a miss.  The
// shading kernels reconstruct the surface from (tri, u, v) and never read t, so the first word
// carries the path id and they skip the ray_o read.  The last three words are the lane's slot as the
// triangle batches left it (pt_device.h hit_slot_*).
__device__ __forceinline__ float4 hit_record(const TriBatchLds* slot, int path) {
    float u, v, code;
    hit_slot_words(slot, u, v, code);
    return make_float4(__int_as_float(path), u, v, code);
}

// Per-bounce counters: queue length and shadow-queue length, each on its own 128-B line
// (appends from different queues never contend for one L2 line).  Zeroed per frame.
// Default / Layered shading items are queued per bucket (shade_bucket): kNeeBuckets NEE and
// kShadeBuckets BSDF-sample counters follow the two queue counters.
constexpr int kShadeBuckets = 3;
// NEE buckets (round 6): 0 = conductor; 1 = kNeeCross, layered items whose light lies across the
// shading plane from the viewer, so that every other layered NEE wave runs the walk's
// compile-time path (layered_f_split; without it 70 % of Sponza-class's and 45 % of Layered's
// walk waves held such a lane, 4.2 / 1.6 % of the lanes); then per
// albedo class k (kNeeClasses) the layered items with a smooth (2 + 2k) and a rough (3 + 2k) top.
// The walk's Russian roulette ends walks over a dark bottom layer early, so a wave that mixes
// them with bright ones runs as long as its brightest lane: the class of an item is the largest
// channel of its albedo against PT_NEE_MID (classes >= 3) and PT_NEE_DARK (classes >= 2).
// Bucket q fills region q / 2 of W.nq from the front (q even) or the back (q odd): a bounce
// queues at most W.paths NEE items in all, so the two ends of a region never meet.
#ifndef PT_NEE_CLASSES
#define PT_NEE_CLASSES 2
#endif
#ifndef PT_NEE_DARK
#define PT_NEE_DARK 0.5f
#endif
#ifndef PT_NEE_MID
#define PT_NEE_MID 0.7f
#endif
constexpr int kNeeClasses = PT_NEE_CLASSES;
constexpr int kNeeBuckets = 2 + 2 * kNeeClasses;
constexpr int kNeeRegions = kNeeBuckets / 2;
constexpr int kNeeCross = 1;
static_assert(kNeeBuckets <= 8, "a shadow ray's item code holds the NEE bucket in bits 28-30");
// (The BSDF-sample items keep the kShadeBuckets sample buckets: a dark class of them, as
// PT_NEE_DARK for the NEE items, was not kept)
constexpr int kCnt = 5 + kNeeBuckets + kShadeBuckets;
constexpr int kCntStride = 32;  // ints per counter = 128 B
// kPool*: the run-time ray pools of k_trace_pair, k_extend and k_shadow_vis (RayPool)
enum { kQueue = 0, kShadowQ = 1, kNee0 = 2, kSmp0 = 2 + kNeeBuckets, kPool = 2 + kNeeBuckets + kShadeBuckets, kPoolExt, kPoolSh };
__device__ __forceinline__ int* cnt(const WFState& W, int b, int k) { return W.count + (kCnt * b + k) * kCntStride; }
// Slot `slot` of NEE bucket q in W.nq
__device__ __forceinline__ size_t nee_index(const WFState& W, int q, int slot) {
    const size_t r = (size_t)(q >> 1) * W.paths;
    return (q & 1) ? r + W.paths - 1 - slot : r + slot;
}
// NEE bucket of a layered item (sample bucket bk 1 / 2: smooth / rough top) from its albedo
__device__ __forceinline__ int nee_layered_bucket(int bk, f3 albedo) {
    const float m = fmaxf(fmaxf(albedo.x, albedo.y), albedo.z);
    int cls = 0;
    if (kNeeClasses >= 3 && m < PT_NEE_MID) cls = 1;
    if (kNeeClasses >= 2 && m < PT_NEE_DARK) cls = kNeeClasses - 1;
    return 2 + 2 * cls + (bk - 1);
}
// Slot `slot` of sample bucket q in W.sq: region q from the front
__device__ __forceinline__ size_t smp_index(const WFState& W, int q, int slot) {
    return (size_t)q * W.paths + slot;
}
// Path throughput | seed.  W.beta in path order (the phases of a bounce read it by path), except
// in the Lambert mode: in queue order next to the ray, ping-pong like ray_o / ray_d (queue b
// in W.beta for even b, W.beta_q for odd b), so k_shade_fused streams it instead of gathering it
// by path: a random 16-B read costs a 64-B line fetch (DESIGN.md §4 counter calibration).
// Queue 0 is in path order, so k_camera's W.beta[q] serves both layouts.
__device__ __forceinline__ float4* queue_beta(const WFState& W, int b) { return (b & 1) ? W.beta_q : W.beta; }
inline size_t count_bytes(int max_bounces) { return sizeof(int) * kCntStride * kCnt * (size_t)(max_bounces + 2); }

// Shading kernels: 1024-thread blocks, one queue item per thread over a grid sized to the
// queue capacity; blocks past the live queue length exit at once.  Queue appends are
// aggregated per block (one atomic per 1024 items): same-address atomics serialise at the
// L2 (≈90 per µs per word, MI355X_MICROARCH.md "dequeue"), and one atomic per wave cost
// ≈0.4 ms per shading launch at 2 M paths.  (Measured alternatives, see DESIGN.md:
// persistent grids with one atomic fetch head serialise the same way, and chunked fetching
// starves waves.)
constexpr int kBlockSh = 1024;
constexpr int kWavesSh = kBlockSh / 64;
#ifndef PT_SHA_BLOCK
#define PT_SHA_BLOCK 1024  // k_shade_a (Default / Layered); 512 / 256: +0.7 % / -3 %, DESIGN.md §5
#endif
constexpr int kBlockShA = PT_SHA_BLOCK, kWavesShA = kBlockShA / 64;
// k_shade_fused waves per SIMD: a CU holds two 1024-thread blocks only at <= 64 VGPRs (8 waves
// per SIMD); at 65..128 VGPRs one block per CU halves the occupancy (measured: 66 VGPRs made
// the Lambert shade 37 % slower).  Lambert fits 64 VGPRs untextured; Dielectric spills ~22
// VGPRs at 64 and still runs 6 % faster (1,795 -> 1,905 Msamples/s); Conductor spills ~41
// and is 1.4 % slower, so it keeps its natural allocation.
#ifndef PT_SHF_WAVES
#define PT_SHF_WAVES 8
#endif
#ifndef PT_SHF_WAVES_OTHER
#define PT_SHF_WAVES_OTHER 1
#endif
constexpr int shf_waves(int mode) { return (mode == 1 || mode == 3) /*Lambert, Dielectric*/ ? PT_SHF_WAVES : PT_SHF_WAVES_OTHER; }
// k_shade_fused / k_shade0_pixel block size per mode.  Conductor and Dielectric run in 256-thread
// blocks: +12.6 % and +6.1 % with the two wavefront streams; Lambert loses 5 % at
// 256, so it keeps 1024.
#ifndef PT_SHF_BLOCK_DIELECTRIC
#define PT_SHF_BLOCK_DIELECTRIC 256
#endif
#ifndef PT_SHF_BLOCK_CONDUCTOR
#define PT_SHF_BLOCK_CONDUCTOR 256
#endif
#ifndef PT_SHF_BLOCK_LAMBERT
#define PT_SHF_BLOCK_LAMBERT 1024
#endif
constexpr int shf_block(int mode) {
    return mode == 3 ? PT_SHF_BLOCK_DIELECTRIC : mode == 2 ? PT_SHF_BLOCK_CONDUCTOR : PT_SHF_BLOCK_LAMBERT;
}
// k_shade_nee / k_shade_smp (Default / Layered: the stochastic GlossyDiffuse eval, the sample)
// run in 256-thread blocks at 4 waves per SIMD (128 VGPRs).  (Round 2 before the bucketed
// queues: one kernel with both phases behind a block barrier, where 256-thread blocks beat
// 1024 / 512 / 128 / 64 threads: Layered 433 vs 375 / 431 / 427 / 425 Msamples/s)
#ifndef PT_SHB_BLOCK
#define PT_SHB_BLOCK 256
#endif
#ifndef PT_SHB_WAVES
#define PT_SHB_WAVES 4  // waves per SIMD the register allocator must allow (128 VGPRs)
#endif
#ifndef PT_SMP_WAVES
#define PT_SMP_WAVES 5  // k_shade_smp: 96 VGPRs, 4-12 spilled; configs 3 / 5 / Layered +0.6 / +0.5 / +0.9 % over 4
#endif
constexpr int kBlockShB = PT_SHB_BLOCK;

// Block-wide compaction: every thread of the block calls this (uniform control flow);
// threads with pred get consecutive slots.  `lds` is WAVES + 1 ints of shared memory
// private to this call site.
template <int WAVES>
__device__ __forceinline__ int block_append(int* counter, bool pred, int* lds) {
    const unsigned long long m = __ballot(pred ? 1 : 0);
    const int prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 0) lds[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < WAVES; ++w) {
            const int c = lds[w];
            lds[w] = tot;
            tot += c;
        }
        lds[WAVES] = tot > 0 ? atomicAdd(counter, tot) : 0;
    }
    __syncthreads();
    return lds[WAVES] + lds[wave] + prefix;
}

// Block-wide append into K bucket regions (counter of bucket k at counter0 + k * kCntStride):
// threads with bucket k in [0, K) get consecutive slots of region k in thread order, bucket < 0
// appends nothing.  One atomic per non-empty bucket per block.  `lds` holds K * (WAVES + 1) ints.
template <int WAVES, int K>
__device__ __forceinline__ int block_append_k(int* counter0, int bucket, int* lds) {
    const int wave = threadIdx.x >> 6;
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long m = __ballot(bucket == k ? 1 : 0);
        if (bucket == k) mine = m;
        if (lane_id() == 0) lds[k * WAVES + wave] = __popcll(m);
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        int tot = 0;
        for (int w = 0; w < WAVES; ++w) {
            const int c = lds[k * WAVES + w];
            lds[k * WAVES + w] = tot;
            tot += c;
        }
        lds[K * WAVES + k] = tot > 0 ? atomicAdd(counter0 + k * kCntStride, tot) : 0;
    }
    __syncthreads();
    if (bucket < 0) return 0;
    const int pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
    return lds[K * WAVES + bucket] + lds[bucket * WAVES + wave] + pre;
}

// Bucket of a Default / Layered shading item.  The items of one bucket run the same BSDF code
// path, so the NEE and sample kernels take them from per-bucket queue regions and their waves
// hold one kind of item: 0 = conductor (Default mode's metallic coin, devicePrograms.cu:400),
// 1 / 2 = the layered BSDF with a smooth / rough top interface (layered_f's topSpec: alpha =
// roughness^2 < 1e-3, GlossyDiffuse.h).  These are the sample buckets; the NEE items split the
// layered ones further (nee_layered_bucket, kNeeCross).
template <int MODE>
__device__ __forceinline__ int shade_bucket(bool conductor, float roughness) {
    if (MODE == kModeDefault && conductor) return 0;
    return sqr(roughness) < 1e-3f ? 1 : 2;
}
constexpr int kItemBits = 28;  // a queue item index is < 2^28 (kMaxWFPaths); the bucket sits above it

// Paths of nf consecutive frames are in flight together (path q = f * P + pixel), so every
// launch works on nf frames' queues: fewer launches and one SIMT tail per nf frames.
// lean (fused modes with the primary dedup): k_extend traces only frame 0's camera rays and the
// bounce-0 k_shade_fused derives the rest of the path state itself (shade0), so only frame 0's
// rays are written -- the other frames' copies, throughputs and radiances are never read.
__global__ __launch_bounds__(kBlockWF) void k_camera(WFState W, DevLaunch L, uint32_t frame0, int nf, int lean) {
    const int P = launch_pixels(L);
    const int Q = P * nf;
    if (wf_cancelled(W)) return;  // no barrier below; the queue count stays 0 if wave 0 of block 0 returns
    if (lean) {
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < P; q += gridDim.x * blockDim.x) {
            f3 o, d;
            const int ip = L.pixel_map ? L.pixel_map[q] : q;  // a mapped launch has row0 = 0: camera_ray's rows are the image's
            camera_ray(L, ip % L.width, ip / L.width, o, d);
            W.ray_o[0][q] = make_float4(o.x, o.y, o.z, __int_as_float(q));
            W.ray_d[0][q] = make_float4(d.x, d.y, d.z, 0.0f);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) *cnt(W, 0, kQueue) = Q;
        return;
    }
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < Q; q += gridDim.x * blockDim.x) {
        const int f = q / P, p = q - f * P;
        const int ip = L.pixel_map ? L.pixel_map[p] : p;  // as above
        const int x = ip % L.width, y = ip / L.width;
        f3 o, d;
        uint32_t pixel;  // the seed's pixel index
        if (L.ss_cells) {  // pt_set_pixel_filter: the frame's cell of this pixel, a pixel of the ss-fold image
            const int* cell = L.ss_cells + 2 * ((frame0 + (uint32_t)f) & (uint32_t)(L.ss * L.ss - 1));
            const int vx = L.ss * x + cell[0], vy = L.ss * (y + L.row0) + cell[1], vw = L.ss * L.width;
            camera_ray_at(L, vx, vy, vw, L.ss * L.image_height, o, d);
            pixel = (uint32_t)(vw * vy + vx);
        } else {
            camera_ray(L, x, y, o, d);
            pixel = (uint32_t)image_pixel(L, p);
        }
        W.ray_o[0][q] = make_float4(o.x, o.y, o.z, __int_as_float(q));
        W.ray_d[0][q] = make_float4(d.x, d.y, d.z, 0.0f);
        const uint32_t seed = tea16(pixel, frame0 + (uint32_t)f);  // devicePrograms.cu:631
        W.beta[q] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(seed));
        W.L[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *cnt(W, 0, kQueue) = Q;
}

#ifndef PT_REFILL_MIN
#define PT_REFILL_MIN 16  // idle lanes before a wave refills (24 before the triangle batches;
                          // with them 12 / 16 / 20 / 32: -1 / 0 / -0 / -5 %)
#endif
constexpr int kRefillMin = PT_REFILL_MIN;

#ifndef PT_TRI_BATCH
#define PT_TRI_BATCH 20  // lanes with a pending leaf before a wave runs its triangle batch (8 / 12 / 16 /
                         // 20 / 24 / 32: -7 / -2 / -0.3 / 0 / -0.3 / -5 %)
#endif

// This wave's static slice of a queue of length n (grid sized to residency, so every wave
// is resident and slices balance statistically; no fetch atomics).  Slices are contiguous: chunks
// dealt round-robin to the waves were not kept.
__device__ __forceinline__ void wave_slice(int n, int& first, int& end) {
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int per = (n + nwaves - 1) / nwaves;
    first = min(n, wave * per);
    end = min(n, first + per);
}

typedef float pt_v4f __attribute__((ext_vector_type(4)));
// Queue records that a kernel streams once are loaded and stored non-temporally, so that they do
// not evict the lines its gathers reuse.  k_shade_fused and k_shade0_pixel (memory-bound, ≈ 66 % of
// HBM peak): Lambert +2 %, Dielectric and Conductor +0.4 %.  k_trace_pair: 19 % less traffic of
// its own, rate ±0.2 %.  k_extend and k_shadow_vis use plain loads and stores (configs 3 / 5
// +0.1 / +0.3 %, Lambert -0.6 % with the hint: not kept).  DESIGN.md §5.
__device__ __forceinline__ float4 ldqs(const float4* p) {
    const pt_v4f v = __builtin_nontemporal_load(reinterpret_cast<const pt_v4f*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void stqs(float4* p, float4 v) {
    __builtin_nontemporal_store(pt_v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<pt_v4f*>(p));
}

// Lane-refilling trace loop over a queue slice: `load(ri, state)` loads ray ri's records into the
// lane's state (origin, direction, tmax in `best`, and whatever else it passes to init in fields
// that init computes afterwards: the lane's old state is dead, so the records take no registers of
// their own), `init(ri, state, slot)` completes the state and initialises the lane's hit slot
// (pt_device.h hit_slot_*); `finish(ri, state, slot)` consumes a finished ray, whose answer is in
// the slot.  A finish that returns a token is split in two: its loads are issued before the refill's
// record loads and `commit(token, slot)` (its stores) runs after them, so the two memory round
// trips of a batch block overlap; commit runs before init, so it still reads the
// finished ray's slot.  A lane whose traversal ends parks
// (`done`) until enough lanes are idle; then the wave runs one batch block that finishes the
// parked rays and refills the idle lanes with the next rays of the slice.  The triangle
// batches take acceptable hits only (wave_tri_batch), so a finished ray's answer is final.
// The rays of a trace launch dealt at run time (PT_TRACE_POOL): queue range [begin, end), handed
// out in chunks of PT_POOL_CHUNK through the counter ctr (zeroed with the queue counters) to the
// waves whose static slices ran out.
#ifndef PT_TRACE_POOL
#define PT_TRACE_POOL 60  // percent of k_trace_pair's rays in the pool (0: static slices only)
#endif
#ifndef PT_TRACE_POOL_X
#define PT_TRACE_POOL_X 60  // the same for k_extend and k_shadow_vis
#endif
#ifndef PT_POOL_CHUNK
#define PT_POOL_CHUNK 512
#endif
// launches of fewer rays than this many per wave keep static slices only: a one-frame call's
// launches (about 300 rays per wave) ran 40 % slower with the pool
#ifndef PT_POOL_MIN_PER_WAVE
#define PT_POOL_MIN_PER_WAVE 2048
#endif
__device__ __forceinline__ bool pool_pays(int n) {
    const long long nwaves = (long long)((gridDim.x * blockDim.x) >> 6);
    return (long long)n >= nwaves * PT_POOL_MIN_PER_WAVE;
}
struct RayPool {
    int* ctr = nullptr;
    int begin = 0, end = 0;
};

struct NoCommit {
    template <class T>
    __device__ void operator()(const T&, const TriBatchLds*) const {}
};
template <int ANY, bool STATS, bool TEX, int BLK, class Load, class Init, class Finish, class Commit = NoCommit>
__device__ __forceinline__ void trace_range(const DevScene& S, int next, int end, int* stk, TriBatchLds* tri_lds,
                                            TravStats& ts, const WFState& W, Load load, Init init, Finish finish,
                                            Commit commit = Commit{}, RayPool pool = RayPool{}) {
    using Tok = decltype(finish(0, *static_cast<const TravRay*>(nullptr), tri_lds));
    constexpr bool kSplit = !std::is_void_v<Tok>;
    using TokS = std::conditional_t<kSplit, Tok, int>;
    int spill[kSpillDepth];
    TravRay st;
    int ri = -1;
    bool done = false;
    // the slice bounds are wave-uniform: keeping them (and the refill bookkeeping) in SGPRs
    // makes the per-step refill test scalar work (it was VALU, with an f64 min from the
    // unsigned popcount; ±0.3 %)
    next = __builtin_amdgcn_readfirstlane(next);
    end = __builtin_amdgcn_readfirstlane(end);
    // look-ahead cancellation (wf_cancel_poll): a cancelled batch's wave stops taking rays from its
    // slice (it finishes the ones in flight), at the start and at every 16th batch block; one wave
    // in eight workgroups relays the host word at every 64th
    uint32_t npoll = 0;
    int* pctr = pool.ctr;
    if (W.cancel_seen && wf_cancel_poll(W, false)) {
        end = next;
        pctr = nullptr;
    }
    while (true) {
        // batch block once enough lanes idle (it costs the wave about as much as a step), and
        // at every step once the slice is drained
        if ((int)__popcll(__ballot(ri < 0 || done)) >= kRefillMin || next >= end) {
            if (W.cancel_seen && (++npoll & 15) == 0 &&
                wf_cancel_poll(W, (npoll & 63) == 0 && (blockIdx.x & 7) == 0 && threadIdx.x == 0)) {
                end = next;
                pctr = nullptr;
            }
            if (pctr && next >= end) {  // static share drained: the next chunk of the pool
                int base = 0;
                if ((threadIdx.x & 63) == 0) base = atomicAdd(pctr, PT_POOL_CHUNK);
                base = __builtin_amdgcn_readfirstlane(__shfl(base, 0, 64));
                next = min(pool.begin + base, pool.end);
                end = min(next + PT_POOL_CHUNK, pool.end);
                if (next >= pool.end) pctr = nullptr;
            }
#if PT_CYCLE_PROBE
            const uint64_t c0 = probe_clock();
#else
            if (STATS) ts.refills++;
#endif
            TokS tok{};
            const bool fin = done;
            if (done) {  // the triangle batches took acceptable hits only: the answer stands
                if constexpr (kSplit)
                    tok = finish(ri, st, tri_lds);
                else
                    finish(ri, st, tri_lds);
                ri = -1;
                done = false;
            }
            const unsigned long long m = __ballot(ri < 0);
            const int pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const bool take = ri < 0 && next + pre < end;
            if (take) {
                ri = next + pre;
                load(ri, st);
            }
            next = min(next + (int)__popcll(m), end);
            if constexpr (kSplit) {
                if (fin) commit(tok, tri_lds);
            }
            if (take) {
                init(ri, st, tri_lds);
                if (STATS) ts.rays++;
                done = S.ntri <= 0;  // empty scene: no BVH root, every ray misses
            }
#if PT_CYCLE_PROBE
            if (STATS) ts.refills += (uint32_t)(probe_clock(st.best) - c0);
#endif
        }
        const bool active = ri >= 0 && !done;
        const unsigned long long act = __ballot(active);
        // only parked lanes left: the next batch block finishes them.  The loop keeps a single
        // back edge (no `continue`): with two latch paths the compiler copied ~20 registers of lane
        // state between them every iteration (12 % of the kernel's VALU instructions)
        if (!act && !__ballot(ri >= 0)) break;
        // postponed leaves: test the pending leaves once enough lanes hold one, or when too few
        // lanes have a node left to visit (then the leaves are the work)
        const int n_act = __popcll(act);
        const int n_leaf = __popcll(__ballot(active && st.leaf != kEmptyChild));
        const int n_node = __popcll(__ballot(active && st.cur >= 0));
        const bool tri_ok = n_leaf >= min(PT_TRI_BATCH, n_act) || 2 * n_node < n_act;
        if (STATS) {
            ts.steps++;
#if !PT_CYCLE_PROBE
            ts.active += n_act;
            ts.node_steps += n_node > 0;
            ts.tri_steps += tri_ok && n_leaf > 0;
#endif
        }
#if PT_CYCLE_PROBE
        const uint64_t c1 = probe_clock();
#endif
        // the triangles of every pending leaf in one wave batch (pt_device.h wave_tri_batch),
        // then the node half of the step
        if (tri_ok && n_leaf > 0) {  // wave-uniform
            const bool occluded = wave_tri_batch<ANY, STATS, TEX>(S, st, active && st.leaf != kEmptyChild, tri_lds, ts);
            if (active && occluded) done = true;
        }
#if PT_CYCLE_PROBE
        const uint64_t c2 = probe_clock(st.best);
        if (STATS) ts.tri_steps += (uint32_t)(c2 - c1);
#endif
        if (STATS) {  // distinct global nodes among the lanes about to load one (pt_get_trace_coherence)
            const bool g = active && !done && st.cur >= S.n_lds;
            unsigned long long rem = __ballot(g);
            if (rem) {
                ts.coh_lanes += (uint32_t)__popcll(rem);
                int distinct = 0;
                while (rem) {
                    const int node = __shfl(st.cur, __ffsll((long long)rem) - 1, 64);
                    rem &= ~__ballot(g && st.cur == node);
                    ++distinct;
                }
                ts.coh[distinct <= 2 ? distinct - 1 : distinct <= 4 ? 2 : distinct <= 8 ? 3 : distinct <= 16 ? 4 : 5]++;
            }
        }
        if (active && !done && trav_node_step<ANY, STATS, kStack>(S, st, stk, BLK, spill, ts)) done = true;
#if PT_CYCLE_PROBE
        if (STATS) {  // node half: until its loads landed (active), the rest (node_steps)
            const uint64_t c4 = probe_clock(st.cur);
            const unsigned long long ml = __ballot(ts.probe_t > c2);
            const uint64_t tl = ml ? (uint64_t)__shfl((long long)ts.probe_t, __ffsll((long long)ml) - 1, 64) : c2;
            ts.active += (uint32_t)(tl - c2);
            ts.node_steps += (uint32_t)(c4 - tl);
        }
#endif
    }
}

// A trace kernel's queue range [first, end): the workgroup's LDS (per-lane stacks, the staged top
// BVH levels, the triangle batches), then the lane-refilling loop.
template <int ANY, bool STATS, bool TEX, int BLK, class Load, class Init, class Finish, class Commit = NoCommit>
__device__ __forceinline__ void trace_queue(DevScene S, int first, int end, TravStats& ts, const WFState& W, Load load,
                                            Init init, Finish finish, Commit commit = Commit{}, RayPool pool = RayPool{}) {
    constexpr int kNodes = lds_nodes_of<BLK>();
    __shared__ int stack[kStack * BLK];
    __shared__ BNode4 top[kNodes > 0 ? kNodes : 1];
    __shared__ TriBatchLds tri_batch[BLK / 64];
    stage_top_nodes<kNodes>(S, top);
    trace_range<ANY, STATS, TEX, BLK>(S, first, end, stack + threadIdx.x, tri_batch + (threadIdx.x >> 6), ts, W, load,
                                      init, finish, commit, pool);
}

template <int ANY, bool STATS, bool TEX, int BLK, class Load, class Init, class Finish>
__device__ __forceinline__ void trace_slice(const DevScene& S, int n, TravStats& ts, const WFState& W, Load load,
                                            Init init, Finish finish, int* pool_ctr) {
    int next, end;
    RayPool pool;
    pool.end = n;
    if (PT_TRACE_POOL_X > 0 && pool_pays(n)) {
        pool.ctr = pool_ctr;
        pool.begin = n - (int)((long long)n * PT_TRACE_POOL_X / 100);
    } else {
        pool.begin = n;
    }
    wave_slice(pool.begin, next, end);
    trace_queue<ANY, STATS, TEX, BLK>(S, next, end, ts, W, load, init, finish, NoCommit{}, pool);
}

// A ray's queue records into the lane's state (trace_range `load`): origin | path and
// direction | tmax.
__device__ __forceinline__ void load_ray(TravRay& st, float4 o, float4 d) {
    st.o = mk(o.x, o.y, o.z);
    st.path = __float_as_int(o.w);
    st.d = mk(d.x, d.y, d.z);
    st.best = d.w;
}

// Closest hit of queue b.  `dup` > 1 (bounce 0 only): the queue holds `dup` copies of the same
// camera rays (one per frame of the batch: the reference has no pixel jitter, so a pixel's ray
// is identical in every frame, devicePrograms.cu:601-623), so only the first n / dup are traced
// and each hit record is written to all copies.  The records are bit-identical to tracing every
// copy; DESIGN.md §5 gives the A/B.
template <bool STATS, bool TEX, int BLK = kBlockTrace>
__global__ __launch_bounds__(BLK, wf_waves(TEX)) void k_extend(DevScene S, WFState W, int b, int dup,
                                                                  int copies, unsigned long long* counters) {
    const int n = *cnt(W, b, kQueue);
    const int n_trace = n / dup;
    const float4* ro = W.ray_o[b & 1];
    const float4* rd = W.ray_d[b & 1];
    TravStats ts;
    trace_slice<kRayClosest, STATS, TEX, BLK>(
        S, n_trace, ts, W,
        [&](int ri, TravRay& st) { load_ray(st, ro[ri], rd[ri]); },
        [&](int ri, TravRay& st, TriBatchLds* slot) {
            trav_init(st, st.o, st.d, 0.0f, 100.0f);
            hit_slot_init_closest(slot, 100.0f);
        },
        [&](int ri, const TravRay& st, const TriBatchLds* slot) {
            // copy k of a bounce-0 ray is path st.path + k * n_trace (queue 0 is in path order);
            // copies = 1: k_shade0_pixel reads the pixel's one record for all its frames
            float4 h = hit_record(slot, st.path);
            for (int k = 0; k < copies; ++k) {
                h.x = __int_as_float(st.path + k * n_trace);
                W.hit[ri + (size_t)k * n_trace] = h;
            }
        }, cnt(W, b, kPoolExt));
    if (blockIdx.x == 0 && threadIdx.x == 0 && counters) {
        atomicAdd(&counters[kCtrSegments], (unsigned long long)n);
        atomicAdd(&counters[kCtrTraceRays], (unsigned long long)n_trace);
        atomicAdd(&counters[kCtrTraceBytes], (32ull + 16ull * (unsigned long long)copies) * (unsigned long long)n_trace);
    }
    flush_trav_stats<STATS>(counters, ts);
}

__device__ __forceinline__ Hit decode_hit(float4 hv) {
    Hit h;
    const int code = __float_as_int(hv.w);
    h.t = hv.x;
    h.u = hv.y;
    h.v = hv.z;
    h.back = code != kMissTri && (code & (int)0x80000000);
    h.tri = code == kMissTri ? -1 : (code & 0x7fffffff);
    return h;
}

// Adds the block's table answers to pt_stats.lit_table_answers: every wave leaves its count in
// lds[wave] before one of the block's barriers (lit_count_wave), thread 0 adds them up after it.
__device__ __forceinline__ void lit_count_wave(bool answered, int* lds) {
    const unsigned long long m = __ballot(answered ? 1 : 0);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = __popcll(m);
}
template <int WAVES, int SLOT = kCtrLitAnswers>
__device__ __forceinline__ void lit_count_block(const DevLaunch& L, const int* lds) {
    if (threadIdx.x != 0 || !L.counters) return;
    int tot = 0;
    for (int w = 0; w < WAVES; ++w) tot += lds[w];
    if (tot > 0) atomicAdd(&L.counters[SLOT], (unsigned long long)tot);
}
// The occluder candidate table (pt_lit.hip k_occ_build): `t` = the entry light * cells + cell of a
// shadow ray the lit table left open (its origin is offset to the light's side of a triangle with
// cells), -1 or a triangle.  True: the candidate passes the tracer's own test on this very ray -- tri_test, then tri_accept_in
// with tmin 0, the ray's tmax, and inv and io formed as trav_init forms them -- so k_trace_pair /
// k_shadow_vis would answer "occluded": they reach that triangle (every BVH box that holds it
// contains its padded box) or stop earlier at another hit.  That holds for ANY entry, so a stale or
// wrong one only costs the test.  A cut-out triangle (E2.w != 0, alpha_cut may drop its hits in the
// textured kernels) never answers.  pt_stats.occluder_table_answers counts them (kCtrOccAnswers).
template <bool TEX>
__device__ __forceinline__ bool occ_answers(const DevScene& S, int t, f3 o, f3 d, float tmax) {
    if (t < 0) return false;
    const float4 A = S.isect[3 * t], E1 = S.isect[3 * t + 1], E2 = S.isect[3 * t + 2];
    float th, uh, vh;
    bool bk;
    if (!tri_test(A, E1, E2, o, d, th, uh, vh, bk)) return false;
    if (TEX && __float_as_int(E2.w) != 0) return false;
    const f3 inv = safe_inv(d);
    return tri_accept_in(A, E1, E2, inv, mk(o.x * inv.x, o.y * inv.y, o.z * inv.z), 0.0f, tmax, th);
}

// The skip table (pt_skip.h) in the fused shading kernels.  kSkipCode: the material modes whose kernels
// carry the lookup (like kOcc, a mode keeps it only where it measured a gain).
// skip_words: both sides' words of the hit triangle, one 8-byte gather issued beside the surface
// records.  skip_orient: x = the word of the side sf.ng points to (the stored winding's, or the other
// where sf.ng_back says so), y = the other side's.  skip_pick: the word of the side continue_path
// offsets the origin to, +-sf.ng, or 0 ("none") unless the normalised direction d the kernel writes
// climbs from that side, dot(d, +-sf.ng) > kSkipMinCos in fp32 (a smooth shading normal can send a
// sampled direction below the geometric plane).  Lambert never samples below the surface
// (lambert_sample forces z >= 0, as kShareOrigin relies on), so its kernels keep one word.
template <int MODE>
constexpr bool kSkipCode = MODE == kModeLambert || MODE == kModeConductor || MODE == kModeDielectric;
__device__ __forceinline__ uint2 skip_words(const DevLaunch& L, int tri) {
    return reinterpret_cast<const uint2*>(L.skip_tab)[tri];
}
__device__ __forceinline__ uint2 skip_orient(uint2 w, const SurfaceHit& sf) {
    return sf.ng_back ? make_uint2(w.y, w.x) : w;
}
template <int MODE>
__device__ __forceinline__ bool skip_under(const BSample& bs) {  // continue_path's test
    return MODE != kModeLambert && dot(bs.dir, mk(0.0f, 0.0f, 1.0f)) < 0.0f;
}
__device__ __forceinline__ uint32_t skip_pick(uint2 w, const SurfaceHit& sf, bool under, f3 d) {
    const float up = dot(d, sf.ng);
    const bool climbs = (under ? -up : up) > kSkipMinCos;
    return climbs ? (under ? w.y : w.x) : 0u;
}

// Bounce-0 shadow dedup (with primary dedup): a pixel's first hit is the same in every frame
// of the batch, so its shadow ray toward light li is too.  k_shadow0_setup builds one shadow
// ray per (pixel, light) from the frame-0 hit, k_shadow_vis traces them into W.vis[light *
// pixels + pixel], and the bounce-0 shading reads that table instead of tracing a shadow ray
// per path.  Same rays, same any-hit answers: the images stay bit-identical.
__device__ __forceinline__ int vis0_index(const DevLaunch& L, int path, int li) {
    const int P1 = launch_pixels(L);
    return li * P1 + path % P1;  // light-major (coherent shadow rays); path = frame * P1 + pixel
}

template <bool TEX>
__global__ __launch_bounds__(kBlockWF) void k_shadow0_setup(DevScene S, DevLaunch L, WFState W) {
    const int P1 = launch_pixels(L);
    const int nl = L.n_lights;
    const int n = P1 * nl;
    if (wf_cancelled(W)) return;  // no barrier below
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const int li = k / P1, p = k - li * P1;
        const Hit h = decode_hit(W.hit[p]);  // frame 0's copy (queue 0 is in path order)
        float4 so = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(k)), sd = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
        if (h.tri >= 0) {
            const float4 c = W.ray_d[0][p];
            SurfaceHit sf;
            reconstruct<TEX>(S, h, mk(c.x, c.y, c.z), sf);
            f3 o, d;
            float tmax;
            shadow_ray(sf.pos, sf.ng, light_vec(L.lights[li], sf.pos), o, d, tmax);
            so = make_float4(o.x, o.y, o.z, __int_as_float(k));
            sd = make_float4(d.x, d.y, d.z, tmax);
        }
        W.sh_o[k] = so;
        W.sh_d[k] = sd;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *cnt(W, 0, kShadowQ) = n;
}

// shade0 (bounce 0 after a lean k_camera): the path state is the camera's -- throughput 1, seed
// tea16(pixel, frame) (devicePrograms.cu:631), radiance 0, direction that of the pixel's frame-0
// ray (queue 0 is in path order) -- so it is derived here instead of read, and every path's
// radiance is written rather than updated.
template <int MODE, bool TEX, bool SHADE0>
__global__ __launch_bounds__(shf_block(MODE), shf_waves(MODE)) void k_shade_fused(DevScene S, DevLaunch L, WFState W, int b, int vis0) {
    constexpr bool shade0 = SHADE0;
    // Lambert (memory-bound, 56 VGPRs): the throughput in queue order (queue_beta), +1.6 %; the
    // Conductor and Dielectric kernels are register-bound, and holding it across the appends
    // cost them 1-2 %, so they gather it by path
    constexpr bool kBetaQ = MODE == kModeLambert;
    constexpr bool kShareOrigin = MODE == kModeLambert;
    constexpr int kBlock = shf_block(MODE), kWaves = kBlock / 64;
    const int n = *cnt(W, b, kQueue);
    const float4* rd = W.ray_d[b & 1];
    float4* no = W.ray_o[(b + 1) & 1];
    float4* nd = W.ray_d[(b + 1) & 1];
    __shared__ int lds_sh[kWaves + 1], lds_q[kWaves + 1];
    __shared__ int lds_lit[kWaves];
    // the occluder candidates: Lambert only -- the register-bound Conductor and Dielectric kernels
    // spill more with the code present even when the table is off
    constexpr bool kOcc = MODE == kModeLambert;
    __shared__ int lds_occ[kOcc ? kWaves : 1];
    const bool lit = !vis0 && L.lit_tri;  // the lit table answers this bounce's NEE tests where it can
    const bool occ = kOcc && lit && L.occ_tab;
    const bool skip = kSkipCode<MODE> && L.skip_tab;  // continuation rays carry a skip word (pt_skip.h)
    if (blockIdx.x == 0 && threadIdx.x == 0 && L.counters) atomicAdd(&L.counters[kCtrShadeItems], (unsigned long long)n);
    if ((int)(blockIdx.x * kBlock) >= n) return;  // block-uniform
    {
        const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
        // a cancelled wave takes no item but still joins the block's appends (block_append)
        const bool valid = i < n && !wf_cancelled(W);
        bool emit_shadow = false, emit_next = false, lit_answer = false;
        f3 so, sdir, contrib, o, d, beta;
        uint32_t seed = 0;
        float stmax = 0.0f;
        int path = 0;
        int occ_t = -1;  // the shadow ray's entry of the occluder table: -1 or a triangle
        uint32_t skip_w = 0;  // the continuation ray's skip word
        const int P1 = launch_pixels(L);
        float4 l0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // shade0: the path's radiance after bounce 0
        if (valid) {
            const float4 hv = ldqs(W.hit + i);
            // the queue-order records go out beside the hit record instead of after it: they do not
            // depend on it, and waiting for the hit first put two HBM round trips in a row (Lambert
            // +2 %)
            const float4 c_q = shade0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : ldqs(rd + i);
            const float4 bv_q = (!shade0 && kBetaQ) ? ldqs(queue_beta(W, b) + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            path = __float_as_int(hv.x);
            const Hit h = decode_hit(hv);
            if (h.tri >= 0) {  // a miss ends the path (__miss__radiance :576-583)
                const int lit_c = lit ? lit_cell(L, h) : -1;  // fetched beside the surface records
                const uint2 skip2 = skip ? skip_words(L, h.tri) : make_uint2(0u, 0u);  // and so are both sides' words
                const float4 c = shade0 ? ldqs(rd + path % P1) : c_q;
                d = mk(c.x, c.y, c.z);
                SurfaceHit sf;
                reconstruct<TEX>(S, h, d, sf);
                if (shade0) {
                    seed = tea16((uint32_t)image_pixel(L, path % P1), L.frame_base + (uint32_t)(path / P1));
                    beta = mk(1.0f, 1.0f, 1.0f);
                } else {
                    float4 bv = kBetaQ ? bv_q : ldqs(W.beta + path);
                    seed = __float_as_uint(bv.w);
                    beta = mk(bv.x, bv.y, bv.z);
                }
                if (path == debug_path_id(L)) {  // pt_set_debug_pixel (devicePrograms.cu:637-644)
                    const float4 l = shade0 ? l0 : W.L[path];
                    debug_record(L, b + 1, __float_as_int(S.isect[3 * h.tri].w), sf, beta, mk(l.x, l.y, l.z));
                }
                const bool conductor = rnd(seed) < sf.metallic;  // :400
                int li;
                const float P = pick_light(L, seed, li);
                if (P > 0.0f) {
                    const DevLight lt = L.lights[li];
                    const f3 ldir = light_vec(lt, sf.pos);
                    f3 lds = light_local(sf, lt);
                    // f has no RNG side effects in these modes: evaluate before the shadow test
                    f3 f = bsdf_f<MODE>(seed, sf.albedo, sf.roughness, conductor, sf.wo, lds);
                    f3 spectrum = nee_spectrum(f, lds);
                    if (!is_zero(spectrum)) {
                        contrib = nee_contrib(beta, spectrum, lt, light_dist2(lt, sf.pos), P);
                        // the lit table: the same add k_trace_pair would make for the unoccluded ray, at
                        // the same place in the path's bounce order
                        lit_answer = lit_side(lit_c, ldir, sf) && lit_bit(L, li, lit_c);
                        if (vis0 || lit_answer) {  // the visibility is already known (bounce 0: per pixel and light)
                            if (lit_answer || W.vis[vis0_index(L, path, li)]) {
                                const float4 l = shade0 ? l0 : W.L[path];
                                l0 = make_float4(l.x + contrib.x, l.y + contrib.y, l.z + contrib.z, 0.0f);
                                if (!shade0) W.L[path] = l0;
                            }
                        } else {
                            shadow_ray(sf.pos, sf.ng, ldir, so, sdir, stmax);
                            emit_shadow = true;
                            if (kOcc && occ && lit_side(lit_c, ldir, sf))
                                occ_t = occ_entry(L, li, lit_c);  // lands while the BSDF is sampled
                        }
                    }
                }
                BSample bs;
                // the last bounce's sampled direction is never traced (SamplePath :646)
                if (b + 1 < L.max_bounces &&
                    bsdf_sample<MODE>(seed, sf.albedo, sf.roughness, conductor, sf.wo, bs)) {
                    emit_next = continue_path(sf, bs, beta, o, d, b + 1, L.max_bounces);
                    if (!kBetaQ) stqs(W.beta + path, make_float4(beta.x, beta.y, beta.z, __uint_as_float(seed)));
                    if (kSkipCode<MODE> && skip) skip_w = skip_pick(skip_orient(skip2, sf), sf, skip_under<MODE>(bs), d);
                }
            }
        }
        if (shade0 && valid) W.L[path] = l0;  // every path of the batch, hit or miss
        if (lit) lit_count_wave(lit_answer, lds_lit);
        const int qi = block_append<kWaves>(cnt(W, b + 1, kQueue), emit_next, lds_q);
        if (lit) lit_count_block<kWaves>(L, lds_lit);
        if (emit_next) {
            stqs(no + qi, make_float4(o.x, o.y, o.z, __int_as_float(path)));
            stqs(nd + qi, make_float4(d.x, d.y, d.z, __uint_as_float(skip_w)));
            if (kBetaQ) stqs(queue_beta(W, b + 1) + qi, make_float4(beta.x, beta.y, beta.z, __uint_as_float(seed)));
        }
        if constexpr (kOcc) {
            // here and not where the ray is built: with the surface still live the test cost 19 spilled
            // VGPRs; one int (the entry, loaded there) carried across the extension-queue stores costs 2
            // (DESIGN.md §5 v61).
            // The origin is the one k_trace_pair will read: the continuation ray's where the record
            // shares it (below), else so.
            if (occ) {
                bool answered = false;
                if (occ_t >= 0) answered = occ_answers<TEX>(S, occ_t, (kShareOrigin && emit_next) ? o : so, sdir, stmax);
                if (answered) emit_shadow = false;  // occluded: no ray, nothing to add
                lit_count_wave(answered, lds_occ);
            }
        }
        const int si = block_append<kWaves>(cnt(W, b, kShadowQ), emit_shadow, lds_sh);
        if constexpr (kOcc) {
            if (occ) lit_count_block<kWaves, kCtrOccAnswers>(L, lds_occ);
        }
        if (emit_shadow) {
            // Lambert: a sampled direction is never below the surface (lambert_sample forces z >= 0),
            // so the continuation ray starts at the shadow ray's origin (continue_path's offset is
            // shadow_ray's, pt_shade.h): the shadow record names that ray (qi) instead of repeating origin
            // and path, and k_trace_pair reads them from the extension queue.  -1: own sh_o record.
            const bool share = kShareOrigin && emit_next;
            if (!share) stqs(W.sh_o + si, make_float4(so.x, so.y, so.z, __int_as_float(path)));
            stqs(W.sh_d + si, make_float4(sdir.x, sdir.y, sdir.z, stmax));
            stqs(W.sh_c + si, make_float4(contrib.x, contrib.y, contrib.z, __int_as_float(share ? qi : -1)));
        }
    }
}

// Bounce 0 of a fused-mode batch with the primary dedup and the (pixel, light) visibility table:
// the nf paths of a pixel start from the same hit (no pixel jitter, devicePrograms.cu:601-623),
// so one thread reconstructs the pixel's surface once and shades its paths in frame order (k_extend
// wrote one hit record per pixel).  Per path: the operations of k_shade_fused<SHADE0> (throughput
// 1, seed tea16(pixel, frame), radiance written, continuation appended to queue 1).
template <int MODE, bool TEX>
__global__ __launch_bounds__(shf_block(MODE), 1) void k_shade0_pixel(DevScene S, DevLaunch L, WFState W, int nf) {
    constexpr bool kBetaQ = MODE == kModeLambert;  // as k_shade_fused
    constexpr int kBlock = shf_block(MODE), kWaves = kBlock / 64;
    const int P1 = launch_pixels(L);
    __shared__ int lds_q[kWaves + 1];
    if (blockIdx.x == 0 && threadIdx.x == 0 && L.counters)
        atomicAdd(&L.counters[kCtrShadeItems], (unsigned long long)P1 * (unsigned long long)nf);
    if ((int)(blockIdx.x * kBlock) >= P1) return;  // block-uniform
    const int p = (int)(blockIdx.x * kBlock + threadIdx.x);
    const bool valid = p < P1 && !wf_cancelled(W);  // a cancelled wave still joins the appends
    int tri = -1;
    SurfaceHit sf;
    const bool skip = kSkipCode<MODE> && L.skip_tab;  // as k_shade_fused
    uint2 skip2 = make_uint2(0u, 0u);
    if (valid) {
        const float4 hv = W.hit[p];
        const Hit h = decode_hit(hv);
        tri = h.tri;
        if (tri >= 0) {
            if (skip) skip2 = skip_words(L, tri);
            const float4 c = W.ray_d[0][p];
            reconstruct<TEX>(S, h, mk(c.x, c.y, c.z), sf);
            skip2 = skip_orient(skip2, sf);
        }
    }
    const int dbg = debug_path_id(L);
    const int ipix = valid ? image_pixel(L, p) : 0;
    float4* no = W.ray_o[1];
    float4* nd = W.ray_d[1];
    for (int f = 0; f < nf; ++f) {  // uniform trip count (block_append below)
        const int path = f * P1 + p;
        bool emit_next = false;
        f3 o, d, beta = mk(1.0f, 1.0f, 1.0f);
        uint32_t seed = 0;
        float4 l0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool under = false;  // the continuation ray's origin is offset against sf.ng (skip_under)
        if (valid && tri >= 0) {
            seed = tea16((uint32_t)ipix, L.frame_base + (uint32_t)f);  // devicePrograms.cu:631
            if (path == dbg) debug_record(L, 1, __float_as_int(S.isect[3 * tri].w), sf, beta, mk(0.0f, 0.0f, 0.0f));
            const bool conductor = rnd(seed) < sf.metallic;  // :400
            int li;
            const float P = pick_light(L, seed, li);
            if (P > 0.0f) {
                const DevLight lt = L.lights[li];
                f3 lds = light_local(sf, lt);
                f3 fv = bsdf_f<MODE>(seed, sf.albedo, sf.roughness, conductor, sf.wo, lds);
                f3 spectrum = nee_spectrum(fv, lds);
                if (!is_zero(spectrum) && W.vis[vis0_index(L, path, li)]) {
                    f3 contrib = nee_contrib(beta, spectrum, lt, light_dist2(lt, sf.pos), P);
                    l0 = make_float4(0.0f + contrib.x, 0.0f + contrib.y, 0.0f + contrib.z, 0.0f);
                }
            }
            BSample bs;
            if (1 < L.max_bounces && bsdf_sample<MODE>(seed, sf.albedo, sf.roughness, conductor, sf.wo, bs)) {
                emit_next = continue_path(sf, bs, beta, o, d, 1, L.max_bounces);
                if (!kBetaQ) stqs(W.beta + path, make_float4(beta.x, beta.y, beta.z, __uint_as_float(seed)));
                if (kSkipCode<MODE> && skip) under = skip_under<MODE>(bs);
            }
        }
        if (valid) stqs(W.L + path, l0);  // every path of the batch, hit or miss
        const int qi = block_append<kWaves>(cnt(W, 1, kQueue), emit_next, lds_q);
        if (emit_next) {
            stqs(no + qi, make_float4(o.x, o.y, o.z, __int_as_float(path)));
            // the skip word is picked here, from the pixel's surface: one register less across the appends
            const uint32_t skip_w = (kSkipCode<MODE> && skip) ? skip_pick(skip2, sf, under, d) : 0u;
            stqs(nd + qi, make_float4(d.x, d.y, d.z, __uint_as_float(skip_w)));
            if (kBetaQ) stqs(queue_beta(W, 1) + qi, make_float4(beta.x, beta.y, beta.z, __uint_as_float(seed)));
        }
    }
}

// Fused modes: the shadow rays of bounce b and the extension rays of bounce b + 1 start at
// the same hit points and are independent, so one launch traces both queues (one SIMT tail
// and one launch instead of two).  Items [0, n_ext) are extension rays (closest hit ->
// hit records), items [n_ext, n_ext + n_sh) shadow rays (any hit -> deferred NEE add).
// SKIP (the launch's shading kernels store skip words, pt_skip.h): the fourth word of an extension
// ray's direction record is 0 or the child link the ray drops unvisited; shadow rays carry none.
template <bool STATS, bool TEX, int BLK = kBlockTrace, bool SKIP = false>
__global__ __launch_bounds__(BLK, wf_waves(TEX)) void k_trace_pair(DevScene S, WFState W, int b,
                                                                      unsigned long long* counters) {
    const int n_ext = *cnt(W, b + 1, kQueue);
    const int n_sh = *cnt(W, b, kShadowQ);
    const float4* ro = W.ray_o[(b + 1) & 1];
    const float4* rd = W.ray_d[(b + 1) & 1];
    TravStats ts;
    // the records of item i into the lane's state: an extension ray's origin | path and direction |
    // skip word, or a shadow ray's origin | path, direction | tmax and contribution.  st.inv holds the
    // three words init writes to the slot (pt_device.h hit_slot_carry) until init computes it: the
    // contribution, or the miss code of a closest-hit slot.
    auto load = [&](int i, TravRay& st) {
        if (i < n_ext) {
            load_ray(st, ldqs(ro + i), ldqs(rd + i));
            if (SKIP) st.skip = __float_as_int(st.best);
            st.best = 100.0f;
            st.inv = mk(0.0f, 0.0f, __int_as_float(kMissTri));
        } else {
            const int j = i - n_ext;
            const float4 c = ldqs(W.sh_d + j), k = ldqs(W.sh_c + j);
            // origin | path: the shadow ray's own record, or (Lambert) the continuation ray of the
            // same path, which starts at the same point (k_shade_fused)
            const int q = __float_as_int(k.w);
            load_ray(st, ldqs(q >= 0 ? ro + q : W.sh_o + j), c);
            st.inv = mk(k.x, k.y, k.z);
        }
    };
    auto init = [&](int i, TravRay& st, TriBatchLds* slot) {
        const bool any = i >= n_ext;
        const int skip_w = SKIP ? st.skip : 0;
        // a shadow ray's slot carries its contribution to commit(); a hit may overwrite it, and an
        // occluded ray adds nothing
        hit_slot_init(slot, st.best, any);
        hit_slot_carry(slot, st.inv.x, st.inv.y, st.inv.z);
        trav_init(st, st.o, st.d, 0.0f, st.best);
        st.any = any;
        if (SKIP) {
            const bool skips = !any && skip_w != 0;
            st.skip = skips ? skip_w : kEmptyChild;
            if (STATS) ts.skips += skips;
        }
    };
    // the deferred NEE add as load (finish, before the refill's record loads) + store (commit,
    // after them): the lane does not wait for the radiance line before the refill
    struct NeeAdd {
        float4* p;
        float4 v;
    };
    auto finish = [&](int i, const TravRay& st, const TriBatchLds* slot) -> NeeAdd {
        NeeAdd a{nullptr, make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
        // the hit-record stores first: a store issued after the radiance load would wait for it
        if (i < n_ext) stqs(W.hit + i, hit_record(slot, st.path));
        __builtin_amdgcn_sched_barrier(0);
        const bool unocc = i >= n_ext && !hit_slot_occluded(slot);
        if (STATS && unocc) ts.unocc++;
        if (unocc) {  // add the deferred NEE contribution
            a.p = W.L + st.path;
            a.v = *a.p;
        }
        return a;
    };
    auto commit = [&](const NeeAdd& a, const TriBatchLds* slot) {
        if (a.p) {
            float x, y, z;
            hit_slot_words(slot, x, y, z);
            *a.p = make_float4(a.v.x + x, a.v.y + y, a.v.z + z, 0.0f);
        }
    };
    // The queue is [extension rays | shadow rays] in contiguous wave slices, so all but one wave
    // trace a single ray kind; a mixed-kind loop serves both (per-kind loops in one kernel and
    // per-wave shares of both kinds were slower).
    int first, end;
    const int n_all = n_ext + n_sh;
    RayPool pool;
    if (PT_TRACE_POOL > 0 && pool_pays(n_all)) {
        pool.ctr = cnt(W, b, kPool);
        pool.end = n_all;
        pool.begin = n_all - (int)((long long)n_all * PT_TRACE_POOL / 100);
    } else {
        pool.begin = pool.end = n_all;
    }
    wave_slice(pool.begin, first, end);
    trace_queue<SKIP ? kRayMixedSkip : kRayMixed, STATS, TEX, BLK>(S, first, end, ts, W, load, init, finish, commit, pool);
    if (blockIdx.x == 0 && threadIdx.x == 0 && counters) {
        atomicAdd(&counters[kCtrSegments], (unsigned long long)n_ext);
        atomicAdd(&counters[kCtrShadowRays], (unsigned long long)n_sh);
        atomicAdd(&counters[kCtrTraceRays], (unsigned long long)(n_ext + n_sh));
        atomicAdd(&counters[kCtrTraceBytes], 48ull * (unsigned long long)(n_ext + n_sh));  // their queue bytes
        atomicAdd(&counters[kCtrPairRays], (unsigned long long)(n_ext + n_sh));
        atomicAdd(&counters[kCtrPairBytes], 48ull * (unsigned long long)(n_ext + n_sh));
        atomicAdd(&counters[kCtrPairShadowRays], (unsigned long long)n_sh);
    }
    flush_trav_stats<STATS>(counters, ts);
}

// First half of a Default / Layered bounce: surface, metallic coin and light pick (the draws
// GlossyDiffuse::f must follow, devicePrograms.cu:400-445), then the item is queued for the
// later phases, by bucket (shade_bucket): the BSDF-sample queue for every hit that continues,
// and either a shadow ray (visibility still unknown; the ray carries item | bucket << 28) or,
// at bounce 0 with the (pixel, light) visibility table, the NEE queue directly.
template <int MODE, bool TEX>
__global__ __launch_bounds__(kBlockShA) void k_shade_a(DevScene S, DevLaunch L, WFState W, int b, int vis0) {
    const int n = *cnt(W, b, kQueue);
    const float4* rd = W.ray_d[b & 1];
    __shared__ int lds_sh[kWavesShA + 1];
    __shared__ int lds_nee[kNeeBuckets * (kWavesShA + 1)], lds_smp[kShadeBuckets * (kWavesShA + 1)];
    __shared__ int lds_lit[kWavesShA], lds_occ[kWavesShA];
    const bool lit = !vis0 && L.lit_tri;  // as k_shade_fused
    const bool occ = lit && L.occ_tab;    // the occluder candidates (occ_answers)
    if ((int)(blockIdx.x * kBlockShA) >= n) return;  // block-uniform
    const int i = (int)(blockIdx.x * kBlockShA + threadIdx.x);
    bool emit = false, lit_answer = false, occ_answer = false;
    int nee_bucket = -1, smp_bucket = -1, code = 0;
    f3 so, sdir;
    float stmax = 0.0f;
    if (i < n && !wf_cancelled(W)) {  // a cancelled wave still joins the appends
        const float4 hv = W.hit[i];
        const float4 c = rd[i];  // beside the hit record (as k_shade_fused)
        const int path = __float_as_int(hv.x);
        const Hit h = decode_hit(hv);
        if (h.tri >= 0) {
            const int lit_c = lit ? lit_cell(L, h) : -1;
            SurfaceHit sf;
            reconstruct<TEX>(S, h, mk(c.x, c.y, c.z), sf);
            float4 bv = W.beta[path];
            uint32_t seed = __float_as_uint(bv.w);
            if (path == debug_path_id(L)) {  // pt_set_debug_pixel (devicePrograms.cu:637-644)
                const float4 l = W.L[path];
                debug_record(L, b + 1, __float_as_int(S.isect[3 * h.tri].w), sf, mk(bv.x, bv.y, bv.z),
                             mk(l.x, l.y, l.z));
            }
            const bool conductor = rnd(seed) < sf.metallic;
            int li;
            const float P = pick_light(L, seed, li);
            W.beta[path] = make_float4(bv.x, bv.y, bv.z, __uint_as_float(seed));
            W.aux[path] = (li << 1) | (conductor ? 1 : 0);
            const int bk = shade_bucket<MODE>(conductor, sf.roughness);
            // the last bounce's sampled direction is never traced (SamplePath :646): no sample item
            if (b + 1 < L.max_bounces) smp_bucket = bk;
            if (P > 0.0f) {
                const DevLight lt = L.lights[li];
                const f3 ldir = light_vec(lt, sf.pos);
                const f3 lds = light_local(sf, lt);  // ahead of the branches that use its normalize
                int nb = 0;  // conductor
                if (MODE == kModeLayered || !conductor)
                    nb = !same_hemisphere(sf.wo, lds) ? kNeeCross : nee_layered_bucket(bk, sf.albedo);
                // the lit table: known unoccluded, straight to the NEE queue like the bounce-0 table
                lit_answer = lit_side(lit_c, ldir, sf) && lit_bit(L, li, lit_c);
                if (vis0 || lit_answer) {
                    if (lit_answer || W.vis[vis0_index(L, path, li)]) nee_bucket = nb;
                } else {
                    shadow_ray(sf.pos, sf.ng, ldir, so, sdir, stmax);
                    code = i | (nb << kItemBits);
                    emit = true;
                    // an occluded item gets neither a shadow ray nor a NEE-queue entry
                    if (occ && lit_side(lit_c, ldir, sf))
                        occ_answer = occ_answers<TEX>(S, occ_entry(L, li, lit_c), so, sdir, stmax);
                    if (occ_answer) emit = false;
                }
            }
        }
    }
    if (lit) lit_count_wave(lit_answer, lds_lit);
    if (occ) lit_count_wave(occ_answer, lds_occ);
    const int si = block_append<kWavesShA>(cnt(W, b, kShadowQ), emit, lds_sh);
    if (lit) lit_count_block<kWavesShA>(L, lds_lit);
    if (occ) lit_count_block<kWavesShA, kCtrOccAnswers>(L, lds_occ);
    if (emit) {
        W.sh_o[si] = make_float4(so.x, so.y, so.z, __int_as_float(code));
        W.sh_d[si] = make_float4(sdir.x, sdir.y, sdir.z, stmax);
    }
    const int ni = block_append_k<kWavesShA, kNeeBuckets>(cnt(W, b, kNee0), nee_bucket, lds_nee);
    if (nee_bucket >= 0) W.nq[nee_index(W, nee_bucket, ni)] = i;
    const int mi = block_append_k<kWavesShA, kShadeBuckets>(cnt(W, b, kSmp0), smp_bucket, lds_smp);
    if (smp_bucket >= 0) W.sq[smp_index(W, smp_bucket, mi)] = i;
}

// Any-hit visibility of the shadow queue of bounce b.  table = 1: the bounce-0 (pixel, light)
// table (k_shadow0_setup), vis[j] = 1 if unoccluded; table = 0: vis[j] = the ray's item code
// if unoccluded, else -1 (k_nee_compact reads it).
template <bool TEX, int BLK = kBlockTrace>
__global__ __launch_bounds__(BLK, wf_waves(false)) void k_shadow_vis(DevScene S, WFState W, int b, int table,
                                                                      unsigned long long* counters) {
    const int n = *cnt(W, b, kShadowQ);
    if (blockIdx.x == 0 && threadIdx.x == 0 && counters) atomicAdd(&counters[kCtrShadowRays], (unsigned long long)n);
    TravStats ts;
    trace_slice<kRayAny, false, TEX, BLK>(
        S, n, ts, W,
        [&](int j, TravRay& st) { load_ray(st, W.sh_o[j], W.sh_d[j]); },
        [&](int j, TravRay& st, TriBatchLds* slot) {
            trav_init(st, st.o, st.d, 0.0f, st.best);
            hit_slot_init_any(slot, st.best);
        },
        [&](int j, const TravRay& st, const TriBatchLds* slot) {
            const bool occluded = hit_slot_occluded(slot);
            W.vis[j] = table ? (occluded ? 0 : 1) : (occluded ? -1 : st.path);
        }, cnt(W, b, kPoolSh));
}

// Visible shadow rays of bounce b -> the NEE bucket queues (vis[j] = item | bucket << 28, or -1).
// kCompactPer consecutive entries per thread, so a block appends 8192 entries with one atomic
// per bucket.
constexpr int kCompactPer = 8;
__global__ __launch_bounds__(kBlockSh) void k_nee_compact(WFState W, int b) {
    const int n = *cnt(W, b, kShadowQ);
    const int base = (int)(blockIdx.x * kBlockSh * kCompactPer);
    if (base >= n) return;  // block-uniform
    __shared__ int lds[kNeeBuckets * (kWavesSh + 1)];
    const int j0 = base + (int)threadIdx.x * kCompactPer;
    const bool cx = wf_cancelled(W);  // a cancelled wave compacts nothing but joins the barriers
    int v[kCompactPer];
    int c[kNeeBuckets] = {};
#pragma unroll
    for (int k = 0; k < kCompactPer; ++k) {
        v[k] = j0 + k < n && !cx ? W.vis[j0 + k] : -1;
#pragma unroll
        for (int q = 0; q < kNeeBuckets; ++q) c[q] += (v[k] >= 0 && (v[k] >> kItemBits) == q) ? 1 : 0;
    }
    // block-exclusive prefix of every bucket's count: wave scan, then the wave totals in LDS
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int incl[kNeeBuckets];
#pragma unroll
    for (int q = 0; q < kNeeBuckets; ++q) {
        int x = c[q];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        incl[q] = x;
        if (lane == 63) lds[q * kWavesSh + wave] = x;
    }
    __syncthreads();
    if ((int)threadIdx.x < kNeeBuckets) {
        const int q = threadIdx.x;
        int tot = 0;
        for (int w = 0; w < kWavesSh; ++w) {
            const int t = lds[q * kWavesSh + w];
            lds[q * kWavesSh + w] = tot;
            tot += t;
        }
        lds[kNeeBuckets * kWavesSh + q] = tot > 0 ? atomicAdd(cnt(W, b, kNee0 + q), tot) : 0;
    }
    __syncthreads();
    int off[kNeeBuckets];
#pragma unroll
    for (int q = 0; q < kNeeBuckets; ++q)
        off[q] = lds[kNeeBuckets * kWavesSh + q] + lds[q * kWavesSh + wave] + incl[q] - c[q];
#pragma unroll
    for (int k = 0; k < kCompactPer; ++k) {
        if (v[k] < 0) continue;
        const int q = v[k] >> kItemBits;
        int slot = off[0];
#pragma unroll
        for (int r = 1; r < kNeeBuckets; ++r) slot = q == r ? off[r] : slot;
#pragma unroll
        for (int r = 0; r < kNeeBuckets; ++r) off[r] += q == r ? 1 : 0;
        W.nq[nee_index(W, q, slot)] = v[k] & ((1 << kItemBits) - 1);
    }
}

// Entry idx of the NEE / sample queue (bucket q: slots nee_index / smp_index, length
// *cnt(W, b, c0 + q)), or -1 past the total.  Buckets are taken in order, so all but a few waves
// hold one bucket.
__device__ __forceinline__ int nee_entry(const WFState& W, int b, int idx) {
    int base = 0;
#pragma unroll
    for (int q = 0; q < kNeeBuckets; ++q) {
        const int n = *cnt(W, b, kNee0 + q);
        if (idx < base + n) return W.nq[nee_index(W, q, idx - base)];
        base += n;
    }
    return -1;
}
__device__ __forceinline__ int smp_entry(const WFState& W, int b, int idx) {
    int base = 0;
#pragma unroll
    for (int q = 0; q < kShadeBuckets; ++q) {
        const int n = *cnt(W, b, kSmp0 + q);
        if (idx < base + n) return W.sq[smp_index(W, q, idx - base)];
        base += n;
    }
    return -1;
}
__device__ __forceinline__ int smp_total(const WFState& W, int b) {
    int n = 0;
#pragma unroll
    for (int q = 0; q < kShadeBuckets; ++q) n += *cnt(W, b, kSmp0 + q);
    return n;
}
__device__ __forceinline__ int nee_total(const WFState& W, int b) {
    int n = 0;
#pragma unroll
    for (int q = 0; q < kNeeBuckets; ++q) n += *cnt(W, b, kNee0 + q);
    return n;
}

// NEE of a Default / Layered bounce over the items whose light is visible (devicePrograms.cu:
// 446-472).  The stochastic GlossyDiffuse eval dominates (≈10^4 instructions per call, DESIGN.md
// §5) and a wave pays for its slowest lane: the items come from the bucketed NEE queue, so every
// wave but the last of each bucket is full and runs one BSDF code path.  Every path sees the
// same operations and random numbers in the same order (the eval writes the advanced seed back
// to W.beta before k_shade_smp reads it).
template <int MODE, bool TEX>
__global__ __launch_bounds__(kBlockShB, PT_SHB_WAVES) void k_shade_nee(DevScene S, DevLaunch L, WFState W, int b) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && L.counters)
        atomicAdd(&L.counters[kCtrShadeItems], (unsigned long long)nee_total(W, b));
    if ((int)(blockIdx.x * kBlockShB) >= nee_total(W, b)) return;  // block-uniform
    if (wf_cancelled(W)) return;  // no barrier below
    const int j = nee_entry(W, b, (int)(blockIdx.x * kBlockShB + threadIdx.x));
    if (j < 0) return;
    const float4 hv = W.hit[j], c = W.ray_d[b & 1][j];
    const int path = __float_as_int(hv.x);
    const Hit h = decode_hit(hv);
    SurfaceHit sf;
    reconstruct<TEX>(S, h, mk(c.x, c.y, c.z), sf);
    // only the path, the light index, |cos| and the squared distance stay live across the layered
    // walk; the throughput and the light are loaded again after it (the same values and
    // operations as loading them before it, so the same bits)
    const int aux = W.aux[path];
    const int li = aux >> 1;
    uint32_t seed = __float_as_uint(W.beta[path].w);
    f3 lds;
    float d2;
    {
        const DevLight lt = L.lights[li];
        lds = light_local(sf, lt);
        d2 = light_dist2(lt, sf.pos);
    }
    const float cosl = abs_dot(lds, mk(0.0f, 0.0f, 1.0f));  // nee_spectrum's factor, taken before the walk
    f3 f = bsdf_f<MODE, true>(seed, sf.albedo, sf.roughness, aux & 1, sf.wo, lds);
    f3 spectrum = f * cosl;
    const float4 bv = W.beta[path];
    const f3 beta = mk(bv.x, bv.y, bv.z);
    if (!is_zero(spectrum)) {
        const f3 add = nee_contrib(beta, spectrum, L.lights[li], d2, light_pdf(L));
        float4 l = W.L[path];
        W.L[path] = make_float4(l.x + add.x, l.y + add.y, l.z + add.z, 0.0f);
    }
    W.beta[path] = make_float4(bv.x, bv.y, bv.z, __uint_as_float(seed));  // f may draw
}

// BSDF sample + continuation of a Default / Layered bounce (devicePrograms.cu:474-509) over the
// bucketed sample queue; continuation rays are appended to queue b + 1.
template <int MODE, bool TEX>
__global__ __launch_bounds__(kBlockShB, PT_SMP_WAVES) void k_shade_smp(DevScene S, DevLaunch L, WFState W, int b) {
    constexpr int kW = kBlockShB / 64;
    __shared__ int lds_q[kW + 1];
    if ((int)(blockIdx.x * kBlockShB) >= smp_total(W, b)) return;  // block-uniform
    const int j = smp_entry(W, b, (int)(blockIdx.x * kBlockShB + threadIdx.x));
    bool emit_next = false;
    f3 o, d;
    int path = 0;
    if (j >= 0 && !wf_cancelled(W)) {  // a cancelled wave still joins the appends
        const float4 hv = W.hit[j], c = W.ray_d[b & 1][j];
        path = __float_as_int(hv.x);
        const Hit h = decode_hit(hv);
        d = mk(c.x, c.y, c.z);
        SurfaceHit sf;
        reconstruct<TEX>(S, h, d, sf);
        const float4 bv = W.beta[path];
        uint32_t seed = __float_as_uint(bv.w);
        f3 beta = mk(bv.x, bv.y, bv.z);
        BSample bs;
        if (bsdf_sample<MODE, true>(seed, sf.albedo, sf.roughness, W.aux[path] & 1, sf.wo, bs)) {
            emit_next = continue_path(sf, bs, beta, o, d, b + 1, L.max_bounces);
            W.beta[path] = make_float4(beta.x, beta.y, beta.z, __uint_as_float(seed));
        }
    }
    float4* no = W.ray_o[(b + 1) & 1];
    float4* nd = W.ray_d[(b + 1) & 1];
    const int qi = block_append<kW>(cnt(W, b + 1, kQueue), emit_next, lds_q);
    if (emit_next) {
        no[qi] = make_float4(o.x, o.y, o.z, __int_as_float(path));
        nd[qi] = make_float4(d.x, d.y, d.z, 0.0f);
    }
}

inline bool fused_mode(int mode) { return mode == kModeLambert || mode == kModeConductor || mode == kModeDielectric; }

// Grid covering `items` slots, one per thread.
inline dim3 item_grid(int items, int block) { return dim3((unsigned)std::max(1, (items + block - 1) / block)); }

// Exactly the blocks that are resident at once (occupancy query, cached) — the lane-
// refilling trace kernels, whose waves each own a static queue slice.
template <typename K>
dim3 occupancy_grid(K kernel, int cus, int block = kBlockTrace) {
    static std::unordered_map<const void*, int> cache;
    const void* key = reinterpret_cast<const void*>(kernel);
    auto it = cache.find(key);
    int per_cu = 0;
    if (it == cache.end()) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || per_cu < 1)
            per_cu = 1;
        cache[key] = per_cu;
    } else {
        per_cu = it->second;
    }
    // (2x / 4x oversubscribed trace grids with the two wavefront streams: Lambert +0.2 / +0.5 %,
    // Dielectric +1.7 / +1.4 %, Layered -0.4 %: noise-level, not kept)
    return dim3((unsigned)(per_cu * std::max(1, cus)));
}

// The variant of a trace kernel for a launch: f(tex, stats, block) with std::bool_constant TEX and
// STATS and std::integral_constant<int> kBlockTraceWide or kBlockTrace.
template <class F>
hipError_t trace_variant(bool tex, bool wide, bool stats, F f) {
    return with_flag(tex, [&](auto tx) {
        return with_flag(wide, [&](auto wd) {
            return with_flag(stats, [&](auto st) {
                return f(tx, st, std::integral_constant<int, wd() ? kBlockTraceWide : kBlockTrace>{});
            });
        });
    });
}

// phase (Default / Layered): 0 = k_shade_a, 1 = k_shade_nee, 2 = k_shade_smp
template <int MODE, bool TEX>
hipError_t launch_shade_t(bool fused, const DevScene& S, const DevLaunch& L, const WFState& W, int b, int items,
                          hipStream_t stream, int phase, int vis0, int shade0) {
    if (fused) {
        if constexpr (MODE == kModeLambert || MODE == kModeConductor || MODE == kModeDielectric)
            with_flag(shade0 != 0, [&](auto s0) {
                hipLaunchKernelGGL((k_shade_fused<MODE, TEX, s0()>), item_grid(items, shf_block(MODE)), dim3(shf_block(MODE)), 0,
                                   stream, S, L, W, b, vis0);
            });
    } else if (phase == 0) {
        hipLaunchKernelGGL((k_shade_a<MODE, TEX>), item_grid(items, kBlockShA), dim3(kBlockShA), 0, stream, S, L, W, b,
                           vis0);
    } else if (phase == 1) {
        hipLaunchKernelGGL((k_shade_nee<MODE, TEX>), item_grid(items, kBlockShB), dim3(kBlockShB), 0, stream, S, L,
                           W, b);
    } else {
        hipLaunchKernelGGL((k_shade_smp<MODE, TEX>), item_grid(items, kBlockShB), dim3(kBlockShB), 0, stream, S, L,
                           W, b);
    }
    return hipGetLastError();
}

template <int MODE>
hipError_t launch_shade(bool fused, const DevScene& S, const DevLaunch& L, const WFState& W, int b, int items,
                        hipStream_t stream, int phase, int vis0, int shade0) {
    return with_flag(S.texinfo != nullptr, [&](auto tx) {
        return launch_shade_t<MODE, tx()>(fused, S, L, W, b, items, stream, phase, vis0, shade0);
    });
}

template <int MODE>
hipError_t launch_shade0_pixel_t(const DevScene& S, const DevLaunch& L, const WFState& W, int nf, hipStream_t stream) {
    constexpr int block = shf_block(MODE);
    const dim3 grid = item_grid(L.n_pixels, block);
    with_flag(S.texinfo != nullptr, [&](auto tx) {
        hipLaunchKernelGGL((k_shade0_pixel<MODE, tx()>), grid, dim3(block), 0, stream, S, L, W, nf);
    });
    return hipGetLastError();
}
hipError_t launch_shade0_pixel(int mode, const DevScene& S, const DevLaunch& L, const WFState& W, int nf,
                               hipStream_t stream) {
    switch (mode) {
        case kModeLambert: return launch_shade0_pixel_t<kModeLambert>(S, L, W, nf, stream);
        case kModeConductor: return launch_shade0_pixel_t<kModeConductor>(S, L, W, nf, stream);
        default: return launch_shade0_pixel_t<kModeDielectric>(S, L, W, nf, stream);
    }
}

// vis0: n_lights when the bounce-0 (pixel, light) visibility table is used at this bounce, else 0
hipError_t launch_shade_mode(int mode, bool fused, const DevScene& S, const DevLaunch& L, const WFState& W, int b,
                             int items, hipStream_t stream, int phase, int vis0, int shade0 = 0) {
    switch (mode) {
        case kModeLambert: return launch_shade<kModeLambert>(fused, S, L, W, b, items, stream, phase, vis0, shade0);
        case kModeConductor: return launch_shade<kModeConductor>(fused, S, L, W, b, items, stream, phase, vis0, shade0);
        case kModeDielectric: return launch_shade<kModeDielectric>(fused, S, L, W, b, items, stream, phase, vis0, shade0);
        case kModeLayered: return launch_shade<kModeLayered>(fused, S, L, W, b, items, stream, phase, vis0, shade0);
        default: return launch_shade<kModeDefault>(fused, S, L, W, b, items, stream, phase, vis0, shade0);
    }
}

}  // namespace

namespace {

// The queue set's arrays: where each lives in WFState, its element size and its elements per path
// (0: `count`, which count_bytes(max_bounces) sizes).
struct QueueArray {
    void** (*slot)(WFState&);
    size_t elem, per_path;
    size_t bytes(size_t paths, int max_bounces) const {
        return per_path ? paths * per_path * elem : count_bytes(max_bounces);
    }
};
#define PT_QUEUE(member, per_path) \
    QueueArray { [](WFState& W) { return (void**)&W.member; }, sizeof(*WFState().member), per_path }
const QueueArray kQueueArrays[] = {
    PT_QUEUE(ray_o[0], 1), PT_QUEUE(ray_o[1], 1), PT_QUEUE(ray_d[0], 1), PT_QUEUE(ray_d[1], 1),
    PT_QUEUE(hit, 1),      PT_QUEUE(beta, 1),     PT_QUEUE(beta_q, 1),   PT_QUEUE(L, 1),
    PT_QUEUE(sh_o, 1),     PT_QUEUE(sh_d, 1),     PT_QUEUE(sh_c, 1),     PT_QUEUE(aux, 1),
    PT_QUEUE(vis, 1),      PT_QUEUE(nq, kNeeRegions), PT_QUEUE(sq, kShadeBuckets), PT_QUEUE(count, 0)};
#undef PT_QUEUE

}  // namespace

size_t wavefront_bytes(int paths, int max_bounces) {
    size_t b = 0;
    for (const QueueArray& a : kQueueArrays) b += a.bytes((size_t)paths, max_bounces);
    return b;
}

hipError_t WFQueues::alloc(int paths, int max_bounces) {
    release();
    for (const QueueArray& a : kQueueArrays) {
        const size_t bytes = a.bytes((size_t)paths, max_bounces);
        const hipError_t e = hipMalloc(a.slot(w_), bytes > 0 ? bytes : 16);
        if (e != hipSuccess) {
            *a.slot(w_) = nullptr;
            release();
            (void)hipGetLastError();
            return e;
        }
    }
    w_.paths = paths;
    w_.max_bounces = max_bounces;
    return hipSuccess;
}

void WFQueues::release() {
    for (const QueueArray& a : kQueueArrays)
        if (*a.slot(w_)) (void)hipFree(*a.slot(w_));
    w_ = WFState{};
}

hipError_t launch_wavefront_batch(const DevScene& S, const DevLaunch& L, const WFState& W, const WFBatch& B) {
    const int mode = B.mode, cus = B.cus;
    const bool stats = B.stats, primary_dedup = B.primary_dedup, wide_trace = B.wide_trace;
    const hipStream_t stream = B.stream;
    const int nf = (int)L.n_frames;  // the batch's frames: L.frame_base .. L.frame_base + nf - 1
    const int P = L.n_pixels * nf;  // paths in flight
    const int maxb = L.max_bounces;
    hipError_t e = hipSuccess;
    if (W.cancel_seen && W.hold_release) {  // pt_set_debug_hold: the batch waits in k_hold first
        hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, stream, W);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    e = hipMemsetAsync(W.count, 0, count_bytes(maxb), stream);
    if (e != hipSuccess) return e;
    // fused modes with the primary dedup: frame 0's camera rays only (k_camera `lean`, shade0)
    const bool lean = fused_mode(mode) && primary_dedup && nf > 1 && maxb > 0;
    hipLaunchKernelGGL(k_camera, item_grid(lean ? L.n_pixels : P, kBlockWF), dim3(kBlockWF), 0, stream, W, L,
                       L.frame_base, nf, lean ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const bool fused = fused_mode(mode);
    const bool tex = S.texinfo != nullptr;  // textured scene: kernels with texture sampling
    // pt_set_kernel_timing: the launch between an event pair of `pool` (null: not timed).  Timed are
    // the k_extend and k_trace_pair launches and the dominant shading kernel of a bounce: k_shade_fused
    // / k_shade0_pixel (fused modes), k_shade_nee (Default / Layered: the stochastic layered eval,
    // 53-60 % of their frame)
    auto timed = [&](EventPool* pool, auto launch) -> hipError_t {
        if (!pool) return launch();
        hipEvent_t a = nullptr, b = nullptr;
        hipError_t r;
        if ((r = pool->next(&a, &b)) != hipSuccess || (r = hipEventRecord(a, stream)) != hipSuccess) return r;
        if ((r = launch()) != hipSuccess) return r;
        return hipEventRecord(b, stream);
    };
    // a trace kernel on exactly the workgroups that are resident at once; wide_trace: the trace
    // kernels of a one-stream call take the wide workgroups (kBlockTraceWide)
    auto trace_launch = [&](auto kernel, int block, auto... args) -> hipError_t {
        hipLaunchKernelGGL(kernel, occupancy_grid(kernel, cus, block), dim3(block), 0, stream, args...);
        return hipGetLastError();
    };
    auto extend = [&](int b, int dup, int copies) -> hipError_t {
        return timed(B.timers.extend, [&] {
            return trace_variant(tex, wide_trace, stats, [&](auto tx, auto st, auto blk) {
                return trace_launch(k_extend<st(), tx(), blk()>, blk(), S, W, b, dup, copies, L.counters);
            });
        });
    };
    auto pair = [&](int b) -> hipError_t {
        return timed(B.timers.pair, [&] {
            return trace_variant(tex, wide_trace, stats, [&](auto tx, auto st, auto blk) {
                return with_flag(L.skip_tab != nullptr, [&](auto sk) {
                    return trace_launch(k_trace_pair<st(), tx(), blk(), sk()>, blk(), S, W, b, L.counters);
                });
            });
        });
    };
    auto shadow_vis = [&](int b, int table) -> hipError_t {  // k_shadow_vis has no STATS variant
        const hipError_t r = trace_variant(tex, wide_trace, false, [&](auto tx, auto, auto blk) {
            return trace_launch(k_shadow_vis<tx(), blk()>, blk(), S, W, b, table, L.counters);
        });
        if (r != hipSuccess) return r;
        if (!table) hipLaunchKernelGGL(k_nee_compact, item_grid(P, kBlockSh * kCompactPer), dim3(kBlockSh), 0, stream, W, b);
        return hipGetLastError();
    };
    // bounce-0 shadow dedup: one shadow ray per (pixel, light) instead of one per path; pays
    // off while the batch has at least as many frames as there are lights
    const int P1 = L.n_pixels;
    const int vis0 = (primary_dedup && nf > 1 && L.n_lights >= 1 && L.n_lights <= nf) ? L.n_lights : 0;
    auto shadow0 = [&]() -> hipError_t {
        if (!vis0) return hipSuccess;
        hipError_t r = with_flag(tex, [&](auto tx) {
            hipLaunchKernelGGL(k_shadow0_setup<tx()>, item_grid(P1 * vis0, kBlockWF), dim3(kBlockWF), 0, stream, S, L, W);
            return hipGetLastError();
        });
        if (r != hipSuccess || (r = shadow_vis(0, 1)) != hipSuccess) return r;
        // the table's rays must not be traced again as bounce-0 shadow rays
        return hipMemsetAsync(W.count + kShadowQ * kCntStride, 0, sizeof(int), stream);
    };
    if (maxb <= 0) {
        // SamplePath's loop never runs (devicePrograms.cu:646): black frames, no segments
    } else if (fused) {
        // extend(0); then per bounce: shade(b) -> [shadow rays of b + extension rays of b+1]
        // lean bounce 0 with the visibility table: one hit record and one surface per pixel
        const bool pixel0 = lean && vis0;
        if ((e = extend(0, primary_dedup ? nf : 1, pixel0 ? 1 : (primary_dedup ? nf : 1))) != hipSuccess) return e;
        if ((e = shadow0()) != hipSuccess) return e;
        for (int b = 0; b < maxb; ++b) {
            if (b == 0 && pixel0) {
                if ((e = timed(B.timers.shade, [&] { return launch_shade0_pixel(mode, S, L, W, nf, stream); })) != hipSuccess)
                    return e;
            } else if ((e = timed(B.timers.shade, [&] {
                            return launch_shade_mode(mode, true, S, L, W, b, P, stream, 0, b == 0 ? vis0 : 0,
                                                     b == 0 && lean);
                        })) != hipSuccess) {
                return e;
            }
            if ((e = pair(b)) != hipSuccess) return e;
        }
    } else {
        for (int b = 0; b < maxb; ++b) {
            const int dup = b == 0 && primary_dedup ? nf : 1;
            if ((e = extend(b, dup, dup)) != hipSuccess) return e;
            const int v0 = b == 0 ? vis0 : 0;
            if (v0 && (e = shadow0()) != hipSuccess) return e;
            // k_shade_a queues the bounce's items by bucket; the visible ones (the bounce-0 table,
            // or k_shadow_vis + k_nee_compact) get the NEE eval, the continuing ones the sample
            if ((e = launch_shade_mode(mode, false, S, L, W, b, P, stream, 0, v0)) != hipSuccess) return e;
            if (!v0 && (e = shadow_vis(b, 0)) != hipSuccess) return e;
            if ((e = timed(B.timers.shade, [&] { return launch_shade_mode(mode, false, S, L, W, b, P, stream, 1, v0); })) !=
                hipSuccess)
                return e;
            if (b + 1 < maxb && (e = launch_shade_mode(mode, false, S, L, W, b, P, stream, 2, v0)) != hipSuccess)
                return e;
        }
    }
    if (B.accum_wait && (e = hipStreamWaitEvent(stream, B.accum_wait, 0)) != hipSuccess) return e;
    if ((e = accum_batch(W.L, L, nf, stream)) != hipSuccess) return e;
    if (B.accum_done && (e = hipEventRecord(B.accum_done, stream)) != hipSuccess) return e;
    return hipGetLastError();
}

}  // namespace pt
