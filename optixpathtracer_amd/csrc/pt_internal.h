// pt_internal.h — host-side declarations shared by the C-ABI driver (pt_capi*.cpp, pt_renderer.h) and
// the kernel translation units (pt_build.hip, pt_render.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "pt_device.h"

namespace pt {

// A run-time flag as a compile-time constant for a launcher: f(std::true_type{}) or
// f(std::false_type{}), so a kernel's bool template arguments are written flag() in one launch.
template <class F>
auto with_flag(bool v, F f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}

// Scene triangle soup in ORIGINAL order (meshes concatenated), world space.
struct BuildInput {
    const float4* tri_orig;  // 3 per triangle: v0|orig idx bits, v1|material bits, v2|0
    const float4* nrm_orig;  // 3 per triangle
    const float4* uv_orig;   // 2 per triangle (uv0, uv1 | uv2, 0) or NULL (no textures)
    int n;
    float cmin[3], cmax[3];  // centroid bounds (Morton quantisation range)
    int builder;             // kBuilder*: the front end that makes the binary tree (pt_create's default
                             // is kBuilderSAHGPU); any other value builds with PLOC
    const float4* tri_host;  // the same triangles on the host (kBuilderSAH builds there)
};
constexpr int kBuilderPLOC = 0;
constexpr int kBuilderLBVH = 1;
constexpr int kBuilderSAH = 2;     // host binned SAH (pt_sah.cpp)
constexpr int kBuilderSAHGPU = 3;  // the same tree built on the GPU (pt_sah_gpu.hip)

// Host binned-SAH binary tree (pt_sah.cpp) in the GPU builders' layout: order = original triangle
// per DFS leaf, child codes (>= 0 internal, ~k DFS leaf k), leaf ranges and plain boxes; root 0.
void sah_binary_tree(const float4* tri, int n, std::vector<uint32_t>& order, std::vector<int2>& child,
                     std::vector<int2>& range, std::vector<float4>& box);
// The same binary tree built on the GPU (pt_sah_gpu.hip): order, child, range and box are device
// arrays of n, n - 1, n - 1 and 2 (n - 1) entries; identical to sah_binary_tree's up to the
// internal node numbering (root 0).  Synchronises `stream`.
hipError_t sah_build_gpu(const float4* tri, int n, uint32_t* order, int2* child, int2* range, float4* box,
                         hipStream_t stream);
// Insertion-based optimisation of that tree in place (pt_sah.cpp); returns the relative cost cut.
// PT_SAH_REINSERT = the most rounds kBuilderSAH runs (0: off, the default since round 5: it measured
// 0.0 % on Sponza-class for 30-55 ms of host build, profiles/r04v_ab_reinsert_undo_sponza.log, and
// the GPU builder reproduces the unrefined tree).
#ifndef PT_SAH_REINSERT
#define PT_SAH_REINSERT 0
#endif
double sah_reinsert(std::vector<uint32_t>& order, std::vector<int2>& child, std::vector<int2>& range,
                    std::vector<float4>& box, const float4* tri, int rounds);

// BVH4 (the SAH-optimal collapse of the builder's binary tree) + triangle records in leaf order.
struct BuildOutput {
    BNode4* nodes;  // capacity max(1, n) nodes
    float4* isect;  // 3n
    float4* shade;  // 4n
    float4* tuv;    // 2n or NULL
    int n_nodes;    // written by bvh_build; 0 after a failed build
    int depth;      // BVH4 levels
    // first node of every BVH4 level (breadth-first numbering) and, last, n_nodes: level l is
    // nodes level_base[l] .. level_base[l + 1] - 1 (refit_levels walks them deepest first)
    std::vector<int> level_base;
};

// The collapse's SAH constants (pt_build.hip k_sah_dp; refit's cost reduction uses the same).  With
// the dual traversal step (pt_device.h) a triangle test overlaps a node visit, hence cTri < cNode.
#ifndef PT_SAH_CTRI
#define PT_SAH_CTRI 0.5f
#endif
constexpr float kSahCNode = 1.0f;
constexpr float kSahCTri = PT_SAH_CTRI;

// GPU BVH build (pt_build.hip): in.builder's front end makes a binary tree and puts the triangle
// records in leaf order, then the common back end collapses the tree into the BVH4.  Replaces
// optixAccelBuild (OptixRenderer.cpp:306-456).
// Returns hipSuccess or the first error; *ms = device time of the build.
hipError_t bvh_build(const BuildInput& in, BuildOutput& out, hipStream_t stream, float* ms);

// Wavefront path state: SoA queues in HBM, capacity = paths (one path per pixel per frame).
struct WFState {
    float4* ray_o[2] = {nullptr, nullptr};  // queue b&1: origin.xyz | path id
    float4* ray_d[2] = {nullptr, nullptr};  // direction.xyz | 0
    float4* hit = nullptr;                  // path, u, v, tri | back<<31 (-1 = miss), queue order
    float4* beta = nullptr;                 // path throughput.xyz | seed: path order (Default / Layered),
                                            // queue order of the even bounces (fused modes)
    float4* beta_q = nullptr;               // fused modes: throughput | seed of the odd bounces' queues
    float4* L = nullptr;                    // path radiance of the frame, path order
    float4* sh_o = nullptr;                 // shadow queue: origin | path
    float4* sh_d = nullptr;                 // direction | tmax
    float4* sh_c = nullptr;                 // deferred NEE contribution (fused modes)
    int* aux = nullptr;                     // light index << 1 | conductor (RNG-coupled modes)
    int* vis = nullptr;                     // shadow result per shadow ray (RNG-coupled modes)
    int* nq = nullptr;                      // NEE items (RNG-coupled modes): kNeeRegions regions of `paths`,
                                            // two buckets each, one from either end (pt_wavefront.hip)
    int* sq = nullptr;                      // BSDF-sample items: kShadeBuckets regions of `paths`
    int* count = nullptr;                   // per bounce: queue, shadow, NEE and sample bucket lengths
    int paths = 0;
    int max_bounces = 0;
    // Look-ahead cancellation (pt_capi_ahead.cpp cancel_look_ahead), set per batch: a speculative
    // render-ahead batch carries the renderer's cancel words and the epoch it was enqueued under,
    // and its kernels stop early once the host has published a newer epoch (wf_cancelled,
    // trace_range).  Null for every other batch: no polling.
    const unsigned* cancel_host = nullptr;  // pinned host word: the newest cancel epoch (PCIe reads)
    unsigned* cancel_seen = nullptr;        // device relay of it (agent-scope loads, L2-served)
    unsigned cancel_epoch = 0;
    // pt_set_debug_hold (tests only): a speculative batch with this pinned word starts with k_hold,
    // which returns once the batch is cancelled, the word is set, or 10 s have passed
    const unsigned* hold_release = nullptr;
};
// Bytes of a queue set: the sum over the table of its arrays (pt_wavefront.hip kQueueArrays).
size_t wavefront_bytes(int paths, int max_bounces);
// Owner of a queue set's arrays: frees them in its destructor and hands out the WFState the kernels
// take by value.  alloc and release walk the same table as wavefront_bytes.
class WFQueues {
    WFState w_;

public:
    WFQueues() = default;
    WFQueues(const WFQueues&) = delete;
    WFQueues& operator=(const WFQueues&) = delete;
    ~WFQueues() { release(); }
    // Releases what it held first.  No partial queue set survives a failed allocation: paths() stays
    // 0, so the next launch_frames allocates again instead of launching on null queues.
    hipError_t alloc(int paths, int max_bounces);
    void release();
    const WFState& state() const { return w_; }
    int paths() const { return w_.paths; }
    int max_bounces() const { return w_.max_bounces; }
};
// pt_set_kernel_timing: the pools whose event pairs bracket a batch's k_extend launches, its
// k_trace_pair launches and the dominant shading launch of each bounce (k_shade_fused / k_shade0_pixel
// in the fused modes, k_shade_nee in Default / Layered).  The launcher draws a pair at the launch it
// brackets.  Null: not timed.
struct EventPool;  // pt_resource.h
struct WFTimers {
    EventPool* extend = nullptr;
    EventPool* pair = nullptr;
    EventPool* shade = nullptr;
};
// What a wavefront batch needs besides its DevLaunch and its queues.
struct WFBatch {
    int mode = 0;                // material mode (kMode*)
    bool stats = false;          // the trace kernels' STATS variants
    bool primary_dedup = false;  // trace the batch's identical camera rays once per pixel (k_extend `dup`)
    bool wide_trace = false;     // the call runs on one stream, so the trace kernels take the wide
                                 // workgroups (pt_wavefront.hip kBlockTraceWide)
    int cus = 0;                 // compute units of the device: the trace kernels' grids
    hipStream_t stream = nullptr;
    // optional: the batch's accumulate waits for accum_wait and records accum_done, so batches on
    // different streams still add into the sum in frame order
    hipEvent_t accum_wait = nullptr, accum_done = nullptr;
    WFTimers timers;
};
// Enqueue one batch (all bounces) of the wavefront pipeline: the L.n_frames frames from L.frame_base
// are traced together and added to L's destination (accum_batch); W must hold n_frames * n_pixels paths.
hipError_t launch_wavefront_batch(const DevScene& S, const DevLaunch& L, const WFState& W, const WFBatch& B);
// The accumulate stage (pt_accum.hip): adds the nf frames of `radiance` (the batch's WFState::L, nf
// records per launch pixel in path order) to L's destination in frame order.  L.pixel_map: the mapped
// kernel, into the fp32 sum and the adaptive moments (no accum64, no frame_stride).  L.ss_taps: every
// frame's image gathered through the (2 L.ss_R + 1)^2 taps of the frame's cell first (DESIGN.md §13;
// a whole image: row0 = 0 and no pixel map, L.ss_R from 1 to kFilterMaxR).  Else the plain kernel.
// hipErrorInvalidValue where a combination has no kernel.
constexpr int kFilterMaxR = 2;
hipError_t accum_batch(const float4* radiance, const DevLaunch& L, int nf, hipStream_t stream);
// sum32[i] = (float)sum64[i] (the multi-device fp64 reduce's result -> the fp32 sum buffer)
hipError_t accum_f64_to_f32(const double* sum64, float* sum32, size_t n, hipStream_t stream);

// Render launches.
hipError_t launch_render(int kernel, int mode, bool stats, const DevScene& S, const DevLaunch& L,
                         hipStream_t stream);
hipError_t launch_trace(const DevScene& S, const float* d_rays, int n, int* d_prim, float* d_thit, float* d_u,
                        float* d_v, int* d_back, int any_hit, hipStream_t stream);

// Lit table (pt_lit.h, pt_lit.hip).  lit_subdivide: the per-triangle words from a host copy of the
// leaf-ordered isect records; false = the scene runs without the table.  lit_build: clears and
// rebuilds the bits of n_lights lights (`words` 32-bit words each) on `stream`.  diagonal / diag: the
// scene box's diagonal, from which every cell takes its margin (lit_margin_cell).
bool lit_subdivide(const float4* isect, int ntri, std::vector<uint32_t>& words, uint32_t* cells, float* diagonal);
hipError_t lit_build(const DevScene& S, const uint32_t* tri_words, uint32_t cells, uint32_t words,
                     const DevLight* lights, int n_lights, uint32_t* bits, float diag, hipStream_t stream);
// The occluder candidate table (pt_lit.hip k_occ_build): occ[light * cells + cell] = -1 or a
// leaf-order triangle that probably occludes the cell's shadow rays; runs after lit_build on `stream`.
hipError_t occ_build(const DevScene& S, const uint32_t* tri_words, uint32_t cells, uint32_t words,
                     const DevLight* lights, int n_lights, const uint32_t* bits, int* occ, hipStream_t stream);
// The skip table (pt_skip.h, pt_lit.hip k_skip_build): words[2 t + side] = 0 or the BVH4 child link an
// extension ray leaving that side of leaf-order triangle t drops unvisited; node_parent (n_nodes + 1
// ints) and tri_parent (ntri ints) are the build's scratch.  Runs on `stream`.
hipError_t skip_build(const DevScene& S, int* node_parent, int* tri_parent, uint32_t* words, hipStream_t stream);

// Geometry updates (pt_refit.hip).  RefitMesh: what k_rebake needs of one mesh.
struct RefitMesh {
    float m[16];      // model matrix, column-major
    int dirty;        // re-bake this mesh's triangles
    int normal_mode;  // 0: its normals bake to zeros; 1: transformed here (kNormalBaked); 2: kept in
                      // object space (kNormalObject, pt_device.h)
    int pad[2];
};
// Re-bakes the records of the dirty meshes' triangles in place (isect / shade, leaf order).  overts /
// onorms: object-space vertices and normals of all meshes; tidx: per original triangle, its three
// indices into them.
hipError_t refit_rebake(const RefitMesh* meshes, const float4* overts, const float4* onorms, const int4* tidx, int n,
                        float4* isect, float4* shade, hipStream_t stream);
// Recomputes every node box from the triangle records, one launch per level, deepest first.
hipError_t refit_levels(BNode4* nodes, const float4* isect, const std::vector<int>& level_base, hipStream_t stream);
// SAH cost reduction: partial[0 .. sah_partial_blocks(n) - 1] = per-block fp64 sums (to be added in
// block order), partial[sah_partial_blocks(n)] = the root's half area.
int sah_partial_blocks(int n_nodes);
hipError_t sah_partial_launch(const BNode4* nodes, int n_nodes, double* partial, hipStream_t stream);

// Progressive view buffer (pt_display.hip).
hipError_t display_fill(float* p, size_t n, float v, hipStream_t stream);
hipError_t display_blend(float* fb, const float* frame, size_t n, float w, bool continuous, hipStream_t stream);

// First-hit feature buffers and the a-trous filter (pt_aov.hip).  AovBuffers: what k_gbuffer writes
// per pixel (row 0 = bottom): the seven AOVs of ptamd.h PT_AOV_*, the filter's 16-byte guide records
// (normal | 1 at a hit, 0 at a miss; position | depth; albedo | 0; Hit.u | Hit.v | prim's bits | 0,
// the weights of v1 and v2 at the hit and 0, 0 at a miss) and the count of hit pixels.
struct AovBuffers {
    float *albedo, *normal, *gnormal, *position, *depth, *rough_metal;
    int* prim;
    float4 *guide_n, *guide_p, *guide_a, *guide_b;
    unsigned long long* hits;  // one counter, zeroed by the caller
};
// L: width, height, row0, image_height and the camera are read, nothing else.
hipError_t gbuffer_render(const DevScene& S, const DevLaunch& L, const AovBuffers& B, hipStream_t stream);
// One filter iteration: cin -> cout, or with `last` -> out (W*H*3, remodulated).
struct AtrousParams {
    const float4* cin;
    float4* cout;
    float* out;
    const float4 *gn, *gp, *ga;
    int w, h, step;
    float inv_c, inv_n, inv_p, floor;
    int demodulate;
};
// The iterations of a step up to lds_max_step (at most kAtrousLdsMaxStep; 0 = none) stage their
// tile and its halo in LDS, the others load every tap from global memory.  Same bits either way.
// Steps 1, 2, 4: a (16 + 4 step)^2 tile of 48 B records (49 KB at step 4); steps 8 and 16: 12 rows
// `step` apart of 32 + 4 step records (55 KB at step 16).
constexpr int kAtrousLdsMaxStep = 16;
constexpr int kAtrousLdsDefaultStep = 16;  // what pt_denoise uses: the fastest measured
// c[p] = in[p] * scale, divided by max(albedo, floor) at the hit pixels when demodulate.
hipError_t atrous_pack(const float* in, float scale, bool demodulate, float floor, const float4* gn, const float4* ga,
                       float4* c, size_t n, hipStream_t stream);
hipError_t atrous_iteration(const AtrousParams& A, bool last, int lds_max_step, hipStream_t stream);

// Temporal reprojection and the variance-guided filter (pt_temporal.hip).  Records
// of 16 bytes throughout: colour | variance, and moment 1 | moment 2 | history length | 0.
struct TemporalParams {
    const float4* c;           // this call's packed colour (atrous_pack)
    const float4 *gn, *gp;     // this view's guides
    const float4 *pgn, *pgp;   // the previous call's guides
    const float4 *hc, *hm;     // the previous call's colour and moment records
    float4 *tc, *tm;           // out: blended colour | variance, and the moment record
    unsigned long long* count; // [0] hit pixels with accepted history, [1] without, [2] moved (motion
                               // only); zeroed by the caller
    int w, h, history;         // history = 0: no previous call to reproject into
    float prev_view[16], prev_proj[16];  // inverses of the previous call's inv_view and inv_proj
    float alpha, alpha_moments, max_history, normal_cos, plane_distance;
    // motion only: the barycentric guide records, the vertex snapshot (3 records per global
    // triangle, `ntri` of them) and where each pixel's previous position goes (0 at a miss)
    const float4 *gb, *snap;
    float4* pp;
    int ntri;
};
// motion: a hit pixel is reprojected from the point its triangle's snapshot vertices give at the
// hit's barycentrics (DESIGN.md §11 "Motion vectors") instead of from its present position.
hipError_t temporal_blend(const TemporalParams& T, bool motion, hipStream_t stream);
// snap[3 g .. 3 g + 2] = the world-space vertices of leaf-order triangle t, g = its global index (isect[3 t].w).
hipError_t temporal_snapshot(const float4* isect, const float4* shade, int ntri, float4* snap, hipStream_t stream);
// out[3 p ..] = (fx - x, fy - y, 1) of §11 step 1 for pp[p] where gn[p].w != 0, history and clip.w > 0; else 0, 0, 0.
hipError_t temporal_motion_screen(const float4* pp, const float4* gn, const float* prev_view, const float* prev_proj,
                                  int history, int w, int h, float* out, hipStream_t stream);
// tc[p].w of the hit pixels whose history is shorter than variance_history: the 7x7 estimate from tm.
hipError_t temporal_variance(const float4* gn, const float4* gp, const float4* tm, float4* tc, int w, int h, float inv_n,
                             float inv_p, float variance_history, hipStream_t stream);
// den[p] = sigma_luminance * sqrt(3x3 Gaussian of cin.w) + 1e-8: the colour term's divisor of one iteration.
hipError_t temporal_luminance_scale(const float4* cin, const float4* gn, float* den, int w, int h, float sigma_luminance,
                                    hipStream_t stream);
// One variance-guided iteration: AtrousParams as for atrous_iteration (inv_c is not read), den from
// temporal_luminance_scale, and hist = where the colour | variance result is stored besides (or NULL).
hipError_t temporal_atrous_iteration(const AtrousParams& A, const float* den, float4* hist, bool last, int lds_max_step,
                                     hipStream_t stream);

// Adaptive sampling (pt_adaptive.hip).  AdaptiveBuffers: the image-sized state
// (row 0 = bottom), the per-tile state (8x8 tiles from pixel (0, 0), row-major, clipped at the right
// and top edges) and the list of the next round's pixels.
constexpr int kTileActive = 1;   // rendered in the next round
constexpr int kTileStopped = 0;  // its error met the threshold
constexpr int kTileFull = 2;     // it holds max_samples samples
struct AdaptiveBuffers {
    int w, h, tiles_x, tiles_y;
    uint32_t* n;       // samples per pixel
    double* moments;   // S1, S2 per pixel
    float* err;        // e per pixel, of the last estimate it took part in
    float* tile_err;   // the same per tile
    int* tile_rounds;  // rounds the tile was rendered in
    int* tile_state;   // kTile*
    int *tile_cnt, *tile_off;  // the compaction's counts and their exclusive scan
    int* pixel_map;    // image pixels of the active tiles: tile ascending, raster order inside
    int* count;        // its length
    void* scan_tmp;    // hipCUB's scratch, scan_bytes of it (adaptive_scan_bytes)
    size_t scan_bytes;
};
hipError_t adaptive_scan_bytes(int tiles, size_t* bytes);
// After a round: e and the tile error of the tiles it rendered, their new state, then adaptive_compact.
hipError_t adaptive_estimate(const AdaptiveBuffers& A, float threshold, uint32_t min_samples, uint32_t max_samples,
                             float luminance_floor, hipStream_t stream);
// pixel_map and count from tile_state.
hipError_t adaptive_compact(const AdaptiveBuffers& A, hipStream_t stream);
// mean[3 p ..] = sum[3 p ..] / (float)n[p]
hipError_t adaptive_resolve(const float* sum, const uint32_t* n, float* mean, int pixels, hipStream_t stream);

}  // namespace pt
