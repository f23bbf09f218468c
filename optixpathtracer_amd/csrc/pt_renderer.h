// pt_renderer.h — the renderer behind the C ABI (include/ptamd.h) and what the driver's translation
// units share: pt_capi.cpp (entry points), pt_capi_bake.cpp, pt_capi_scene.cpp, pt_capi_launch.cpp,
// pt_capi_ahead.cpp, pt_capi_tables.cpp, pt_capi_stats.cpp, pt_capi_denoise.cpp, pt_capi_temporal.cpp, pt_capi_adaptive.cpp and pt_capi_filter.cpp.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ptamd.h"
#include "pt_internal.h"
#include "pt_lit.h"
#include "pt_resource.h"

namespace pt {

// The calling thread's last error (pt_last_error); both return the status they are given or derive.
extern thread_local std::string g_last_error;
int fail(int code, const std::string& msg);
// Device allocations that fail for lack of memory report PT_ERR_NOMEM (the caller can retry
// with fewer frames per launch); every other HIP failure is PT_ERR_HIP.
int hip_fail(hipError_t e, const char* where);

#define PT_HIP(call, where)                              \
    do {                                                 \
        hipError_t e__ = (call);                         \
        if (e__ != hipSuccess) return hip_fail(e__, where); \
    } while (0)

// event pairs held by one renderer before launch_frames retires them (EventPool)
constexpr size_t kMaxPendingEvents = 4096;
// the smallest traversal stack of any kernel (pt_device.h stack_capacity: 71 entries for the
// wavefront's 11 LDS entries and 64 spill slots in chunks of 5)
constexpr int kMinTraversalStack = std::min(stack_capacity(PT_WF_STACK), stack_capacity(PT_MK_STACK));

// The scene as pt_create received it, kept for geometry updates (pt_commit_geometry): object-space
// vertices and normals of all meshes concatenated, per-triangle global vertex indices in original
// order, the per-mesh matrices, and what else the bake and a rebuild need.
struct GeomHost {
    std::vector<float4> verts, norms;  // xyz | 0; norms are zeros for a mesh without normals
    std::vector<int4> tidx;            // per original triangle: three indices into verts, w = mesh
    std::vector<float> model;          // 16 per mesh
    std::vector<int> voff;             // first vertex of mesh m (n_meshes + 1 entries)
    std::vector<int> has_normals, alpha;  // per mesh: normals given; albedo-textured (cut-out flag)
    std::vector<float4> uvs;           // 2 per triangle, textured scenes only
    int n_meshes() const { return (int)has_normals.size(); }
    // pt_device.h normal mode of mesh m under its present matrix: kNormalBaked where the 3x3 part has
    // at most one entry per row and that entry is +-1 (transforming the vertex normals first then
    // gives the bits of the reference's order), kNormalObject otherwise
    int normal_mode(int m) const {
        if (!has_normals[(size_t)m]) return 0;
        const float* M = &model[16 * (size_t)m];
        for (int r = 0; r < 3; ++r) {
            int nonzero = 0;
            for (int c = 0; c < 3; ++c) {
                const float e = M[4 * c + r];
                if (e != 0.0f) ++nonzero;
                if (e != 0.0f && e != 1.0f && e != -1.0f) return 2;
            }
            if (nonzero > 1) return 2;
        }
        return 1;
    }
    // rows [1].y and [3..5] of mesh m's material record (pt_device.h): the normal mode and the matrix rows
    void normal_rows(int m, float4* rec) const {
        const float* M = &model[16 * (size_t)m];
        rec[1].y = (float)normal_mode(m);
        for (int r = 0; r < 3; ++r) rec[3 + r] = make_float4(M[r], M[4 + r], M[8 + r], M[12 + r]);
    }
};

// The changes to one mesh staged since the last commit (pt_set_mesh_transform / pt_set_mesh_vertices).
struct StagedMesh {
    bool has_model = false, has_verts = false, has_norms = false;
    float model[16];
    std::vector<float> verts, norms;
};

// Everything a 1-spp image depends on besides its frame id (render_key).
struct RenderKey {
    int w = 0, h = 0, n_lights = 0, max_bounces = 0, mode = 0, kernel = 0, debug_pixel = -1;
    uint32_t lights_version = 0, debug_frame = 0, debug_version = 0, geom_version = 0, filter_version = 0;
    const void* lights = nullptr;
    float cam[3 + 16 + 16] = {};
    bool operator==(const RenderKey& o) const {
        return w == o.w && h == o.h && n_lights == o.n_lights && max_bounces == o.max_bounces && mode == o.mode &&
               kernel == o.kernel && debug_pixel == o.debug_pixel && lights_version == o.lights_version &&
               debug_frame == o.debug_frame && debug_version == o.debug_version && geom_version == o.geom_version &&
               filter_version == o.filter_version && lights == o.lights &&
               std::memcmp(cam, o.cam, sizeof cam) == 0;
    }
};

// What the first hit of a pixel depends on: the part of the render key that the G-buffer is cached
// under (pt_capi_ahead.cpp view_key).
struct ViewKey {
    int w = 0, h = 0;
    uint32_t geom_version = 0;
    float cam[3 + 16 + 16] = {};
    bool operator==(const ViewKey& o) const {
        return w == o.w && h == o.h && geom_version == o.geom_version && std::memcmp(cam, o.cam, sizeof cam) == 0;
    }
};

// Two ring slots: once the ramp reaches its length, pt_render enqueues the next batch into
// the other slot while the caller downloads this one's frames (on dl_stream, after the
// slot's `ready` event), so rendering and the device-to-host copies overlap.
struct RingSlot {
    DevBuf<float> d;
    int cap(size_t n3) const { return (int)(d.size() / n3); }  // frames of n3 floats it has room for
    uint32_t first = 0, n = 0;
    RenderKey key;
    Event start, ready;        // recorded on `stream` around the slot's batch
    bool measured = true;      // its duration is in frame_ms_est
    bool speculative = false;  // a cancellable look-ahead batch (cancel_look_ahead)
    // a speculative batch a call has taken a frame from (render_frame_image): no longer
    // cancellable, and a cancel of a later batch waits for it first
    bool served = false;
};

// What the lit table and the occluder table each keep about their last build: what it was built
// for, the events around it, and a figure counted from its contents when the statistics first ask
// (pt_capi_tables.cpp).
struct BuiltTable {
    uint32_t version = 0;  // the lit version, the light array and the light count it was built for
    const void* lights = nullptr;
    int n = 0;
    Event ev[2];  // around the last build
    bool ev_pending = false;
    double build_ms = 0.0;
    int64_t count = -1;  // of the last build; -1 = not counted yet (pt_get_stats)
    bool current(uint32_t v, const void* l, int nl) const { return version == v && lights == l && n == nl; }
    int begin(hipStream_t stream);  // before the build's launches
    int end(hipStream_t stream, uint32_t v, const void* l, int nl);  // after them: built for (v, l, nl)
    void harvest();  // the last build's events -> build_ms; the caller has waited for them
    void invalidate_count() { count = -1; }
};

}  // namespace pt

// Members are destroyed in reverse order of declaration: the streams are declared first, so they
// outlive every buffer, event and queue set that work still in flight on them may use.
struct pt_renderer {
    int device = 0;
    pt::Stream stream;
    pt::Stream dl_stream;
    // wavefront batches alternate between two streams, each with its own queues, so one batch's
    // kernels overlap the other's (pt_set_wavefront_streams; 1 = everything on `stream`)
    static constexpr int kMaxWFStreams = 4;
    int wf_streams = 0;  // 0 = auto (launch_frames): two for Conductor and Dielectric, one otherwise
    pt::Stream xstream[kMaxWFStreams];  // [0] unused: stream 0 is `stream`
    pt::WFQueues xwf[kMaxWFStreams];    // [0] unused: stream 0's queues are `wf`
    pt::Event ev_fork, ev_join[kMaxWFStreams], ev_accum[2];
    hipStream_t wf_stream(int k) const { return k ? xstream[k] : stream; }
    // scene
    pt::DevBuf<pt::BNode4> d_nodes;
    pt::DevBuf<float4> d_isect;
    pt::DevBuf<float4> d_shade;
    int bvh_nodes = 0, bvh_depth = 0;
    bool trav_stats = false;
    pt::WFQueues wf;
    pt::DevBuf<float4> d_mats;
    int ntri = 0;
    int nmesh = 0;
    // launch state (LaunchParams.h:9-28)
    int width = 0, height = 0;
    float cam_pos[3] = {0, 0, 0};
    float inv_view[16] = {0};
    float inv_proj[16] = {0};
    pt::DevBuf<pt::DevLight> lights_own;  // the renderer's own light array (pt_set_lights)
    pt::DevLight* d_lights = nullptr;     // the array in use: lights_own, or a pt_launch caller's
    int n_lights = 0;
    int max_bounces = 0;
    int material_mode = PT_MAT_DEFAULT;
    int kernel = PT_KERNEL_MEGA;
    uint32_t frame_id = 0;
    // buffers
    pt::DevBuf<float4> d_tuv;       // per-triangle texcoords (leaf order), textured scenes only
    pt::DevBuf<uint32_t> d_texels;  // RGBA8 texel pool
    pt::DevBuf<int4> d_texinfo;     // per texture: offset, width, height
    pt::DevBuf<float> d_frame;      // 1-spp frame (pt_render)
    pt::Event ev_frame;  // after the d_frame render (no ring)
    // a one-frame call in row bands (pt_set_band_split): band 0 holds the first band0_rows rows
    // (0: the last one-frame call was not banded); ev_band0 follows its k_accum, so pt_render can
    // download them while band 1 still renders
    int band0_rows = 0;
    pt::Event ev_band0;
    uint32_t lights_version = 0;
    uint32_t debug_version = 0;  // bumped by pt_set_debug_pixel (the records are rewritten)
    pt::DevBuf<float> d_display;  // progressive view buffer (pt_display_*)
    int display_max = -1;
    int display_samples = 0;
    bool display_ready = false;
    pt::DevBuf<float> d_accum;  // internal sum buffer
    float* user_accum = nullptr;
    pt::DevBuf<unsigned long long> d_counters;
    bool primary_dedup = true;  // pt_set_primary_dedup
    bool band_split = true;     // pt_set_band_split: one-frame calls render two row bands on two streams
    bool wide_trace = true;     // one-stream calls: wide trace workgroups (PTAMD_WIDE_TRACE env 0 turns it off)
    int frames_per_launch = 128;  // 56 GB of queues at 1080p (16 -> 64 frames +5 % Lambert,
                                  // 64 -> 128 with the ray pools +0.7 to +2.5 %)
    int nf_fit = 0;  // > 0: the largest batch whose queues fitted after an out-of-memory halving
                     // (launch_frames); cleared by pt_set_frames_per_launch and pt_resize, and once
                     // the free memory would hold the full batch again
    // pt_set_queue_budget: the most bytes all wavefront streams' queues may hold together
    // (0 = default, a quarter of the device memory; < 0 = no budget, only the 2^28-path cap)
    int64_t queue_budget = 0;
    int last_streams = 0, last_batch = 0;  // streams and frames per batch of the last wavefront call
    // pt_set_accum_fp64: the sum is kept in fp64 (d_accum64; device 0 of a multi-device renderer
    // also multi.d_part64), accum() holds its fp32 rounding
    bool accum64 = false;
    pt::DevBuf<double> d_accum64;
    // debug path (pt_set_debug_pixel): pixel W*y+x (-1 = off), frame id, per-bounce records
    int debug_pixel = -1;
    uint32_t debug_frame = 0;
    pt::DevBuf<float> d_debug;

    // geometry updates (pt_set_mesh_transform / pt_set_mesh_vertices / pt_commit_geometry): the
    // retained scene on the host and on the device, the changes staged since the last commit, the
    // tree's level bases for the refit, and the SAH cost of the tree now and as last built
    struct Geom {
        pt::GeomHost host;
        std::vector<float4> mats;  // host copy of d_mats: a new matrix rewrites its mesh's normal mode and rows
        std::vector<pt::StagedMesh> staged;
        bool any_staged = false;
        int builder = pt::kBuilderSAHGPU;
        std::vector<int> level_base;
        pt::DevBuf<float4> d_overts;
        pt::DevBuf<float4> d_onorms;
        pt::DevBuf<int4> d_tidx;
        pt::DevBuf<pt::RefitMesh> d_rmesh;
        pt::DevBuf<double> d_sah_part;  // sah_partial_blocks(max(1, ntri)) + 1 doubles
        pt::Event ev[2];
        uint32_t version = 0;  // bumped per commit: no ring frame rendered before it is served after
        uint64_t commits = 0, refits = 0, rebuilds = 0;
        double commit_ms = 0.0;
        double sah_cost = 0.0, sah_cost_built = 0.0;
        double sah_root_built = 0.0;  // the root's half area as last built: both costs are relative to it
    } geom;

    // render-ahead (pt_set_render_ahead): while nothing that changes the image changes between
    // pt_render calls, a miss renders the next k frames in one wavefront batch into a ring of
    // 1-spp images (k doubling per sequential miss up to max_frames), and the calls for those
    // frame ids download them from the ring
    struct Ahead {
        int max_frames = 64;
        // A render-ahead batch is also bounded by memory and by time (ahead_frames): its queues and
        // the two ring slots take at most a quarter of the device memory (and only what is free), and
        // its estimated duration stays within budget_ms (pt_set_render_ahead_budget), so a
        // call that changes the state waits for at most about that much work already enqueued.
        double budget_ms = 50.0;
        double frame_ms_est = 0.0;  // ms per frame of the last measured ring batch (0: none yet)
        int oom_cap = 1 << 30;  // largest batch since an allocation failed (reset per sequence)
        pt::RingSlot ring[2];
        int ring_k = 1, ring_last = 0;  // ramp length, slot rendered last
        bool spec_pending = false;      // a look-ahead batch was enqueued since the last collect
        // render-ahead frames rendered into the ring and calls served from it (pt_stats)
        uint64_t rendered = 0, served = 0;
        // Look-ahead cancellation (cancel_look_ahead, pt_wavefront.hip wf_cancel_poll): the newest
        // cancel epoch in pinned host memory, which the kernels of a speculative batch read over PCIe
        // (cancel.d) and relay through a device word (d_cancel_seen); cancel_epoch is the epoch
        // the next speculative batch is enqueued under.
        pt::PinnedWord cancel;
        pt::DevBuf<unsigned> d_cancel_seen;
        unsigned cancel_epoch = 0;
        uint64_t cancelled = 0;  // look-ahead batches cancelled (pt_stats)
        // pt_set_debug_hold (tests): the next speculative batches start with k_hold, which waits until
        // the batch is cancelled, the pinned release word is set, or 10 s pass
        bool debug_hold = false;
        pt::PinnedWord hold;
        uint64_t held = 0;  // speculative batches enqueued behind a hold (pt_stats)
        void reset_counts() { rendered = served = cancelled = held = 0; }  // pt_stats_reset
    } ahead;

    // stats: one HIP event pair per kernel launch, on the library stream
    struct Timing {
        pt::EventPool ev;
        uint64_t launches = 0;
        // optional per-launch timing of the wavefront's closest-hit trace kernel (k_extend)
        bool kernel_timing = false;
        pt::EventPool tev;
        double trace_ms = 0.0;
        uint64_t trace_launches = 0;
        // the k_trace_pair launches among them (fused modes: every timed trace launch after a batch's
        // k_extend), in a pool of their own so their time is reported per kernel (pt_stats pair_kernel_*)
        pt::EventPool pev;
        double pair_ms = 0.0;
        uint64_t pair_launches = 0;
        // the same for the dominant shading kernel of a bounce (pt_stats shade_kernel_*)
        pt::EventPool sev;
        double shade_ms = 0.0;
        uint64_t shade_launches = 0;
        bool pending = false;
        uint64_t samples = 0;
        double last_ms = 0.0, total_ms = 0.0;
        uint64_t calls = 0;
        double bvh_ms = 0.0;
        void reset_counts() {  // pt_stats_reset: everything but the build time
            samples = calls = launches = trace_launches = pair_launches = shade_launches = 0;
            last_ms = total_ms = trace_ms = pair_ms = shade_ms = 0.0;
        }
    } timing;

    // multi-device (pt_options.n_devices >= 1): this renderer is device 0 of the list; peers are
    // single-device renderers of the other devices; comms[g] is device g's RCCL communicator
    struct Multi {
        std::vector<pt_renderer*> peers;
        std::vector<ncclComm_t> comms;
        pt::DevBuf<float> d_part;  // device 0's own partial sum (the total is accum())
        pt::DevBuf<double> d_part64;
    } multi;

    // lit table (pt_lit.h): the per-triangle words are fixed at pt_create (d_tri NULL: the scene
    // runs without it), the bits follow the lights: lit_prepare rebuilds them on `stream` when
    // version (bumped by pt_set_lights, and by a pt_launch with the table forced on, whose device light array the
    // host cannot compare) or the light array differ from what they were built for
    struct Lit {
        int mode = -1;  // pt_set_lit_table: < 0 auto, 0 off, > 0 on
        pt::DevBuf<uint32_t> d_tri;
        pt::DevBuf<uint32_t> d_bits;  // kLitMaxLights * words
        uint32_t cells = 0, words = 0;
        uint32_t words_cap = 0;  // words per light d_bits has room for (a commit may grow the table)
        float diag = 0.0f;  // the scene box's diagonal: every cell's margin follows from it (lit_margin_cell)
        uint32_t version = 1;
        bool active = false;  // this call's launches read the table (make_launch)
        bool launch_call = false;  // inside pt_launch: auto leaves the table alone (lit_wanted)
        pt::BuiltTable built;  // count: the bits set
    } lit;
    // occluder candidate table (pt_lit.hip k_occ_build): one int per (light, cell), sized for the
    // lights in use and rebuilt after the bits whenever they are (occ_prepare; a failed allocation
    // means the renderer runs without it); pt_occluder_table_upload replaces the entries until then
    struct Occ {
        int mode = -1;  // pt_set_occluder_table: < 0 auto, 0 off, > 0 on
        pt::DevBuf<int> d_tab;  // n_lights * lit.cells entries in use; size(): entries it has room for
        bool alloc_failed = false;  // no memory for it: the renderer runs without (until the cells change)
        bool active = false;  // this call's launches read the table (make_launch)
        pt::BuiltTable built;  // count: entries >= 0 of the last build or upload
    } occ;
    // skip table (pt_skip.h): two words per leaf-ordered triangle, a function of the triangle records
    // and the BVH numbering alone.  version is bumped wherever either changes (lit_resubdivide: the
    // scene build and every geometry commit); skip_prepare rebuilds the words on `stream` when they
    // are stale (a failed allocation means the renderer runs without the table)
    struct Skip {
        int mode = -1;  // pt_set_skip_table: < 0 auto, 0 off, > 0 on
        pt::DevBuf<uint32_t> d_words;              // 2 * ntri
        pt::DevBuf<int> d_node_parent, d_tri_parent;  // the build's scratch
        uint32_t version = 1;
        bool in_bounds = false;  // every vertex within kLitMaxCoord (pt_skip.h)
        bool alloc_failed = false;
        bool active = false;  // this call's launches read and write the words (make_launch)
        pt::BuiltTable built;
    } skip;

    // first-hit feature buffers and the denoiser (pt_capi_denoise.cpp, pt_aov.hip): the G-buffer of
    // the view it was rendered for (gbuffer_prepare renders it again when view_key differs), the
    // filter's ping-pong colour records, its W*H*3 result and the upload buffer of a host source.
    // All of the renderer's size: pt_resize frees them.
    struct Aov {
        pt::DevBuf<float> d_albedo, d_normal, d_gnormal, d_position, d_depth, d_rough_metal;
        pt::DevBuf<int> d_prim;
        pt::DevBuf<float4> d_gn, d_gp, d_ga, d_gb;  // guide records (pt_internal.h AovBuffers)
        pt::DevBuf<unsigned long long> d_hits;
        pt::DevBuf<float4> d_c[2];
        pt::DevBuf<float> d_out, d_in;
        pt::ViewKey key;
        bool rendered = false;  // the G-buffer holds key's view
        uint64_t renders = 0;
        int iterations = 0;  // of the last pt_denoise
        pt::Event ev_g[2], ev_f[2];  // around the last G-buffer render and the last filter run
        bool g_timed = false, f_timed = false;
        void release() {
            for (pt::DevBuf<float>* b :
                 {&d_albedo, &d_normal, &d_gnormal, &d_position, &d_depth, &d_rough_metal, &d_out, &d_in})
                b->reset();
            for (pt::DevBuf<float4>* b : {&d_gn, &d_gp, &d_ga, &d_gb, &d_c[0], &d_c[1]}) b->reset();
            d_prim.reset();
            rendered = g_timed = f_timed = false;
        }
    } aov;

    // temporal reprojection (pt_capi_temporal.cpp, pt_temporal.hip): what the last
    // pt_denoise_temporal left for the next one -- its guides and camera, the colour | variance
    // history (iteration 0's result), the moment records (two sets: a call reads one and writes
    // the other) -- and what pt_temporal_download shows of that call.
    struct Temporal {
        pt::DevBuf<float4> d_pgn, d_pgp;  // the guides of the last call's view
        pt::DevBuf<float4> d_hc;          // colour | variance history
        pt::DevBuf<float4> d_m[2];        // moment 1 | moment 2 | length | 0; d_m[cur] is the last call's
        pt::DevBuf<float4> d_tc;          // what entered iteration 0: blended colour | variance
        pt::DevBuf<float> d_den;          // the colour term's divisor of one iteration
        pt::DevBuf<unsigned long long> d_count;  // reprojected, reset, moved
        int cur = 0;
        bool valid = false;  // d_pgn .. d_m[cur] hold a call's state
        float inv_view[16] = {}, inv_proj[16] = {};  // of that call
        uint64_t calls = 0;
        pt::Event ev[4];  // pack + blend | variance | iterations
        bool timed = false;
        // motion vectors (pt_temporal_options.motion_vectors): the world-space vertices per global
        // triangle as of geometry version snap_version; snap_prev = it shows the geometry of the last
        // call, which had the option on.  d_pp: the previous positions the motion kernel wrote.
        pt::DevBuf<float4> d_snap, d_pp;
        uint32_t snap_version = 0;
        bool snap_have = false, snap_prev = false;
        bool mv_last = false, mv_used = false;  // the last call: the option was on; the motion kernel ran
        bool had_history = false;               // ... and it had a history,
        float prev_view[16] = {}, prev_proj[16] = {};  // which it reprojected through these
        pt::Event ev_s[2];  // around the last call's snapshot
        bool snap_timed = false;
        void release() {
            for (pt::DevBuf<float4>* b : {&d_pgn, &d_pgp, &d_hc, &d_m[0], &d_m[1], &d_tc, &d_snap, &d_pp}) b->reset();
            d_den.reset();
            valid = timed = snap_have = snap_prev = mv_last = mv_used = had_history = snap_timed = false;
        }
    } temporal;

    // adaptive sampling (pt_capi_adaptive.cpp, pt_adaptive.hip): the state of the last
    // pt_render_adaptive and what pt_get_adaptive_info reports of it.  pt_resize frees the buffers,
    // pt_accum_clear drops the state (the sum it describes is gone).
    struct Adaptive {
        pt::AdaptiveStore buf;
        bool valid = false;  // buf holds a finished call's state, of the renderer's size
        int rounds = 0;
        double render_ms = 0.0, estimate_ms = 0.0;
        pt::EventPool ev;  // around every round's estimate, and the resolve
        void release() {
            buf.release();
            valid = false;
        }
    } adaptive;

    // pixel filter (pt_capi_filter.cpp, pt_accum.hip): the setting with radius and param resolved,
    // its tap radius R = ceil(radius - 1/2) and the tables the launches point at.  version is part of
    // the render key: no ring frame rendered under another setting is served.
    struct Filter {
        pt_pixel_filter set = {(uint32_t)sizeof(pt_pixel_filter), 1, PT_FILTER_BOX, 0.5f, 0.0f};
        int R = 0;
        pt::FilterStore buf;
        uint32_t version = 0;
        bool active() const { return set.supersample > 1 || R > 0; }
    } filter;

    pt_renderer() = default;  // no destructor: every member releases what it holds
    pt::DevScene scene() const {
        pt::DevScene S;
        S.nodes = d_nodes;
        S.isect = d_isect;
        S.shade = d_shade;
        S.mats = d_mats;
        S.tuv = d_tuv;
        S.texels = d_texels;
        S.texinfo = d_texinfo;
        S.ntri = ntri;
        S.n_nodes = bvh_nodes;
        S.lds_nodes = nullptr;
        S.n_lds = 0;
        return S;
    }
    float* accum() const { return user_accum ? user_accum : d_accum.get(); }
};

namespace pt {

// pt_capi_bake.cpp (host only).  ingest_scene: validates the scene and copies it into the retained
// form, the material records and the texture table; on a rejection *err holds the message and
// nothing else is written.
int ingest_scene(const pt_scene* scene, GeomHost& G, std::vector<float4>& mats, std::vector<int4>& texinfo,
                 size_t* ntexel, bool* any_tex, std::string* err);
void bake_scene(const GeomHost& G, std::vector<float4>& tri, std::vector<float4>& nrm, float cmin[3], float cmax[3]);

// pt_capi_scene.cpp
int upload_scene(pt_renderer* r, const pt_scene* scene, const std::vector<int4>& texinfo, size_t ntexel);
int build_scene(pt_renderer* r, bool any_tex);
int commit_geometry(pt_renderer* r, int how);

// pt_capi_launch.cpp
size_t queue_bytes_held(const pt_renderer* r);
size_t queue_budget_bytes(const pt_renderer* r);
// What makes a launch a mapped one (DevLaunch::pixel_map): `count` image pixels and their adaptive state.
struct PixelMap {
    const int* map;
    int count;
    uint32_t* n;
    double* moments;
};
// One call of launch_frames: frames first .. first + n - 1 and where they go.
struct FrameCall {
    uint32_t first = 0, n = 0;
    float* accum = nullptr;          // the fp32 sum the frames add into
    double* accum64 = nullptr;       // pt_set_accum_fp64: the fp64 sum; accum then holds its fp32 rounding
    size_t frame_stride = 0;         // > 0: frame first + j is written alone to accum + j * frame_stride
    bool speculative = false;        // a cancellable look-ahead batch (cancel_look_ahead)
    const PixelMap* pixels = nullptr;  // a mapped call: these pixels of the image only
};
int launch_frames(pt_renderer* r, const FrameCall& c);
int render_frames_multi(pt_renderer* r, uint32_t first, uint32_t n);

// pt_capi_ahead.cpp
ViewKey view_key(const pt_renderer* r);
void ring_free(pt_renderer* r);
void cancel_look_ahead(pt_renderer* r, bool force = false);
int render_frame_image(pt_renderer* r, const float** img, hipEvent_t* ready = nullptr, bool look_ahead = false,
                       hipEvent_t* part_ready = nullptr, size_t* part_floats = nullptr);

// pt_capi_tables.cpp
bool lit_wanted(const pt_renderer* r);
bool occ_wanted(const pt_renderer* r);
bool table_current(const pt_renderer* r, const BuiltTable& t);
int lit_prepare(pt_renderer* r);
int lit_resubdivide(pt_renderer* r);
int lit_table_download(pt_renderer* r, pt_lit_table_info* info, uint32_t* tri_words, int64_t tri_bytes, uint32_t* bits,
                       int64_t bits_bytes);
int occ_table_download(pt_renderer* r, int64_t* entries_out, int32_t* entries, int64_t bytes);
int occ_table_upload(pt_renderer* r, const int32_t* entries, int64_t bytes);
bool skip_wanted(const pt_renderer* r);
int skip_prepare(pt_renderer* r);
int skip_table_download(pt_renderer* r, int64_t* words_out, uint32_t* words, int64_t bytes);

// pt_capi_stats.cpp
int collect_pending(pt_renderer* r);

// The first min(struct_size, sizeof(T)) bytes of a versioned struct travel; 0 = the size field itself is cut off.
template <class T>
size_t versioned_bytes(const T* s) {
    return s->struct_size < sizeof(uint32_t) ? 0 : std::min<size_t>(s->struct_size, sizeof(T));
}
// `into` holds the defaults and takes what the caller's struct (or NULL) has of them; the bytes as above.
template <class T>
size_t versioned_merge(T& into, const T* user) {
    const size_t n = user ? versioned_bytes(user) : sizeof(T);
    if (user && n) std::memcpy(&into, user, n);
    return n;
}
// d, under the caller's struct_size, into as much of the caller's struct as that size covers; the bytes as above.
template <class T>
size_t versioned_write(T* user, T d) {
    const size_t n = versioned_bytes(user);
    d.struct_size = user->struct_size;
    std::memcpy(user, &d, n);
    return n;
}

// pt_capi_denoise.cpp
int gbuffer_prepare(pt_renderer* r);
// What pt_denoise and pt_denoise_temporal do alike, in the order their checks fire: check_source,
// merge, begin (the caller's own checks in between), finish.  Errors carry the entry point's name, `fn`.
struct DenoiseCall {
    const char* fn;
    pt_renderer* r;
    int32_t source;
    const float* host_in;
    pt_denoise_options o;  // merge: the defaults under the caller's options
    size_t n;              // begin: pixels
    const float* src;      // begin: the source on the device; a host source is uploaded
    int lds;               // begin: the largest step whose iteration stages its tile in LDS
    AtrousParams P;        // begin: the fields that every iteration shares

    int err(int code, const char* what) const;
    int check_source() const;
    int merge(const pt_denoise_options* opt);
    // checks o (sigma_color only if it is read) and the state; the G-buffer is current and the buffers exist
    int begin(bool reads_sigma_color);
    int finish(float* host_out) const;  // the download, unless host_out is NULL
};

// pt_capi_filter.cpp
// Whether the supersampled image of a w x h frame has 2^31 pixels or more: its pixel index is the
// path's seed and an int on the device.
bool filter_image_too_large(int supersample, int64_t w, int64_t h);

// pt_capi.cpp
void mat4_inverse(const float* m, float* out);

}  // namespace pt
