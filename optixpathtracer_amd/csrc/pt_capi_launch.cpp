// pt_capi_launch.cpp — enqueueing frames: the launch record, the queue budget, the wavefront plan and
// its batches, the megakernel loop, the multi-device split.
#include "pt_renderer.h"

using namespace pt;

namespace {

int next_event_pair(pt_renderer* r, hipEvent_t* a, hipEvent_t* b) {
    PT_HIP(r->timing.ev.next(a, b), "hipEventCreate");
    return PT_OK;
}

// Rows [row0, row0 + rows) of the image, one band of a one-frame call; rows = 0: the whole image.
struct RowBand {
    int row0 = 0, rows = 0;
};

// The complete launch record of one batch of call c: its n_frames frames from frame id frame_base,
// over the call's pixels or over one band of the image's rows.
DevLaunch make_launch(const pt_renderer* r, const FrameCall& c, uint32_t frame_base, uint32_t n_frames,
                      RowBand band = {}) {
    DevLaunch L;
    L.width = r->width;
    L.height = r->height;
    L.row0 = 0;
    L.image_height = r->height;
    std::memcpy(L.cam_pos, r->cam_pos, sizeof L.cam_pos);
    std::memcpy(L.inv_view, r->inv_view, sizeof L.inv_view);
    std::memcpy(L.inv_proj, r->inv_proj, sizeof L.inv_proj);
    L.lights = r->d_lights;
    L.n_lights = r->n_lights;
    L.max_bounces = r->max_bounces;
    L.frame_base = frame_base;
    L.n_frames = n_frames;
    L.accum = c.frame_stride ? c.accum + (size_t)(frame_base - c.first) * c.frame_stride : c.accum;
    L.accum64 = c.accum64;
    L.frame_stride = c.frame_stride;
    L.counters = r->d_counters;
    L.debug_pixel = r->d_debug ? r->debug_pixel : -1;
    L.debug_frame = r->debug_frame;
    L.debug = r->d_debug;
    L.lit_tri = r->lit.active ? r->lit.d_tri.get() : nullptr;
    L.lit_bits = r->lit.d_bits;
    L.lit_words = r->lit.words;
    L.occ_tab = r->lit.active && r->occ.active ? r->occ.d_tab.get() : nullptr;
    L.lit_cells = r->lit.cells;
    L.skip_tab = r->skip.active ? r->skip.d_words.get() : nullptr;
    L.pixel_map = nullptr;
    L.n_pixels = r->width * r->height;
    L.adapt_n = nullptr;
    L.adapt_moments = nullptr;
    L.ss_cells = r->filter.buf.cells;  // pt_set_pixel_filter: NULL without supersampling
    L.ss = r->filter.set.supersample;
    L.ss_taps = r->filter.buf.taps;  // NULL for a filter no wider than the box
    L.ss_R = r->filter.R;
    if (c.pixels) {  // a mapped launch: these pixels of the whole image
        L.pixel_map = c.pixels->map;
        L.n_pixels = c.pixels->count;
        L.adapt_n = c.pixels->n;
        L.adapt_moments = c.pixels->moments;
    }
    if (band.rows > 0) {  // rows [row0, row0 + height) of the frame; the sum buffers at the band
        L.row0 = band.row0;
        L.height = band.rows;
        L.n_pixels = L.width * L.height;
        const size_t off = 3 * (size_t)r->width * (size_t)L.row0;
        L.accum += off;
        if (L.accum64) L.accum64 += off;
    }
    return L;
}

}  // namespace

namespace pt {

// Bytes the wavefront queues of all streams hold now.
size_t queue_bytes_held(const pt_renderer* r) {
    size_t b = r->wf.paths() > 0 ? wavefront_bytes(r->wf.paths(), r->wf.max_bounces()) : 0;
    for (int k = 1; k < pt_renderer::kMaxWFStreams; ++k)
        if (r->xwf[k].paths() > 0) b += wavefront_bytes(r->xwf[k].paths(), r->xwf[k].max_bounces());
    return b;
}

// The most bytes all streams' queues may hold together (pt_set_queue_budget): the caller's
// figure, or by default a quarter of the device memory (hipDeviceTotalMem / 4) -- on an MI355X
// above the 56 GB the 128-frame 1080p batch takes on one stream, so the Lambert, Default and
// Layered modes keep it, while two-stream Conductor / Dielectric calls take smaller batches
// (DESIGN.md §5).  SIZE_MAX: no budget.
size_t queue_budget_bytes(const pt_renderer* r) {
    if (r->queue_budget < 0) return SIZE_MAX;
    if (r->queue_budget > 0) return (size_t)r->queue_budget;
    size_t total = 0;
    if (hipDeviceTotalMem(&total, r->device) != hipSuccess || total == 0) {
        (void)hipGetLastError();
        return SIZE_MAX;
    }
    return total / 4;
}

}  // namespace pt

namespace {

constexpr int kMaxWFPaths = 1 << 28;  // 56 GB of queues at 208 B per path

// What plan_wavefront decides for one wavefront call.
struct WFPlan {
    int nf_cap = 1;      // frames per batch
    int ns = 1;          // streams the batches (or the two bands) alternate between
    bool bands = false;  // a one-frame call whose rows may split into two bands
};

// Queues for the plan's ns streams, nf_cap frames each; an allocation that fails for lack of
// memory shrinks the plan (smaller batches on the first stream, fewer streams beyond it).
int reserve_queues(pt_renderer* r, WFPlan* plan, size_t budget, int P) {
    const int maxb = std::max(1, r->max_bounces);
    int& nf_cap = plan->nf_cap;
    for (int k = 0; k < plan->ns; ++k) {
        WFQueues& w = k ? r->xwf[k] : r->wf;
        // queues larger than the budget's share (a lowered budget) are allocated again, smaller
        // (a budget below one frame's queues still allows one frame: no reallocation per call)
        const bool over = budget != SIZE_MAX && w.paths() > P &&
                          (size_t)plan->ns * wavefront_bytes(w.paths(), w.max_bounces()) > budget;
        if (w.paths() < P * nf_cap || w.max_bounces() < r->max_bounces || over) {
            for (int j = 0; j < pt_renderer::kMaxWFStreams; ++j)
                if (r->wf_stream(j)) PT_HIP(hipStreamSynchronize(r->wf_stream(j)), "hipStreamSynchronize");
            w.release();
            hipError_t ae = w.alloc(P * nf_cap, maxb);
            if (ae == hipErrorOutOfMemory && k == 0) {
                // queues of the other streams (an earlier call's, or a mode with more
                // streams) go first, then the full batch again
                bool freed = false;
                for (int j = 1; j < pt_renderer::kMaxWFStreams; ++j)
                    if (r->xwf[j].paths() > 0) {
                        r->xwf[j].release();
                        freed = true;
                    }
                if (freed) ae = w.alloc(P * nf_cap, maxb);
            }
            // the first stream's queues: halve the batch until they fit (every batch size gives
            // the same image), PT_ERR_NOMEM only when one frame does not; the size that fitted
            // stays the cap until the memory would take the full batch (plan_wavefront),
            // pt_set_frames_per_launch or pt_resize
            while (ae == hipErrorOutOfMemory && k == 0 && nf_cap > 1) {
                nf_cap = (nf_cap + 1) / 2;
                r->nf_fit = nf_cap;
                ae = w.alloc(P * nf_cap, maxb);
            }
            // the extra streams only overlap batches: when their queues do not fit, render on
            // the k streams that do (the image is the same, added in frame order either way)
            if (ae == hipErrorOutOfMemory && k > 0) {
                plan->ns = k;
                break;
            }
            PT_HIP(ae, "WFQueues::alloc");
        }
    }
    return PT_OK;
}

// The shape of a wavefront call of n frames: frames per batch, streams, bands, and the queues to
// hold them (reserve_queues).  P: the pixels of a frame of this call -- the image's, or a mapped
// call's (its batches then hold P * frames paths, so fewer pixels mean fewer batches).
int plan_wavefront(pt_renderer* r, uint32_t n, WFPlan* plan, int P, bool mapped) {
    // Frames per wavefront launch chain: the queues hold nf frames' paths (208 B each), at most
    // kMaxWFPaths of them.  Batching amortises launch gaps and the per-kernel SIMT tail:
    // Lambert 1080p 545 / 648 / 664 Msamples/s at 1 / 8 / 16 frames.
    const int maxb = std::max(1, r->max_bounces);
    const int nf_full = std::max(1, std::min({r->frames_per_launch, (int)std::min<uint32_t>(n, 1u << 20),
                                              kMaxWFPaths / std::max(1, P)}));
    // a batch size that fitted after an out-of-memory halving is kept until the free memory
    // (plus what the queues hold now) would take the full batch again
    if (r->nf_fit > 0 && r->nf_fit < nf_full) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            if (free_b + queue_bytes_held(r) >= wavefront_bytes(P * nf_full, maxb)) r->nf_fit = 0;
        } else {
            (void)hipGetLastError();
        }
    }
    int nf_cap = std::min(nf_full, r->nf_fit > 0 ? r->nf_fit : (1 << 30));
    // two batches or more: alternate them between two streams with their own queues, so one
    // batch's kernels run beside the other's (the memory-bound shading of one beside the
    // VALU-bound tracing of the other, and each kernel's SIMT tail filled); k_accum still adds
    // the batches in frame order (accum_wait / accum_done)
    const int nbatch = (int)((n + (uint32_t)nf_cap - 1) / (uint32_t)nf_cap);
    // One frame (pt_render / pt_display_add_frame without render-ahead, the path a viewer that
    // moves the camera every frame gets): its rows split into two bands, one per stream, so
    // each band's kernels fill the other's SIMT tails.  Every pixel's path depends only on its
    // pixel and frame id, so the image is the same bit for bit.
    // A pixel filter wider than the box reads across the band edge: no bands, as for a mapped call.
    const bool bands = n == 1 && r->band_split && r->height >= 16 && !mapped && r->filter.R == 0;  // both bands non-empty
    // auto: a second stream pays where one batch's shading fills the other's trace tails
    // (Conductor +0.6 %, Dielectric +4 % at 128 frames); Lambert, Default and Layered run as
    // fast on one stream with half the queue memory
    const bool two = r->material_mode == PT_MAT_CONDUCTOR || r->material_mode == PT_MAT_DIELECTRIC;
    const int want = r->wf_streams > 0 ? r->wf_streams : (bands || two ? 2 : 1);
    const int ns = std::max(1, std::min(want, bands ? 2 : nbatch));
    // the queue budget (pt_set_queue_budget): the ns streams' queues
    // together stay within it, by smaller batches (every batch size gives the same image);
    // queues that streams beyond ns still hold are freed when they would overrun it
    const size_t budget = queue_budget_bytes(r);
    if (budget != SIZE_MAX) {
        const size_t per_frame = wavefront_bytes(P, maxb);
        const int nf_b = (int)std::max<size_t>(1, budget / ((size_t)ns * per_frame));
        nf_cap = std::min(nf_cap, nf_b);
        size_t used = (size_t)ns * wavefront_bytes(P * nf_cap, maxb);
        for (int k = ns; k < pt_renderer::kMaxWFStreams; ++k) {
            if (r->xwf[k].paths() == 0) continue;
            const size_t held = wavefront_bytes(r->xwf[k].paths(), r->xwf[k].max_bounces());
            if (used + held <= budget) {
                used += held;
                continue;
            }
            PT_HIP(hipStreamSynchronize(r->xstream[k]), "hipStreamSynchronize");
            r->xwf[k].release();
        }
    }
    plan->nf_cap = nf_cap;
    plan->ns = ns;
    plan->bands = bands;
    const int rc = reserve_queues(r, plan, budget, P);
    if (rc != PT_OK) return rc;
    r->last_streams = plan->ns;
    r->last_batch = plan->nf_cap;
    return PT_OK;
}

// The events a call on ns streams (nband row bands) needs besides its launches' pairs, and the
// extra streams themselves.
int fork_resources(pt_renderer* r, int ns, int nband) {
    if (ns > 1) {
        PT_HIP(r->ev_fork.ensure(hipEventDisableTiming), "hipEventCreate");
        for (Event& e : r->ev_accum) PT_HIP(e.ensure(hipEventDisableTiming), "hipEventCreate");
    }
    for (int k = 1; k < ns; ++k)
        if (!r->xstream[k]) {
            PT_HIP(r->xstream[k].create(), "hipStreamCreate");
            PT_HIP(r->ev_join[k].ensure(hipEventDisableTiming), "hipEventCreate");
        }
    if (nband > 1) PT_HIP(r->ev_band0.ensure(hipEventDisableTiming), "hipEventCreate");
    return PT_OK;
}

// The queues of stream sk for one batch; a speculative batch also carries the cancel words.
WFState batch_queues(pt_renderer* r, int sk, bool speculative, bool first_batch) {
    WFState wq = (sk ? r->xwf[sk] : r->wf).state();
    if (speculative && r->ahead.d_cancel_seen) {  // a look-ahead batch: its kernels poll the cancel words
        wq.cancel_host = r->ahead.cancel.d;
        wq.cancel_seen = r->ahead.d_cancel_seen;
        wq.cancel_epoch = r->ahead.cancel_epoch;
        if (r->ahead.debug_hold && r->ahead.hold.d && first_batch) {  // pt_set_debug_hold: k_hold first
            wq.hold_release = r->ahead.hold.d;
            r->ahead.held++;
        }
    }
    return wq;
}

// Enqueue the n frames of a wavefront call in the plan's batches, with their events, bands and
// cancel words.
int enqueue_wavefront(pt_renderer* r, const WFPlan& plan, const FrameCall& c) {
    int rc = PT_OK;
    const DevScene S = r->scene();
    const int ns = plan.ns, nf_cap = plan.nf_cap;
    const bool dual = ns > 1;
    const int nband = plan.bands && ns > 1 ? 2 : 1;  // row bands of a one-frame call
    if ((rc = fork_resources(r, ns, nband)) != PT_OK) return rc;
    int dev_cus = 256;
    (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, r->device);
    if ((rc = lit_prepare(r)) != PT_OK) return rc;  // before the fork: every stream sees the new bits
    if ((rc = skip_prepare(r)) != PT_OK) return rc;  // a table switched on since the scene was built
    hipEvent_t a = nullptr, b = nullptr;  // dual: one event pair around the whole call
    if (dual) {
        rc = next_event_pair(r, &a, &b);
        if (rc) return rc;
        PT_HIP(hipEventRecord(a, r->stream), "hipEventRecord");
        PT_HIP(hipEventRecord(r->ev_fork, r->stream), "hipEventRecord");
        for (int k = 1; k < ns; ++k) PT_HIP(hipStreamWaitEvent(r->xstream[k], r->ev_fork, 0), "hipStreamWaitEvent");
    }
    // band 0 is the smaller one (7/16 of the rows), so it finishes first and pt_render's
    // download of its rows overlaps the rest of band 1
    const int rows0 = r->height * 7 / 16;
    r->band0_rows = nband > 1 ? rows0 : 0;
    WFBatch B;
    B.mode = r->material_mode;
    B.stats = r->trav_stats;
    B.wide_trace = ns == 1 && r->wide_trace;
    B.cus = dev_cus;
    pt_renderer::Timing& t = r->timing;
    if (t.kernel_timing) B.timers = WFTimers{&t.tev, &t.pev, &t.sev};
    int batch = 0;
    for (uint32_t f = 0; f < c.n; ++batch) {  // one event pair per batch (the batch's kernel chain)
        const int nf = (int)std::min<uint32_t>((uint32_t)nf_cap, c.n - f);
        const int band = nband > 1 ? batch : 0;
        RowBand rows;
        if (nband > 1) rows = band == 0 ? RowBand{0, rows0} : RowBand{rows0, r->height - rows0};
        const DevLaunch L = make_launch(r, c, c.first + f, (uint32_t)nf, rows);
        const int sk = batch % ns;  // stream of this batch
        B.stream = r->wf_stream(sk);
        if (!dual) {
            rc = next_event_pair(r, &a, &b);
            if (rc) return rc;
            PT_HIP(hipEventRecord(a, r->stream), "hipEventRecord");
        }
        const WFState wq = batch_queues(r, sk, c.speculative, batch == 0);
        // batches add into the sum in frame order; bands touch disjoint pixels
        B.accum_wait = dual && batch > 0 && nband == 1 ? r->ev_accum[(batch - 1) & 1].e : nullptr;
        B.accum_done = dual && nband == 1 ? r->ev_accum[batch & 1].e : nullptr;
        // with sub-pixel cells the frames of a batch have their own camera rays: no primary dedup
        B.primary_dedup = r->primary_dedup && !L.ss_cells;
        PT_HIP(launch_wavefront_batch(S, L, wq, B), "wavefront launch");
        if (!dual) PT_HIP(hipEventRecord(b, r->stream), "hipEventRecord");
        if (nband > 1 && band == 0) PT_HIP(hipEventRecord(r->ev_band0, B.stream), "hipEventRecord");
        if (band + 1 == nband) f += (uint32_t)nf;
    }
    if (dual) {
        for (int k = 1; k < ns; ++k) {
            PT_HIP(hipEventRecord(r->ev_join[k], r->xstream[k]), "hipEventRecord");
            PT_HIP(hipStreamWaitEvent(r->stream, r->ev_join[k], 0), "hipStreamWaitEvent");
        }
        PT_HIP(hipEventRecord(b, r->stream), "hipEventRecord");
    }
    return PT_OK;
}

// The megakernel: chunks of frames_per_launch frames on the library stream, one event pair each.
int enqueue_megakernel(pt_renderer* r, int kernel, const FrameCall& c) {
    const DevScene S = r->scene();
    const uint32_t chunk = (uint32_t)std::max(1, r->frames_per_launch);
    for (uint32_t done = 0; done < c.n;) {
        uint32_t k = std::min(chunk, c.n - done);
        DevLaunch L = make_launch(r, c, c.first + done, k);
        hipEvent_t a, b;
        const int rc = next_event_pair(r, &a, &b);
        if (rc) return rc;
        PT_HIP(hipEventRecord(a, r->stream), "hipEventRecord");
        PT_HIP(launch_render(kernel, r->material_mode, r->trav_stats, S, L, r->stream), "render launch");
        PT_HIP(hipEventRecord(b, r->stream), "hipEventRecord");
        done += k;
    }
    return PT_OK;
}

// What launch_frames refuses: a destination form or a feature that the resolved kernel has no path for.
int check_call(const pt_renderer* r, const FrameCall& c, int kernel) {
    const bool wavefront = kernel == PT_KERNEL_WAVEFRONT;
    if (c.accum64 && !wavefront)
        return fail(PT_ERR_INVALID, "fp64 accumulation (pt_set_accum_fp64) runs with the wavefront kernel");
    if (c.frame_stride && !wavefront)
        return fail(PT_ERR_INVALID, "per-frame images (render-ahead) run with the wavefront kernel");
    if (c.pixels && (!wavefront || c.accum64 || c.frame_stride))
        return fail(PT_ERR_INVALID, "mapped launches run with the wavefront kernel, into the fp32 sum");
    if (r->filter.active()) {  // pt_set_pixel_filter
        if (!wavefront)
            return fail(PT_ERR_INVALID, "a pixel filter (pt_set_pixel_filter) runs with the wavefront kernel, not the megakernel");
        if (c.pixels && r->filter.R > 0)
            return fail(PT_ERR_INVALID, "mapped launches take no pixel filter wider than the box");
        if (filter_image_too_large(r->filter.set.supersample, r->width, r->height))
            return fail(PT_ERR_INVALID, "pixel filter: supersample^2 * width * height must stay below 2^31");
    }
    return PT_OK;
}

}  // namespace

namespace pt {

// Launch the call's frames in chunks, adding into its destination; brackets with events.  Does not
// wait for earlier work: the event pairs of every launch since the last synchronisation point
// are summed at the next pt_synchronize / pt_get_stats / download (collect_pending).
int launch_frames(pt_renderer* r, const FrameCall& c) {
    int rc = PT_OK;
    // callers that never synchronise through the library (pt_stream interop, device sum buffers,
    // loops over pt_launch / pt_display_add_frame) would grow the event pools without bound:
    // past kMaxPendingEvents pairs, retire them first (this waits for the enqueued work)
    const pt_renderer::Timing& t = r->timing;
    if (t.ev.used + t.tev.used + t.pev.used + t.sev.used > kMaxPendingEvents && (rc = collect_pending(r)) != PT_OK)
        return rc;
    r->timing.pending = true;
    r->band0_rows = 0;  // set by enqueue_wavefront when this call renders its frame in row bands
    r->lit.active = false;  // the wavefront branch decides (lit_prepare)
    r->skip.active = false;  // and skip_prepare
    // AUTO = wavefront: it beats the megakernel in every material mode (1080p
    // depth 8, 16 frames per launch, Msamples/s wavefront / megakernel: Lambert 725 / 414,
    // Dielectric 1239 / 758, Default 255 / 104).
    int kernel = r->kernel;
    if (kernel == PT_KERNEL_AUTO) kernel = PT_KERNEL_WAVEFRONT;
    if ((rc = check_call(r, c, kernel)) != PT_OK) return rc;
    const uint64_t P = c.pixels ? (uint64_t)c.pixels->count : (uint64_t)r->width * (uint64_t)r->height;
    if (kernel == PT_KERNEL_WAVEFRONT) {
        WFPlan plan;
        if ((rc = plan_wavefront(r, c.n, &plan, (int)P, c.pixels != nullptr)) != PT_OK) return rc;
        rc = enqueue_wavefront(r, plan, c);
    } else {
        rc = enqueue_megakernel(r, kernel, c);
    }
    if (rc != PT_OK) return rc;
    r->timing.samples += (uint64_t)c.n * P;
    r->timing.calls++;
    return PT_OK;
}

// Multi-device pt_render_frames: frame ids first .. first+n-1 split into contiguous blocks
// (device g renders first + g*n/N .. , the same split as optixpathtracer_amd/sharding.py), each
// device adding its block in frame order into its own fp32 sum; then one ncclReduce (sum) of
// the N sums onto device 0's accum().  Every sample keeps its (pixel, frame id) seed, so the
// image equals the single-device one up to the fp32 order of the N-way sum.  Each device's work
// and its reduce are enqueued on that device's stream; nothing waits here.
int render_frames_multi(pt_renderer* r, uint32_t first, uint32_t n) {
    const int N = (int)r->multi.comms.size();
    const size_t count = 3 * (size_t)r->width * (size_t)r->height;
    uint32_t f = first;
    for (int g = 0; g < N; ++g) {
        const uint32_t per = n / (uint32_t)N, extra = n % (uint32_t)N;
        const uint32_t ng = per + ((uint32_t)g < extra ? 1u : 0u);
        pt_renderer* d = g == 0 ? r : r->multi.peers[(size_t)g - 1];
        if (ng > 0) {
            PT_HIP(hipSetDevice(d->device), "hipSetDevice");
            FrameCall c;
            c.first = f;
            c.n = ng;
            c.accum = g == 0 ? r->multi.d_part.get() : d->accum();
            if (r->accum64) c.accum64 = g == 0 ? r->multi.d_part64.get() : d->d_accum64.get();
            const int rc = launch_frames(d, c);
            if (rc) return rc;
        }
        f += ng;
    }
    ncclResult_t nr = ncclGroupStart();
    for (int g = 0; g < N && nr == ncclSuccess; ++g) {
        pt_renderer* d = g == 0 ? r : r->multi.peers[(size_t)g - 1];
        if (r->accum64) {  // fp64 partial sums -> fp64 total on device 0
            const double* send = g == 0 ? r->multi.d_part64 : d->d_accum64;
            double* recv = g == 0 ? r->d_accum64 : d->d_accum64;  // significant on the root only
            nr = ncclReduce(send, recv, count, ncclFloat64, ncclSum, 0, r->multi.comms[(size_t)g], d->stream);
        } else {
            const float* send = g == 0 ? r->multi.d_part : d->accum();
            float* recv = g == 0 ? r->accum() : d->accum();  // significant on the root only
            nr = ncclReduce(send, recv, count, ncclFloat32, ncclSum, 0, r->multi.comms[(size_t)g], d->stream);
        }
    }
    const ncclResult_t ne = ncclGroupEnd();
    (void)hipSetDevice(r->device);
    if (nr != ncclSuccess || ne != ncclSuccess)
        return fail(PT_ERR_HIP, std::string("ncclReduce: ") + ncclGetErrorString(nr != ncclSuccess ? nr : ne));
    if (r->accum64) PT_HIP(accum_f64_to_f32(r->d_accum64, r->accum(), count, r->stream), "fp64 -> fp32 sum");
    return PT_OK;
}

}  // namespace pt
