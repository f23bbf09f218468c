// pt_capi_ahead.cpp — render-ahead: the render key, the ring of 1-spp images, look-ahead cancellation.
#include "pt_renderer.h"

using namespace pt;

namespace pt {

// Everything a 1-spp image depends on besides its frame id (the geometry by its commit count).
static RenderKey render_key(const pt_renderer* r) {
    RenderKey k;
    k.w = r->width;
    k.h = r->height;
    k.n_lights = r->n_lights;
    k.max_bounces = r->max_bounces;
    k.mode = r->material_mode;
    k.kernel = r->kernel;
    k.debug_pixel = r->d_debug ? r->debug_pixel : -1;
    k.debug_frame = r->debug_frame;
    k.lights_version = r->lights_version;
    k.debug_version = r->debug_version;
    k.geom_version = r->geom.version;
    k.filter_version = r->filter.version;
    k.lights = r->d_lights;
    std::memcpy(k.cam, r->cam_pos, sizeof r->cam_pos);
    std::memcpy(k.cam + 3, r->inv_view, sizeof r->inv_view);
    std::memcpy(k.cam + 19, r->inv_proj, sizeof r->inv_proj);
    return k;
}

// The render key's share that a first hit depends on: size, camera and committed geometry.
ViewKey view_key(const pt_renderer* r) {
    const RenderKey k = render_key(r);
    ViewKey v;
    v.w = k.w;
    v.h = k.h;
    v.geom_version = k.geom_version;
    std::memcpy(v.cam, k.cam, sizeof v.cam);
    return v;
}

void ring_free(pt_renderer* r) {
    for (RingSlot& s : r->ahead.ring) {
        s.d.reset();  // hipFree waits for the work that may still read it
        s.n = 0;
        s.measured = true;
        s.speculative = false;
        s.served = false;
    }
    r->ahead.ring_k = 1;
    r->ahead.oom_cap = 1 << 30;
}

// Frames one render-ahead batch may hold now.  Memory: the batch's wavefront queues (one stream)
// and both ring slots take at most a quarter of the device memory, and no more than is free
// besides what the renderer already holds for them (render-ahead sized its queues
// like pt_render_frames, 28 GB at 1080p).  Time: the batch's estimated duration stays within
// ahead_budget_ms, from the per-frame time of the last measured ring batch (a call that changes
// the state waits behind at most the batch in flight).  Always >= 1.
static int ahead_frames(pt_renderer* r, size_t n3, bool by_time) {
    int k = std::min(r->ahead.max_frames, r->ahead.oom_cap);
    const size_t P = n3 / 3;
    const size_t per_frame = wavefront_bytes((int)P, std::max(1, r->max_bounces)) + 2 * sizeof(float) * n3;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) {
        size_t held = 2 * sizeof(float) * n3 * (size_t)std::max(r->ahead.ring[0].cap(n3), r->ahead.ring[1].cap(n3));
        if (r->wf.paths() > 0) held += wavefront_bytes(r->wf.paths(), r->wf.max_bounces());
        const size_t avail = std::min(total_b / 4, free_b + held);
        k = std::min<size_t>((size_t)k, std::max<size_t>(1, avail / per_frame));
    } else {
        (void)hipGetLastError();
    }
    if (by_time && r->ahead.budget_ms > 0.0 && r->ahead.frame_ms_est > 0.0)
        k = std::min(k, std::max(1, (int)(r->ahead.budget_ms / r->ahead.frame_ms_est)));
    return std::max(1, k);
}

// A finished ring batch's duration per frame -> frame_ms_est (no wait: only batches done by now).
static void ring_measure(pt_renderer* r) {
    for (RingSlot& sl : r->ahead.ring) {
        if (sl.measured || sl.n == 0 || hipEventQuery(sl.ready) != hipSuccess) continue;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, sl.start, sl.ready) == hipSuccess && ms > 0.0f) r->ahead.frame_ms_est = ms / sl.n;
        (void)hipGetLastError();
        sl.measured = true;
    }
}

// Slot s of the ring with room for `cap` frames and its events.
static int ring_reserve(pt_renderer* r, int s, int cap, size_t n3) {
    RingSlot& sl = r->ahead.ring[s];
    PT_HIP(sl.ready.ensure(), "hipEventCreate");
    PT_HIP(sl.start.ensure(), "hipEventCreate");
    if (cap <= sl.cap(n3)) return PT_OK;
    if (sl.d) PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");  // before the old frames go
    PT_HIP(sl.d.alloc(n3 * (size_t)cap), "hipMalloc render-ahead ring");
    return PT_OK;
}

// The cancel words of the look-ahead batches (allocated at the first one; false if they cannot
// be, and the batch is then enqueued without them).
static bool cancel_words(pt_renderer* r) {
    if (r->ahead.d_cancel_seen) return true;
    pt_renderer::Ahead& A = r->ahead;
    if (A.cancel.alloc(0) != hipSuccess || A.cancel.map() != hipSuccess || A.d_cancel_seen.alloc(1) != hipSuccess ||
        hipMemsetAsync(A.d_cancel_seen, 0, sizeof(unsigned), r->stream) != hipSuccess) {
        (void)hipGetLastError();
        A.cancel.reset();
        A.d_cancel_seen.reset();
        return false;
    }
    A.cancel_epoch = 0;
    return true;
}

// Render frames [first, first + n) into ring slot s (room for `cap` frames) as 1-spp images and
// record its events.  `speculative`: the look-ahead batch, which cancel_look_ahead can stop.
static int ring_fill(pt_renderer* r, int s, const RenderKey& k, uint32_t first, int n, int cap, size_t n3,
              bool speculative = false) {
    RingSlot& sl = r->ahead.ring[s];
    sl.n = 0;
    sl.measured = true;
    sl.served = false;
    sl.speculative = speculative && cancel_words(r);
    int rc = ring_reserve(r, s, std::max(n, cap), n3);
    if (rc == PT_OK) PT_HIP(hipEventRecord(sl.start, r->stream), "hipEventRecord");
    FrameCall c;  // every frame its own image of the slot
    c.first = first;
    c.n = (uint32_t)n;
    c.accum = sl.d;
    c.frame_stride = n3;
    c.speculative = sl.speculative;
    if (rc == PT_OK) rc = launch_frames(r, c);
    if (rc != PT_OK) return rc;
    PT_HIP(hipEventRecord(sl.ready, r->stream), "hipEventRecord");
    sl.key = k;
    sl.first = first;
    sl.n = (uint32_t)n;
    sl.measured = false;
    r->ahead.rendered += (uint64_t)n;
    return PT_OK;
}

// Cancel the look-ahead batch in flight.  The reference renders one
// frame per Render() call (OptixRenderer.cpp:617-647) and its viewer moves the camera between
// calls (OptixView.cpp:133-139); frames pt_render rendered ahead under the old state are then
// useless, and the next call would wait behind up to ahead_budget_ms of them.  When the state
// no longer matches the speculative slot (or `force`: the caller is about to change it, and
// waits on the library stream first), a newer epoch is published in the pinned host word: the
// batch's kernels see it within about a trace kernel's poll interval and stop
// (pt_wavefront.hip wf_cancel_poll), the rest of its launches drain as no-ops, and the slot
// is discarded.  A batch that already finished is kept.
void cancel_look_ahead(pt_renderer* r, bool force) {
    if (!r->ahead.spec_pending || !r->ahead.cancel.h) return;
    RingSlot& sl = r->ahead.ring[r->ahead.ring_last];
    if (sl.n == 0 || !sl.speculative) return;  // not speculative: also a batch a call took a frame from
    if (!force && sl.key == render_key(r)) return;
    if (hipEventQuery(sl.ready) == hipSuccess) return;  // done: its frames stay valid for their state
    (void)hipGetLastError();                            // hipErrorNotReady
    // The epoch stops every batch enqueued under an older one: a served batch still in flight
    // (the other slot, enqueued earlier on the same stream) finishes first
    RingSlot& other = r->ahead.ring[r->ahead.ring_last ^ 1];
    if (other.served && other.n > 0 && hipEventQuery(other.ready) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipEventSynchronize(other.ready);
    }
    ++r->ahead.cancel_epoch;
    __atomic_store_n(r->ahead.cancel.h, r->ahead.cancel_epoch, __ATOMIC_SEQ_CST);
    sl.n = 0;
    sl.speculative = false;
    r->ahead.cancelled++;
}

// The 1-spp image of frame r->frame_id for pt_render / pt_display_add_frame (OptixRenderer::Render,
// OptixRenderer.cpp:617-647), enqueued on r->stream; *ready (if given) is an event after which the
// image may be read from another stream.  With render-ahead (wavefront kernel), a frame a ring
// slot holds under the same render state is taken from it; a miss renders the next k frames as one
// batch into a slot, k doubling on every miss that continues the ring's frame sequence under the
// same state (up to ahead_frames: render_ahead, the memory cap and the time budget) and 1
// otherwise, so an interactive caller that changes the camera every frame pays for one frame per
// call.  With `look_ahead` (pt_render, whose downloads run on dl_stream), the first call served
// from a slot of the full ramp length also enqueues the following frames into the other slot,
// which the GPU renders while the caller downloads this slot's frames.  Each ring image is the
// one-frame sum into zeros that the plain path computes, bit for bit.  The debug pixel's records
// belong to the call that renders its frame, so with a debug pixel set every call renders its
// own frame.
int render_frame_image(pt_renderer* r, const float** img, hipEvent_t* ready, bool look_ahead, hipEvent_t* part_ready,
                       size_t* part_floats) {
    const size_t n3 = 3 * (size_t)r->width * (size_t)r->height;
    const int kernel = r->kernel == PT_KERNEL_AUTO ? PT_KERNEL_WAVEFRONT : r->kernel;
    const uint32_t f = r->frame_id;
    const bool debug = r->d_debug && r->debug_pixel >= 0;
    cancel_look_ahead(r);  // a state change since the look-ahead batch: stop it (also with render-ahead now off)
    if (r->ahead.max_frames > 1 && kernel == PT_KERNEL_WAVEFRONT && !debug) {
        ring_measure(r);
        const RenderKey k = render_key(r);
        int s = -1;
        bool seq = false;
        for (int i = 0; i < 2; ++i) {
            const RingSlot& sl = r->ahead.ring[i];
            if (sl.n == 0 || !(k == sl.key)) continue;
            if (f - sl.first < sl.n) s = i;  // unsigned: also false for f < first
            if (i == r->ahead.ring_last && f == sl.first + sl.n) seq = true;
        }
        int rc = PT_OK;
        if (s < 0) {  // miss: the next k frames into the slot not rendered last
            if (!seq) r->ahead.oom_cap = 1 << 30;  // a new sequence tries the full length again
            const int kmax = ahead_frames(r, n3, false);
            const int kf = seq ? std::min(2 * r->ahead.ring_k, ahead_frames(r, n3, true)) : 1;
            s = r->ahead.ring_last ^ 1;
            rc = ring_fill(r, s, k, f, kf, kf == 1 ? 1 : kmax, n3);
            if (rc == PT_OK) {
                r->ahead.ring_k = kf;
                r->ahead.ring_last = s;
            } else if (rc == PT_ERR_NOMEM) {
                // no room for this batch: later batches of the sequence stay below it, and this
                // call renders its own frame alone (below)
                r->ahead.oom_cap = std::max(1, kf / 2);
                r->ahead.ring[s].n = 0;
            }
        }
        if (rc == PT_OK) {
            RingSlot& sl = r->ahead.ring[s];
            // A frame handed out of a speculative batch may be read by work the caller has
            // already queued behind it (pt_display_add_frame's blend does not wait for the
            // batch): the batch is no longer cancellable
            if (sl.speculative) {
                sl.speculative = false;
                sl.served = true;
            }
            *img = sl.d + (size_t)(f - sl.first) * n3;
            if (ready) *ready = sl.ready;
            r->ahead.served++;
            const int o = s ^ 1;
            const uint32_t next = sl.first + sl.n;
            // the ramp is done once doubling this slot's length would pass the target length (the
            // length, a device-memory query, only for a call that may enqueue: ADVICE round 4)
            const bool may_look = look_ahead && f == sl.first && sl.n > 1 &&
                                  !(r->ahead.ring[o].n > 0 && r->ahead.ring[o].key == k && r->ahead.ring[o].first == next);
            const int kl = may_look ? ahead_frames(r, n3, true) : 0;  // the full ramp length now
            if (may_look && 2 * (int)sl.n > kl) {
                const int lrc = ring_fill(r, o, k, next, kl, ahead_frames(r, n3, false), n3, true);
                if (lrc == PT_OK) {
                    r->ahead.ring_k = kl;
                    r->ahead.ring_last = o;
                    r->ahead.spec_pending = true;
                } else if (lrc != PT_ERR_NOMEM) {
                    return lrc;
                } else {
                    r->ahead.ring[o].n = 0;
                }  // no room for the second slot: this call's frame is served all the same
            }
            return PT_OK;
        }
        if (rc != PT_ERR_NOMEM) return rc;
    }
    PT_HIP(hipMemsetAsync(r->d_frame, 0, sizeof(float) * n3, r->stream), "hipMemset frame");
    FrameCall c;
    c.first = f;
    c.n = 1;
    c.accum = r->d_frame;
    const int rc = launch_frames(r, c);
    if (rc) return rc;
    *img = r->d_frame;
    if (part_ready && r->band0_rows > 0) {  // the first band's rows are final once ev_band0 passes
        *part_ready = r->ev_band0;
        *part_floats = 3 * (size_t)r->width * (size_t)r->band0_rows;
    }
    if (ready) {
        PT_HIP(r->ev_frame.ensure(hipEventDisableTiming), "hipEventCreate");
        PT_HIP(hipEventRecord(r->ev_frame, r->stream), "hipEventRecord");
        *ready = r->ev_frame;
    }
    return PT_OK;
}

}  // namespace pt
