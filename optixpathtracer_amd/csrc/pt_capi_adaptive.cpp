// pt_capi_adaptive.cpp — adaptive sampling (pt_render_adaptive): the rounds, their
// state and what shows it.  A round is a mapped call of launch_frames (pt_capi_launch.cpp) over the
// pixels of the active tiles; the kernels that estimate, compact and resolve are in pt_adaptive.hip.
#include <chrono>

#include "pt_renderer.h"

using namespace pt;

namespace {

constexpr int kAdaptiveKinds = 5;
constexpr int kAdaptiveChannels[kAdaptiveKinds] = {1, 1, 2, 1, 1};
constexpr int kTilePixels = 8;

// Design choices: a 5 % mean relative standard error is where a tile's noise stops
// being visible next to its neighbours'; 16-frame rounds are the shortest that still get the
// bounce-0 visibility table with up to 16 lights (a round's fixed cost is measured in §12); the
// floor keeps unlit pixels from holding a tile.
const pt_adaptive_options kDefaults = {(uint32_t)sizeof(pt_adaptive_options), 0.05f, 16, 1024, 16, 0.01f};

int tiles_of(int pixels) { return (pixels + kTilePixels - 1) / kTilePixels; }

AdaptiveBuffers buffers_of(const pt_renderer* r) {
    const AdaptiveStore& S = r->adaptive.buf;
    AdaptiveBuffers A{};
    A.w = r->width;
    A.h = r->height;
    A.tiles_x = tiles_of(r->width);
    A.tiles_y = tiles_of(r->height);
    A.n = S.n;
    A.moments = S.moments;
    A.err = S.err;
    A.tile_err = S.tile_err;
    A.tile_rounds = S.tile_rounds;
    A.tile_state = S.tile_state;
    A.tile_cnt = S.tile_cnt;
    A.tile_off = S.tile_off;
    A.pixel_map = S.pixel_map;
    A.count = S.count;
    A.scan_tmp = S.scan_tmp.get();
    A.scan_bytes = S.scan_tmp.size();
    return A;
}

// The buffers of the renderer's size, cleared: no samples, every tile active.
int reset_state(pt_renderer* r) {
    AdaptiveStore& S = r->adaptive.buf;
    const size_t pixels = (size_t)r->width * (size_t)r->height;
    const size_t tiles = (size_t)tiles_of(r->width) * (size_t)tiles_of(r->height);
    if (S.pixels() != pixels || S.tiles() != tiles) {
        size_t scan = 0;
        PT_HIP(adaptive_scan_bytes((int)tiles, &scan), "scan size");
        PT_HIP(S.alloc(pixels, tiles, scan), "hipMalloc adaptive state");
    }
    hipStream_t st = r->stream;
    PT_HIP(hipMemsetAsync(S.n, 0, sizeof(uint32_t) * pixels, st), "hipMemset adaptive state");
    PT_HIP(hipMemsetAsync(S.moments, 0, sizeof(double) * 2 * pixels, st), "hipMemset adaptive state");
    PT_HIP(hipMemsetAsync(S.err, 0, sizeof(float) * pixels, st), "hipMemset adaptive state");
    PT_HIP(hipMemsetAsync(S.tile_err, 0, sizeof(float) * tiles, st), "hipMemset adaptive state");
    PT_HIP(hipMemsetAsync(S.tile_rounds, 0, sizeof(int) * tiles, st), "hipMemset adaptive state");
    PT_HIP(hipMemsetD32Async((hipDeviceptr_t)S.tile_state.get(), kTileActive, tiles, st), "hipMemset adaptive state");
    return PT_OK;
}

int round_up(int v, int to) { return (v + to - 1) / to * to; }

}  // namespace

extern "C" {

int pt_adaptive_options_default(pt_adaptive_options* o) {
    if (!o) return fail(PT_ERR_INVALID, "pt_adaptive_options_default: NULL");
    if (!versioned_write(o, kDefaults)) return fail(PT_ERR_INVALID, "pt_adaptive_options_default: struct_size is not set");
    return PT_OK;
}

int pt_render_adaptive(pt_renderer* r, uint32_t first_frame_id, const pt_adaptive_options* opt, float* host_rgb_mean) {
    if (!r) return fail(PT_ERR_INVALID, "pt_render_adaptive: NULL renderer");
    pt_adaptive_options o = kDefaults;
    if (!versioned_merge(o, opt)) return fail(PT_ERR_INVALID, "pt_render_adaptive: options struct_size is not set");
    if (!(o.threshold >= 0.0f)) return fail(PT_ERR_INVALID, "pt_render_adaptive: threshold must be >= 0");
    if (o.round_frames < 2) return fail(PT_ERR_INVALID, "pt_render_adaptive: round_frames must be >= 2");
    if (o.min_samples < 1) return fail(PT_ERR_INVALID, "pt_render_adaptive: min_samples must be >= 1");
    if (o.max_samples < o.min_samples) return fail(PT_ERR_INVALID, "pt_render_adaptive: max_samples must be >= min_samples");
    if (o.round_frames > (1 << 20) || o.max_samples > (1 << 30) - o.round_frames)
        return fail(PT_ERR_INVALID, "pt_render_adaptive: round_frames or max_samples too large");
    if (!(o.luminance_floor > 0.0f)) return fail(PT_ERR_INVALID, "pt_render_adaptive: luminance_floor must be > 0");
    if (r->kernel == PT_KERNEL_MEGA) return fail(PT_ERR_INVALID, "pt_render_adaptive: runs with the wavefront kernel, not the megakernel");
    if (!r->multi.comms.empty()) return fail(PT_ERR_INVALID, "pt_render_adaptive: not on a multi-device renderer");
    if (r->accum64) return fail(PT_ERR_INVALID, "pt_render_adaptive: not with fp64 accumulation (pt_set_accum_fp64)");
    if (r->user_accum) return fail(PT_ERR_INVALID, "pt_render_adaptive: not with a caller-owned accumulation buffer");
    if (r->debug_pixel >= 0) return fail(PT_ERR_INVALID, "pt_render_adaptive: not with a debug pixel set");
    if (r->filter.R > 0) return fail(PT_ERR_INVALID, "pt_render_adaptive: not with a pixel filter wider than the box (pt_set_pixel_filter)");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_render_adaptive: call pt_resize first");
    const int R = o.round_frames;
    const uint32_t min_n = (uint32_t)round_up(o.min_samples, R), max_n = (uint32_t)round_up(o.max_samples, R);
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    cancel_look_ahead(r);  // as a state change: the rounds must not wait behind speculative frames
    pt_renderer::Adaptive& Ad = r->adaptive;
    int rc = pt_accum_clear(r);  // also drops the last call's state
    if (rc) return rc;
    if ((rc = reset_state(r)) != PT_OK) return rc;
    const AdaptiveBuffers A = buffers_of(r);
    PT_HIP(adaptive_compact(A, r->stream), "adaptive compaction kernels");  // round 0: every pixel, in tile order
    Ad.rounds = 0;
    Ad.render_ms = Ad.estimate_ms = 0.0;
    Ad.ev.used = 0;  // pairs a failed call left unrecorded
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t done = 0; done < max_n; done += (uint32_t)R) {
        int active = 0;  // the one word the host reads per round
        PT_HIP(hipMemcpyAsync(&active, A.count, sizeof(int), hipMemcpyDeviceToHost, r->stream), "download active count");
        PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
        if (active <= 0) break;
        const PixelMap pm = {A.pixel_map, active, A.n, A.moments};
        FrameCall c;
        c.first = first_frame_id + done;
        c.n = (uint32_t)R;
        c.accum = r->accum();
        c.pixels = &pm;
        if ((rc = launch_frames(r, c)) != PT_OK) return rc;
        hipEvent_t a = nullptr, b = nullptr;
        PT_HIP(Ad.ev.next(&a, &b), "hipEventCreate");
        PT_HIP(hipEventRecord(a, r->stream), "hipEventRecord");
        PT_HIP(adaptive_estimate(A, o.threshold, min_n, max_n, o.luminance_floor, r->stream), "adaptive estimate kernels");
        PT_HIP(hipEventRecord(b, r->stream), "hipEventRecord");
        Ad.rounds++;
    }
    hipEvent_t a = nullptr, b = nullptr;
    PT_HIP(Ad.ev.next(&a, &b), "hipEventCreate");
    PT_HIP(hipEventRecord(a, r->stream), "hipEventRecord");
    PT_HIP(adaptive_resolve(r->accum(), A.n, Ad.buf.mean, r->width * r->height, r->stream), "adaptive resolve kernel");
    PT_HIP(hipEventRecord(b, r->stream), "hipEventRecord");
    if (host_rgb_mean)
        PT_HIP(hipMemcpyAsync(host_rgb_mean, Ad.buf.mean, sizeof(float) * 3 * (size_t)r->width * (size_t)r->height,
                              hipMemcpyDeviceToHost, r->stream),
               "download mean");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    Ad.render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    size_t pairs = 0;
    PT_HIP(Ad.ev.collect(&Ad.estimate_ms, &pairs), "adaptive events");
    Ad.valid = true;
    return collect_pending(r);
}

int pt_adaptive_channels(int32_t kind) { return kind >= 0 && kind < kAdaptiveKinds ? kAdaptiveChannels[kind] : -1; }

int pt_adaptive_download(pt_renderer* r, int32_t kind, void* host, int64_t bytes) {
    if (!r || !host) return fail(PT_ERR_INVALID, "pt_adaptive_download: NULL");
    if (pt_adaptive_channels(kind) < 0) return fail(PT_ERR_INVALID, "pt_adaptive_download: no such kind");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_adaptive_download: call pt_resize first");
    if (!r->adaptive.valid) return fail(PT_ERR_STATE, "pt_adaptive_download: call pt_render_adaptive first");
    const AdaptiveStore& S = r->adaptive.buf;
    const void* src = nullptr;
    int64_t want = 0;
    switch (kind) {
        case PT_ADAPTIVE_SAMPLES: src = S.n.get(), want = (int64_t)sizeof(uint32_t) * (int64_t)S.pixels(); break;
        case PT_ADAPTIVE_ERROR: src = S.err.get(), want = (int64_t)sizeof(float) * (int64_t)S.pixels(); break;
        case PT_ADAPTIVE_MOMENTS: src = S.moments.get(), want = (int64_t)sizeof(double) * 2 * (int64_t)S.pixels(); break;
        case PT_ADAPTIVE_TILE_ERROR: src = S.tile_err.get(), want = (int64_t)sizeof(float) * (int64_t)S.tiles(); break;
        default: src = S.tile_rounds.get(), want = (int64_t)sizeof(int32_t) * (int64_t)S.tiles(); break;
    }
    if (bytes != want)
        return fail(PT_ERR_INVALID, "pt_adaptive_download: the buffer must hold " + std::to_string(want) + " bytes, not " +
                                        std::to_string(bytes));
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipMemcpyAsync(host, src, (size_t)bytes, hipMemcpyDeviceToHost, r->stream), "download adaptive state");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    return collect_pending(r);
}

float* pt_adaptive_mean_device_ptr(pt_renderer* r) { return r && r->adaptive.valid ? r->adaptive.buf.mean.get() : nullptr; }

int pt_get_adaptive_info(pt_renderer* r, pt_adaptive_info* out) {
    if (!r || !out) return fail(PT_ERR_INVALID, "pt_get_adaptive_info: NULL");
    if (!versioned_bytes(out)) return fail(PT_ERR_INVALID, "pt_get_adaptive_info: struct_size is not set");
    pt_adaptive_info d{};
    d.tiles = tiles_of(r->width) * tiles_of(r->height);
    const pt_renderer::Adaptive& Ad = r->adaptive;
    if (Ad.valid) {
        PT_HIP(hipSetDevice(r->device), "hipSetDevice");
        std::vector<uint32_t> n(Ad.buf.pixels());
        std::vector<int> state(Ad.buf.tiles());
        PT_HIP(hipMemcpyAsync(n.data(), Ad.buf.n, sizeof(uint32_t) * n.size(), hipMemcpyDeviceToHost, r->stream), "download counts");
        PT_HIP(hipMemcpyAsync(state.data(), Ad.buf.tile_state, sizeof(int) * state.size(), hipMemcpyDeviceToHost, r->stream),
               "download tile states");
        PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
        uint32_t most = 0;
        for (uint32_t v : n) d.samples += v, most = std::max(most, v);
        d.samples_uniform = (uint64_t)n.size() * (uint64_t)most;
        for (int s : state) d.tiles_stopped += s == kTileStopped ? 1 : 0;
        d.rounds = Ad.rounds;
        d.render_ms = Ad.render_ms;
        d.estimate_ms = Ad.estimate_ms;
    }
    versioned_write(out, d);
    return PT_OK;
}

}  // extern "C"
