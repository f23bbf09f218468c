// pt_capi_temporal.cpp — pt_denoise_temporal and its state: the history that one call leaves for
// the next, the launches of DESIGN.md §11 and the entry points.  The kernels are in pt_temporal.hip;
// the G-buffer, the pack pass and the scratch colour buffers are pt_denoise's (pt_capi_denoise.cpp).
// Motion vectors (pt_temporal_options.motion_vectors, pt_motion_*): the vertex snapshot and the rule
// for when the motion kernel runs are here too.
#include "pt_renderer.h"

using namespace pt;

namespace {

constexpr int kTemporalKinds = 4;
constexpr int kTemporalChannels[kTemporalKinds] = {1, 2, 1, 3};
constexpr int kMotionKinds = 3;
constexpr int kMotionChannels[kMotionKinds] = {2, 3, 3};

const pt_temporal_options kTemporalDefaults = {(uint32_t)sizeof(pt_temporal_options), 0.2f, 0.2f, 32, 0.9f, 0.02f, 4.0f, 4, 0};

// The history buffers; the scratch colour and result buffers are DenoiseCall::begin's.
int alloc_temporal(pt_renderer* r, size_t n, bool motion) {
    pt_renderer::Temporal& T = r->temporal;
    if (T.d_tc.size() != n) {
        T.valid = false;
        for (DevBuf<float4>* b : {&T.d_pgn, &T.d_pgp, &T.d_hc, &T.d_m[0], &T.d_m[1]}) PT_HIP(b->alloc(n), "hipMalloc history");
        PT_HIP(T.d_den.alloc(n), "hipMalloc history");
        PT_HIP(T.d_tc.alloc(n), "hipMalloc history");  // last: its size says that all of them exist
    }
    if (!T.d_count) PT_HIP(T.d_count.alloc(3), "hipMalloc history");
    if (motion) {
        const size_t ns = 3 * (size_t)std::max(1, r->ntri);
        if (T.d_snap.size() != ns) {
            T.snap_have = T.snap_prev = false;
            PT_HIP(T.d_snap.alloc(ns), "hipMalloc vertex snapshot");
        }
        if (T.d_pp.size() != n) PT_HIP(T.d_pp.alloc(n), "hipMalloc previous positions");
        for (Event& e : T.ev_s) PT_HIP(e.ensure(), "hipEventCreate");
    }
    for (Event& e : T.ev) PT_HIP(e.ensure(), "hipEventCreate");
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_temporal_options_default(pt_temporal_options* o) {
    if (!o) return fail(PT_ERR_INVALID, "pt_temporal_options_default: NULL");
    if (!versioned_write(o, kTemporalDefaults))
        return fail(PT_ERR_INVALID, "pt_temporal_options_default: struct_size is not set");
    return PT_OK;
}

int pt_denoise_temporal(pt_renderer* r, int32_t source, const float* host_in, float scale, const pt_temporal_options* topt,
                        const pt_denoise_options* dopt, float* host_out) {
    DenoiseCall c{"pt_denoise_temporal", r, source, host_in};
    int rc = c.check_source();
    if (rc) return rc;
    pt_temporal_options t = kTemporalDefaults;
    if (!versioned_merge(t, topt))
        return fail(PT_ERR_INVALID, "pt_denoise_temporal: temporal options struct_size is not set");
    rc = c.merge(dopt);
    if (rc) return rc;
    if (!(t.alpha > 0.0f && t.alpha <= 1.0f) || !(t.alpha_moments > 0.0f && t.alpha_moments <= 1.0f))
        return fail(PT_ERR_INVALID, "pt_denoise_temporal: alpha and alpha_moments must be in (0, 1]");
    if (t.max_history < 1) return fail(PT_ERR_INVALID, "pt_denoise_temporal: max_history must be >= 1");
    if (!(t.normal_cos >= -1.0f && t.normal_cos <= 1.0f))
        return fail(PT_ERR_INVALID, "pt_denoise_temporal: normal_cos must be in [-1, 1]");
    if (!(t.plane_distance > 0.0f)) return fail(PT_ERR_INVALID, "pt_denoise_temporal: plane_distance must be > 0");
    if (!(t.sigma_luminance > 0.0f)) return fail(PT_ERR_INVALID, "pt_denoise_temporal: sigma_luminance must be > 0");
    if (t.variance_history < 0) return fail(PT_ERR_INVALID, "pt_denoise_temporal: variance_history must be >= 0");
    rc = c.begin(false);  // sigma_color is not read
    if (rc) return rc;
    pt_renderer::Aov& A = r->aov;
    pt_renderer::Temporal& T = r->temporal;
    const pt_denoise_options& o = c.o;
    AtrousParams& P = c.P;
    const size_t n = c.n;
    const bool motion = t.motion_vectors != 0;
    rc = alloc_temporal(r, n, motion);
    if (rc) {
        T.release();
        return rc;
    }
    const int prev = T.cur, cur = T.cur ^ 1;

    TemporalParams K{};
    K.c = A.d_c[0];
    K.gn = A.d_gn;
    K.gp = A.d_gp;
    K.pgn = T.d_pgn;
    K.pgp = T.d_pgp;
    K.hc = T.d_hc;
    K.hm = T.d_m[prev];
    K.tc = T.d_tc;
    K.tm = T.d_m[cur];
    K.count = T.d_count;
    K.w = r->width;
    K.h = r->height;
    K.history = T.valid ? 1 : 0;
    if (T.valid) {
        mat4_inverse(T.inv_view, K.prev_view);
        mat4_inverse(T.inv_proj, K.prev_proj);
    }
    K.alpha = t.alpha;
    K.alpha_moments = t.alpha_moments;
    K.max_history = (float)t.max_history;
    K.normal_cos = t.normal_cos;
    K.plane_distance = t.plane_distance;
    // the motion kernel: only where the snapshot shows the previous call's geometry and that is not the
    // present one (for unchanged vertices it computes what the plain kernel does, bit for bit)
    const bool use_motion = motion && T.valid && T.snap_have && T.snap_prev && T.snap_version != r->geom.version;
    K.gb = A.d_gb;
    K.snap = T.d_snap;
    K.pp = T.d_pp;
    K.ntri = r->ntri;
    const bool had_history = T.valid;

    T.valid = false;  // until every launch below is enqueued
    T.snap_prev = T.mv_last = T.mv_used = T.snap_timed = false;
    PT_HIP(hipMemsetAsync(T.d_count, 0, 3 * sizeof(unsigned long long), r->stream), "hipMemset history counters");
    PT_HIP(hipEventRecord(T.ev[0], r->stream), "hipEventRecord");
    PT_HIP(atrous_pack(c.src, scale, P.demodulate != 0, P.floor, P.gn, P.ga, A.d_c[0], n, r->stream), "filter pack kernel");
    PT_HIP(temporal_blend(K, use_motion, r->stream), "temporal kernel");
    PT_HIP(hipEventRecord(T.ev[1], r->stream), "hipEventRecord");
    if (t.variance_history > 1)  // a history is at least 1 long: nothing is shorter than 0 or 1
        PT_HIP(temporal_variance(P.gn, P.gp, T.d_m[cur], T.d_tc, P.w, P.h, P.inv_n, P.inv_p, (float)t.variance_history,
                                 r->stream),
               "temporal variance kernel");
    PT_HIP(hipEventRecord(T.ev[2], r->stream), "hipEventRecord");
    // iteration 0: d_tc -> d_hc (the history itself); then d_hc -> d_c[0] -> d_c[1] -> d_c[0] ...
    for (int i = 0; i < o.iterations; ++i) {
        const bool last = i == o.iterations - 1;
        P.step = 1 << i;
        P.cin = i == 0 ? T.d_tc.get() : i == 1 ? T.d_hc.get() : A.d_c[i & 1].get();
        P.cout = i == 0 ? T.d_hc.get() : A.d_c[(i & 1) ^ 1].get();
        PT_HIP(temporal_luminance_scale(P.cin, P.gn, T.d_den, P.w, P.h, t.sigma_luminance, r->stream), "filter divisor kernel");
        PT_HIP(temporal_atrous_iteration(P, T.d_den, i == 0 && last ? T.d_hc.get() : nullptr, last, c.lds, r->stream),
               "temporal filter kernel");
    }
    // this view's guides are the next call's previous ones (the cached G-buffer stays as it is)
    PT_HIP(hipMemcpyAsync(T.d_pgn, A.d_gn, sizeof(float4) * n, hipMemcpyDeviceToDevice, r->stream), "keep guides");
    PT_HIP(hipMemcpyAsync(T.d_pgp, A.d_gp, sizeof(float4) * n, hipMemcpyDeviceToDevice, r->stream), "keep guides");
    PT_HIP(hipEventRecord(T.ev[3], r->stream), "hipEventRecord");
    if (motion) {  // the snapshot follows the kernel that read it, and shows this call's geometry from here on
        if (!T.snap_have || T.snap_version != r->geom.version) {
            PT_HIP(hipEventRecord(T.ev_s[0], r->stream), "hipEventRecord");
            PT_HIP(temporal_snapshot(r->d_isect, r->d_shade, r->ntri, T.d_snap, r->stream), "snapshot kernel");
            PT_HIP(hipEventRecord(T.ev_s[1], r->stream), "hipEventRecord");
            T.snap_timed = true;
            T.snap_version = r->geom.version;
            T.snap_have = true;
        }
        T.snap_prev = T.mv_last = true;
        T.mv_used = use_motion;
    }
    T.had_history = had_history;
    std::memcpy(T.prev_view, K.prev_view, sizeof T.prev_view);
    std::memcpy(T.prev_proj, K.prev_proj, sizeof T.prev_proj);
    std::memcpy(T.inv_view, r->inv_view, sizeof T.inv_view);
    std::memcpy(T.inv_proj, r->inv_proj, sizeof T.inv_proj);
    T.cur = cur;
    T.valid = true;
    T.timed = true;
    T.calls++;
    return c.finish(host_out);
}

int pt_temporal_reset(pt_renderer* r) {
    if (!r) return fail(PT_ERR_INVALID, "pt_temporal_reset: NULL renderer");
    r->temporal.valid = false;
    return PT_OK;
}

int pt_temporal_channels(int32_t kind) { return kind >= 0 && kind < kTemporalKinds ? kTemporalChannels[kind] : -1; }

int pt_temporal_download(pt_renderer* r, int32_t kind, void* host, int64_t bytes) {
    if (!r || !host) return fail(PT_ERR_INVALID, "pt_temporal_download: NULL");
    const int ch = pt_temporal_channels(kind);
    if (ch < 0) return fail(PT_ERR_INVALID, "pt_temporal_download: no such kind");
    pt_renderer::Temporal& T = r->temporal;
    if (!T.timed || T.d_tc.size() == 0) return fail(PT_ERR_STATE, "pt_temporal_download: call pt_denoise_temporal first");
    const size_t n = T.d_tc.size();
    const int64_t want = 4 * (int64_t)ch * (int64_t)n;
    if (bytes != want)
        return fail(PT_ERR_INVALID, "pt_temporal_download: the buffer must hold " + std::to_string(want) + " bytes, not " +
                                        std::to_string(bytes));
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    const float4* src = kind == PT_TEMPORAL_VARIANCE ? T.d_tc.get() : kind == PT_TEMPORAL_COLOR ? T.d_hc.get() : T.d_m[T.cur].get();
    std::vector<float4> rec(n);
    PT_HIP(hipMemcpyAsync(rec.data(), src, sizeof(float4) * n, hipMemcpyDeviceToHost, r->stream), "download history");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    float* out = static_cast<float*>(host);
    for (size_t i = 0; i < n; ++i) {
        const float4 v = rec[i];
        switch (kind) {
            case PT_TEMPORAL_HISTORY_LENGTH: out[i] = v.z; break;
            case PT_TEMPORAL_MOMENTS: out[2 * i] = v.x, out[2 * i + 1] = v.y; break;
            case PT_TEMPORAL_VARIANCE: out[i] = v.w; break;
            default: out[3 * i] = v.x, out[3 * i + 1] = v.y, out[3 * i + 2] = v.z; break;
        }
    }
    return collect_pending(r);
}

int pt_motion_channels(int32_t kind) { return kind >= 0 && kind < kMotionKinds ? kMotionChannels[kind] : -1; }

int pt_motion_download(pt_renderer* r, int32_t kind, void* host, int64_t bytes) {
    if (!r || !host) return fail(PT_ERR_INVALID, "pt_motion_download: NULL");
    const int ch = pt_motion_channels(kind);
    if (ch < 0) return fail(PT_ERR_INVALID, "pt_motion_download: no such kind");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_motion_download: call pt_resize first");
    pt_renderer::Temporal& T = r->temporal;
    if (kind != PT_MOTION_BARYCENTRIC && !(T.timed && T.mv_last && T.d_tc.size() != 0))
        return fail(PT_ERR_STATE, "pt_motion_download: the last pt_denoise_temporal did not have motion_vectors on");
    const size_t n = (size_t)r->width * (size_t)r->height;
    const int64_t want = 4 * (int64_t)ch * (int64_t)n;
    if (bytes != want)
        return fail(PT_ERR_INVALID, "pt_motion_download: the buffer must hold " + std::to_string(want) + " bytes, not " +
                                        std::to_string(bytes));
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    float* out = static_cast<float*>(host);
    // the previous positions of the last call: what the motion kernel wrote, or that call's position guide
    const float4* pp = T.mv_used ? T.d_pp.get() : T.d_pgp.get();
    if (kind == PT_MOTION_SCREEN) {
        DevBuf<float> d_out;
        PT_HIP(d_out.alloc(3 * n), "hipMalloc screen motion");
        PT_HIP(temporal_motion_screen(pp, T.d_pgn, T.prev_view, T.prev_proj, T.had_history ? 1 : 0, r->width, r->height,
                                      d_out, r->stream),
               "screen motion kernel");
        PT_HIP(hipMemcpyAsync(out, d_out, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, r->stream), "download screen motion");
        PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
        return collect_pending(r);
    }
    if (kind == PT_MOTION_BARYCENTRIC) {
        const int rc = gbuffer_prepare(r);
        if (rc) return rc;
        pp = r->aov.d_gb;
    }
    std::vector<float4> rec(n);
    PT_HIP(hipMemcpyAsync(rec.data(), pp, sizeof(float4) * n, hipMemcpyDeviceToHost, r->stream), "download motion");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    for (size_t i = 0; i < n; ++i) {
        const float4 v = rec[i];
        if (kind == PT_MOTION_BARYCENTRIC) out[2 * i] = v.x, out[2 * i + 1] = v.y;
        else out[3 * i] = v.x, out[3 * i + 1] = v.y, out[3 * i + 2] = v.z;
    }
    return collect_pending(r);
}

int pt_get_temporal_info(pt_renderer* r, pt_temporal_info* out) {
    if (!r || !out) return fail(PT_ERR_INVALID, "pt_get_temporal_info: NULL");
    if (!versioned_bytes(out)) return fail(PT_ERR_INVALID, "pt_get_temporal_info: struct_size is not set");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    pt_renderer::Temporal& T = r->temporal;
    pt_temporal_info d{};
    d.history_valid = T.valid ? 1 : 0;
    d.calls = T.calls;
    if (T.timed) {
        float ms = 0.0f;
        PT_HIP(hipEventElapsedTime(&ms, T.ev[0], T.ev[1]), "temporal events");
        d.temporal_ms = ms;
        PT_HIP(hipEventElapsedTime(&ms, T.ev[1], T.ev[2]), "temporal events");
        d.variance_ms = ms;
        PT_HIP(hipEventElapsedTime(&ms, T.ev[2], T.ev[3]), "temporal events");
        d.filter_ms = ms;
        unsigned long long c[3] = {0, 0, 0};
        PT_HIP(hipMemcpy(c, T.d_count, sizeof c, hipMemcpyDeviceToHost), "download history counters");
        d.reprojected_pixels = c[0];
        d.reset_pixels = c[1];
        d.moved_pixels = c[2];
        d.motion_used = T.mv_used ? 1 : 0;
        if (T.snap_timed) {
            PT_HIP(hipEventElapsedTime(&ms, T.ev_s[0], T.ev_s[1]), "snapshot events");
            d.snapshot_ms = ms;
        }
    }
    versioned_write(out, d);
    return collect_pending(r);
}

}  // extern "C"
