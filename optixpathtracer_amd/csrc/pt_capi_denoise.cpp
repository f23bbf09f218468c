// pt_capi_denoise.cpp — first-hit feature buffers (pt_aov_*) and the a-trous denoiser (pt_denoise):
// the G-buffer cache, the filter's launches and the entry points, and DenoiseCall, the checks and set-up
// that pt_denoise shares with pt_denoise_temporal.  The kernels are in pt_aov.hip and pt_atrous.h.
#include "pt_renderer.h"

using namespace pt;

namespace {

constexpr int kAovKinds = 7;
constexpr int kAovChannels[kAovKinds] = {3, 3, 3, 3, 1, 1, 2};

const pt_denoise_options kDefaults = {(uint32_t)sizeof(pt_denoise_options), 5, 1, 1.0f, 0.3f, 1.0f, 1e-3f};

void* aov_ptr(pt_renderer* r, int kind) {
    pt_renderer::Aov& A = r->aov;
    switch (kind) {
        case PT_AOV_ALBEDO: return A.d_albedo.get();
        case PT_AOV_NORMAL: return A.d_normal.get();
        case PT_AOV_GEOM_NORMAL: return A.d_gnormal.get();
        case PT_AOV_POSITION: return A.d_position.get();
        case PT_AOV_DEPTH: return A.d_depth.get();
        case PT_AOV_PRIM: return A.d_prim.get();
        case PT_AOV_ROUGH_METAL: return A.d_rough_metal.get();
        default: return nullptr;
    }
}

int alloc_gbuffer(pt_renderer* r, size_t n) {
    pt_renderer::Aov& A = r->aov;
    if (A.d_gn.size() == n) return PT_OK;
    for (DevBuf<float>* b : {&A.d_albedo, &A.d_normal, &A.d_gnormal, &A.d_position})
        PT_HIP(b->alloc(3 * n), "hipMalloc G-buffer");
    PT_HIP(A.d_depth.alloc(n), "hipMalloc G-buffer");
    PT_HIP(A.d_rough_metal.alloc(2 * n), "hipMalloc G-buffer");
    PT_HIP(A.d_prim.alloc(n), "hipMalloc G-buffer");
    PT_HIP(A.d_ga.alloc(n), "hipMalloc G-buffer");
    PT_HIP(A.d_gp.alloc(n), "hipMalloc G-buffer");
    PT_HIP(A.d_gb.alloc(n), "hipMalloc G-buffer");
    if (!A.d_hits) PT_HIP(A.d_hits.alloc(1), "hipMalloc G-buffer");
    PT_HIP(A.d_gn.alloc(n), "hipMalloc G-buffer");  // last: its size says that all of them exist
    return PT_OK;
}

}  // namespace

namespace pt {

// The G-buffer of the renderer's present view, rendered on r->stream unless the cached one is of
// the same size, camera and geometry commit.  The caller has checked the size and set the device.
int gbuffer_prepare(pt_renderer* r) {
    pt_renderer::Aov& A = r->aov;
    const ViewKey key = view_key(r);
    if (A.rendered && A.key == key) return PT_OK;
    const size_t n = (size_t)r->width * (size_t)r->height;
    A.rendered = false;
    int rc = alloc_gbuffer(r, n);
    if (rc != PT_OK) {
        A.release();
        return rc;
    }
    DevLaunch L{};
    L.width = r->width;
    L.height = r->height;
    L.row0 = 0;
    L.image_height = r->height;
    std::memcpy(L.cam_pos, r->cam_pos, sizeof L.cam_pos);
    std::memcpy(L.inv_view, r->inv_view, sizeof L.inv_view);
    std::memcpy(L.inv_proj, r->inv_proj, sizeof L.inv_proj);
    L.debug_pixel = -1;
    const AovBuffers B = {A.d_albedo, A.d_normal, A.d_gnormal, A.d_position, A.d_depth, A.d_rough_metal,
                          A.d_prim,   A.d_gn,     A.d_gp,      A.d_ga,       A.d_gb,  A.d_hits};
    PT_HIP(A.ev_g[0].ensure(), "hipEventCreate");
    PT_HIP(A.ev_g[1].ensure(), "hipEventCreate");
    PT_HIP(hipMemsetAsync(A.d_hits, 0, sizeof(unsigned long long), r->stream), "hipMemset hit count");
    PT_HIP(hipEventRecord(A.ev_g[0], r->stream), "hipEventRecord");
    PT_HIP(gbuffer_render(r->scene(), L, B, r->stream), "G-buffer kernel");
    PT_HIP(hipEventRecord(A.ev_g[1], r->stream), "hipEventRecord");
    A.g_timed = true;
    A.key = key;
    A.rendered = true;
    A.renders++;
    return PT_OK;
}

int DenoiseCall::err(int code, const char* what) const { return fail(code, std::string(fn) + ": " + what); }

int DenoiseCall::check_source() const {
    if (!r) return err(PT_ERR_INVALID, "NULL renderer");
    if (source != PT_DENOISE_SRC_ACCUM && source != PT_DENOISE_SRC_DISPLAY && source != PT_DENOISE_SRC_HOST &&
        source != PT_DENOISE_SRC_ADAPTIVE)
        return err(PT_ERR_INVALID, "no such source");
    if (source == PT_DENOISE_SRC_HOST && !host_in) return err(PT_ERR_INVALID, "NULL host_in");
    // the newest source says which image it means: a host image beside it is a caller's mistake
    // (the older device sources ignore host_in, and keep doing so)
    if (source == PT_DENOISE_SRC_ADAPTIVE && host_in)
        return err(PT_ERR_INVALID, "host_in must be NULL with the adaptive source");
    return PT_OK;
}

int DenoiseCall::merge(const pt_denoise_options* opt) {
    o = kDefaults;
    if (!versioned_merge(o, opt)) return err(PT_ERR_INVALID, "denoise options struct_size is not set");
    return PT_OK;
}

int DenoiseCall::begin(bool reads_sigma_color) {
    if (o.iterations < 1 || o.iterations > 8) return err(PT_ERR_INVALID, "iterations must be 1..8");
    if ((reads_sigma_color && !(o.sigma_color > 0.0f)) || !(o.sigma_normal > 0.0f) || !(o.sigma_position > 0.0f))
        return err(PT_ERR_INVALID, "the sigmas must be > 0");
    if (!(o.albedo_floor > 0.0f)) return err(PT_ERR_INVALID, "albedo_floor must be > 0");
    if (r->width == 0) return err(PT_ERR_STATE, "call pt_resize first");
    if (source == PT_DENOISE_SRC_DISPLAY && !r->display_ready) return err(PT_ERR_STATE, "call pt_display_reset first");
    if (source == PT_DENOISE_SRC_ADAPTIVE && !r->adaptive.valid) return err(PT_ERR_STATE, "call pt_render_adaptive first");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    pt_renderer::Aov& A = r->aov;
    n = (size_t)r->width * (size_t)r->height;
    const int rc = gbuffer_prepare(r);
    if (rc) return rc;
    for (DevBuf<float4>& c : A.d_c)
        if (c.size() != n) PT_HIP(c.alloc(n), "hipMalloc filter colour");
    if (A.d_out.size() != 3 * n) PT_HIP(A.d_out.alloc(3 * n), "hipMalloc filter result");
    src = source == PT_DENOISE_SRC_ACCUM ? r->accum() : r->d_display.get();
    if (source == PT_DENOISE_SRC_ADAPTIVE) src = r->adaptive.buf.mean;
    if (source == PT_DENOISE_SRC_HOST) {
        if (A.d_in.size() != 3 * n) PT_HIP(A.d_in.alloc(3 * n), "hipMalloc filter source");
        PT_HIP(hipMemcpyAsync(A.d_in, host_in, sizeof(float) * 3 * n, hipMemcpyHostToDevice, r->stream), "upload source");
        PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");  // host_in is the caller's again
        src = A.d_in;
    }
    // A/B switch of tools/denoise_bench.py
    const char* e = std::getenv("PTAMD_DENOISE_LDS");
    lds = e ? std::atoi(e) : kAtrousLdsDefaultStep;
    P = AtrousParams{};
    P.out = A.d_out;
    P.gn = A.d_gn;
    P.gp = A.d_gp;
    P.ga = A.d_ga;
    P.w = r->width;
    P.h = r->height;
    P.inv_n = 1.0f / (o.sigma_normal * o.sigma_normal);
    P.inv_p = 1.0f / (o.sigma_position * o.sigma_position);
    P.floor = o.albedo_floor;
    P.demodulate = o.demodulate != 0;
    return PT_OK;
}

int DenoiseCall::finish(float* host_out) const {
    if (!host_out) return PT_OK;
    PT_HIP(hipMemcpyAsync(host_out, r->aov.d_out, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, r->stream), "download result");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    return collect_pending(r);
}

}  // namespace pt

extern "C" {

int pt_aov_channels(int32_t kind) { return kind >= 0 && kind < kAovKinds ? kAovChannels[kind] : -1; }

int pt_aov_download(pt_renderer* r, int32_t kind, void* host, int64_t bytes) {
    if (!r || !host) return fail(PT_ERR_INVALID, "pt_aov_download: NULL");
    if (pt_aov_channels(kind) < 0) return fail(PT_ERR_INVALID, "pt_aov_download: no such AOV kind");
    if (r->width == 0) return fail(PT_ERR_STATE, "pt_aov_download: call pt_resize first");
    const int64_t want = 4 * (int64_t)pt_aov_channels(kind) * (int64_t)r->width * (int64_t)r->height;
    if (bytes != want)
        return fail(PT_ERR_INVALID, "pt_aov_download: the buffer must hold " + std::to_string(want) + " bytes, not " +
                                        std::to_string(bytes));
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    const int rc = gbuffer_prepare(r);
    if (rc) return rc;
    PT_HIP(hipMemcpyAsync(host, aov_ptr(r, kind), (size_t)bytes, hipMemcpyDeviceToHost, r->stream), "download AOV");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    return collect_pending(r);
}

const void* pt_aov_device_ptr(pt_renderer* r, int32_t kind) {
    return r && r->aov.renders > 0 ? aov_ptr(r, kind) : nullptr;
}

int pt_denoise_options_default(pt_denoise_options* o) {
    if (!o) return fail(PT_ERR_INVALID, "pt_denoise_options_default: NULL");
    if (!versioned_write(o, kDefaults)) return fail(PT_ERR_INVALID, "pt_denoise_options_default: struct_size is not set");
    return PT_OK;
}

int pt_denoise(pt_renderer* r, int32_t source, const float* host_in, float scale, const pt_denoise_options* opt,
               float* host_out) {
    DenoiseCall c{"pt_denoise", r, source, host_in};
    int rc = c.check_source();
    if (!rc) rc = c.merge(opt);
    if (!rc) rc = c.begin(true);
    if (rc) return rc;
    pt_renderer::Aov& A = r->aov;
    AtrousParams& P = c.P;
    PT_HIP(A.ev_f[0].ensure(), "hipEventCreate");
    PT_HIP(A.ev_f[1].ensure(), "hipEventCreate");
    PT_HIP(hipEventRecord(A.ev_f[0], r->stream), "hipEventRecord");
    PT_HIP(atrous_pack(c.src, scale, P.demodulate != 0, P.floor, P.gn, P.ga, A.d_c[0], c.n, r->stream), "filter pack kernel");
    for (int i = 0; i < c.o.iterations; ++i) {
        const float sc = c.o.sigma_color * std::ldexp(1.0f, -i);  // sc * 2^-i, exact
        P.inv_c = 1.0f / (sc * sc);
        P.step = 1 << i;
        P.cin = A.d_c[i & 1];
        P.cout = A.d_c[(i & 1) ^ 1];
        PT_HIP(atrous_iteration(P, i == c.o.iterations - 1, c.lds, r->stream), "filter kernel");
    }
    PT_HIP(hipEventRecord(A.ev_f[1], r->stream), "hipEventRecord");
    A.f_timed = true;
    A.iterations = c.o.iterations;
    return c.finish(host_out);
}

float* pt_denoised_device_ptr(pt_renderer* r) { return r ? r->aov.d_out.get() : nullptr; }

int pt_get_denoise_info(pt_renderer* r, pt_denoise_info* out) {
    if (!r || !out) return fail(PT_ERR_INVALID, "pt_get_denoise_info: NULL");
    if (!versioned_bytes(out)) return fail(PT_ERR_INVALID, "pt_get_denoise_info: struct_size is not set");
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    PT_HIP(hipStreamSynchronize(r->stream), "hipStreamSynchronize");
    pt_renderer::Aov& A = r->aov;
    pt_denoise_info d{};
    d.iterations = A.iterations;
    d.gbuffer_renders = A.renders;
    float ms = 0.0f;
    if (A.g_timed) {
        PT_HIP(hipEventElapsedTime(&ms, A.ev_g[0], A.ev_g[1]), "G-buffer events");
        d.gbuffer_ms = ms;
    }
    if (A.f_timed) {
        PT_HIP(hipEventElapsedTime(&ms, A.ev_f[0], A.ev_f[1]), "filter events");
        d.filter_ms = ms;
    }
    if (A.rendered) {
        unsigned long long hits = 0;
        PT_HIP(hipMemcpy(&hits, A.d_hits, sizeof hits, hipMemcpyDeviceToHost), "download hit count");
        d.hit_pixels = hits;
    }
    versioned_write(out, d);
    return collect_pending(r);
}

}  // extern "C"
