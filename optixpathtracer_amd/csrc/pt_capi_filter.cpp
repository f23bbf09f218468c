// pt_capi_filter.cpp — anti-aliasing (pt_set_pixel_filter): the sub-pixel cells, the
// filters' tap tables and the setting.  The cells and taps are computed on the host and uploaded
// once per setting; k_camera (pt_wavefront.hip) reads the cells, k_accum_filtered (pt_accum.hip)
// the taps.
#include "pt_renderer.h"

using namespace pt;

namespace {

const pt_pixel_filter kDefaults = {(uint32_t)sizeof(pt_pixel_filter), 1, PT_FILTER_BOX, 0.0f, 0.0f};
constexpr int kFilterKinds = 4;
constexpr double kDefaultRadius[kFilterKinds] = {0.5, 1.0, 1.5, 2.0};
constexpr int kMaxTaps = 2 * kFilterMaxR + 1;

bool valid_supersample(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }
int log2_of(int s) { return s == 8 ? 3 : s == 4 ? 2 : s == 2 ? 1 : 0; }

// (sx, sy) of cell index c: the top b bits of the radical inverse of c and of its second Sobol' dimension.
void cell_of(int s, uint32_t c, int* sx, int* sy) {
    const int b = log2_of(s);
    uint32_t ri = 0, sobol = 0, v = 1u << 31;
    for (int k = 0; k < 32; ++k) {
        if (c >> k & 1u) {
            ri |= 1u << (31 - k);
            sobol ^= v;
        }
        v ^= v >> 1;
    }
    *sx = b ? (int)(ri >> (32 - b)) : 0;
    *sy = b ? (int)(sobol >> (32 - b)) : 0;
}

// The 1-D profile of a resolved setting at distance t from the pixel centre, in output pixels.
double profile(const pt_pixel_filter& f, double t) {
    const double r = (double)f.radius, a = std::fabs(t);
    switch (f.kind) {
        case PT_FILTER_BOX: return a <= r ? 1.0 : 0.0;
        case PT_FILTER_TENT: return std::max(0.0, 1.0 - a / r);
        case PT_FILTER_GAUSSIAN: {
            const double s2 = 2.0 * (double)f.param * (double)f.param;
            return std::max(0.0, std::exp(-(t * t) / s2) - std::exp(-(r * r) / s2));
        }
        default: {  // Mitchell-Netravali
            const double B = (double)f.param, C = (1.0 - B) / 2.0, x = 2.0 * a / r;
            if (x < 1.0) return ((12.0 - 9.0 * B - 6.0 * C) * x * x * x + (-18.0 + 12.0 * B + 6.0 * C) * x * x + (6.0 - 2.0 * B)) / 6.0;
            if (x < 2.0)
                return ((-B - 6.0 * C) * x * x * x + (6.0 * B + 30.0 * C) * x * x + (-12.0 * B - 48.0 * C) * x +
                        (8.0 * B + 24.0 * C)) / 6.0;
            return 0.0;
        }
    }
}

// The caller's setting (NULL = the default) checked and resolved, and its R.
int resolve(const char* fn, const pt_pixel_filter* user, pt_pixel_filter* out, int* R) {
    const std::string who = std::string(fn) + ": ";
    pt_pixel_filter f = kDefaults;
    if (!versioned_merge(f, user)) return fail(PT_ERR_INVALID, who + "struct_size is not set");
    f.struct_size = (uint32_t)sizeof f;
    if (!valid_supersample(f.supersample)) return fail(PT_ERR_INVALID, who + "supersample must be 1, 2, 4 or 8");
    if (f.kind < 0 || f.kind >= kFilterKinds) return fail(PT_ERR_INVALID, who + "no such filter kind");
    if (f.radius == 0.0f) f.radius = (float)kDefaultRadius[f.kind];
    if (!(f.radius >= 0.5f && f.radius <= 2.5f)) return fail(PT_ERR_INVALID, who + "radius must be 0 or within 0.5 .. 2.5");
    if (f.param == 0.0f) f.param = f.kind == PT_FILTER_GAUSSIAN ? 0.5f : f.kind == PT_FILTER_MITCHELL ? 1.0f / 3.0f : 0.0f;
    *out = f;
    *R = (int)std::ceil((double)f.radius - 0.5);
    return PT_OK;
}

// One axis of one cell: w[i + R] = f(i + o), i = -R..R, in fp64, normalised, rounded to fp32.
bool tap_row(const pt_pixel_filter& f, int R, int cell_coord, float* w) {
    const double o = ((double)cell_coord + 0.5) / (double)f.supersample - 0.5;
    double v[kMaxTaps], sum = 0.0;
    for (int i = -R; i <= R; ++i) sum += v[i + R] = profile(f, (double)i + o);
    if (!std::isfinite(sum) || !(sum > 0.0)) return false;
    for (int i = 0; i <= 2 * R; ++i) w[i] = (float)(v[i] / sum);
    return true;
}

// The whole table: per cell 2 R + 1 taps along x, then 2 R + 1 along y.
int tap_table(const char* fn, const pt_pixel_filter& f, int R, std::vector<float>& taps) {
    const int s = f.supersample, K = 2 * R + 1;
    taps.assign((size_t)s * s * 2 * K, 0.0f);
    for (int c = 0; c < s * s; ++c) {
        int sx, sy;
        cell_of(s, (uint32_t)c, &sx, &sy);
        float* row = &taps[(size_t)c * 2 * K];
        if (!tap_row(f, R, sx, row) || !tap_row(f, R, sy, row + K))
            return fail(PT_ERR_INVALID, std::string(fn) + ": the taps' sum is not finite and positive");
    }
    return PT_OK;
}

}  // namespace

namespace pt {

bool filter_image_too_large(int supersample, int64_t w, int64_t h) {
    return (int64_t)supersample * supersample * w * h >= (int64_t)1 << 31;
}

}  // namespace pt

extern "C" {

int pt_pixel_filter_default(pt_pixel_filter* f) {
    if (!f) return fail(PT_ERR_INVALID, "pt_pixel_filter_default: NULL");
    if (!versioned_write(f, kDefaults)) return fail(PT_ERR_INVALID, "pt_pixel_filter_default: struct_size is not set");
    return PT_OK;
}

int pt_pixel_filter_cells(int32_t supersample, int32_t* xy) {
    if (!xy) return fail(PT_ERR_INVALID, "pt_pixel_filter_cells: NULL");
    if (!valid_supersample(supersample)) return fail(PT_ERR_INVALID, "pt_pixel_filter_cells: supersample must be 1, 2, 4 or 8");
    for (int c = 0; c < supersample * supersample; ++c) {
        int sx, sy;
        cell_of(supersample, (uint32_t)c, &sx, &sy);
        xy[2 * c] = sx;
        xy[2 * c + 1] = sy;
    }
    return PT_OK;
}

int pt_pixel_filter_taps(const pt_pixel_filter* f, int32_t cell, int32_t* R_out, float* wx, float* wy) {
    pt_pixel_filter s;
    int R = 0;
    int rc = resolve("pt_pixel_filter_taps", f, &s, &R);
    if (rc) return rc;
    if (cell < 0 || cell >= s.supersample * s.supersample) return fail(PT_ERR_INVALID, "pt_pixel_filter_taps: cell out of range");
    std::vector<float> taps;
    if ((rc = tap_table("pt_pixel_filter_taps", s, R, taps)) != PT_OK) return rc;
    const int K = 2 * R + 1;
    if (R_out) *R_out = R;
    if (wx) std::memcpy(wx, &taps[(size_t)cell * 2 * K], sizeof(float) * K);
    if (wy) std::memcpy(wy, &taps[(size_t)cell * 2 * K + K], sizeof(float) * K);
    return PT_OK;
}

int pt_set_pixel_filter(pt_renderer* r, const pt_pixel_filter* f) {
    if (!r) return fail(PT_ERR_INVALID, "pt_set_pixel_filter: NULL renderer");
    pt_pixel_filter s;
    int R = 0;
    int rc = resolve("pt_set_pixel_filter", f, &s, &R);
    if (rc) return rc;
    const bool active = s.supersample > 1 || R > 0;
    if (active && !r->multi.comms.empty()) return fail(PT_ERR_INVALID, "pt_set_pixel_filter: not on a multi-device renderer");
    if (filter_image_too_large(s.supersample, r->width, r->height))
        return fail(PT_ERR_INVALID, "pt_set_pixel_filter: supersample^2 * width * height must stay below 2^31");
    std::vector<float> taps;
    if ((rc = tap_table("pt_set_pixel_filter", s, R, taps)) != PT_OK) return rc;
    PT_HIP(hipSetDevice(r->device), "hipSetDevice");
    // the new tables first, beside the old ones: a failure leaves the setting as it was
    FilterStore next;
    if (s.supersample > 1) {
        std::vector<int> cells(2 * (size_t)s.supersample * s.supersample);
        pt_pixel_filter_cells(s.supersample, cells.data());
        PT_HIP(next.cells.alloc(cells.size()), "hipMalloc filter cells");
        PT_HIP(hipMemcpy(next.cells, cells.data(), sizeof(int) * cells.size(), hipMemcpyHostToDevice), "upload filter cells");
    }
    if (R > 0) {
        PT_HIP(next.taps.alloc(taps.size()), "hipMalloc filter taps");
        PT_HIP(hipMemcpy(next.taps, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice), "upload filter taps");
    }
    r->filter.set = s;
    r->filter.R = R;
    r->filter.version++;
    cancel_look_ahead(r);  // as a moved camera: the look-ahead frames in flight are stale
    // the old tables go once the launches that read them are done (hipFree waits)
    r->filter.buf.swap(next);
    return PT_OK;
}

int pt_get_pixel_filter(pt_renderer* r, pt_pixel_filter* f) {
    if (!r || !f) return fail(PT_ERR_INVALID, "pt_get_pixel_filter: NULL");
    if (!versioned_write(f, r->filter.set)) return fail(PT_ERR_INVALID, "pt_get_pixel_filter: struct_size is not set");
    return PT_OK;
}

}  // extern "C"
