// pt_temporal.hip — temporal reprojection and the variance-guided a-trous filter (SVGF, Schied et
// al. 2017) on top of the G-buffer and the filter of pt_aov.hip.  DESIGN.md §11.
//
// k_temporal: one thread per pixel, 8x8 pixels per wave (tile_pixel).  A hit pixel's world position
// goes through the previous call's view and projection, the four bilinear taps around the point it
// lands on are tested against the previous guides, and the accepted history is blended with this
// call's colour and luminance moments.  Two counters, one atomic per workgroup each; nothing else is atomic.
// k_temporal<true> (motion vectors): the point that goes through the previous camera and into the
// plane test is the hit's previous position instead, the pixel's barycentrics applied to its
// triangle's vertices in k_snapshot's copy of the previous call's geometry: one more guide record
// and three vertex records per hit pixel, one more store, a third counter (the pixels that moved).
// k_snapshot: one thread per leaf-order triangle, three 16-byte copies to its global index's slot.
// k_motion_screen: the reprojected point's offset from the pixel, on demand (pt_motion_download).
// k_temporal_variance: where the history is shorter than variance_history, the variance comes from
// the moments of a 7x7 window, staged in LDS with its halo of 3 (a workgroup none of whose pixels
// needs it returns before staging).
// k_temporal_lscale: per iteration, the 3x3 Gaussian of the variance as the colour term's divisor.
// LuminanceTerm: the iterations are pt_denoise's own kernels, k_filter / k_filter_rows of pt_atrous.h,
// over colour | variance records with the luminance term in place of the colour distance.
// Every load is a 16-byte record except the divisor; the arithmetic is the specification of §11,
// the same in every variant (-ffp-contract=off); tests/temporal_ref.py restates it in numpy.
#include "pt_atrous.h"

namespace pt {

namespace {

__device__ __forceinline__ float dot3(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// §11 step 1: the world point q through the previous camera.  Where it lands in that camera's image
// of n pixels across (not tested against the image) means something only in front of the camera.
struct Reprojection {
    float clip[4];
    __device__ __forceinline__ Reprojection(const float* prev_view, const float* prev_proj, f3 q) {
        const float P[4] = {q.x, q.y, q.z, 1.0f};
        float vw[4];
        mat4_mul_vec4(prev_view, P, vw);
        mat4_mul_vec4(prev_proj, vw, clip);
    }
    __device__ __forceinline__ bool in_front() const { return clip[3] > 0.0f; }
    __device__ __forceinline__ float fx(int n) const { return ((clip[0] / clip[3]) * 0.5f + 0.5f) * (float)n - 0.5f; }
    __device__ __forceinline__ float fy(int n) const { return ((clip[1] / clip[3]) * 0.5f + 0.5f) * (float)n - 0.5f; }
};

template <bool MOTION>
__global__ __launch_bounds__(kBlock) void k_temporal(TemporalParams T) {
    int x, y;
    tile_pixel(x, y);
    bool hit = false, accepted = false, moved = false;
    if (x < T.w && y < T.h) {
        const size_t p = (size_t)y * (size_t)T.w + (size_t)x;
        const float4 c = T.c[p], np = T.gn[p];
        hit = np.w != 0.0f;
        float4 tc = make_float4(c.x, c.y, c.z, 0.0f), tm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 prev = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (hit) {
            const float4 pp = T.gp[p];
            // rp: the point reprojected and plane-tested; reconstruct's expression for s.pos over the snapshot
            f3 rp = mk(pp.x, pp.y, pp.z);
            if (MOTION) {
                const float4 b = T.gb[p];
                const int g = __float_as_int(b.z);
                if (g >= 0 && g < T.ntri) {
                    const float4 v0 = T.snap[3 * (size_t)g], v1 = T.snap[3 * (size_t)g + 1], v2 = T.snap[3 * (size_t)g + 2];
                    const float u = b.x, v = b.y;
                    const float w = 1.0f - u - v;
                    rp = mk(w * v0.x + u * v1.x + v * v2.x, w * v0.y + u * v1.y + v * v2.y, w * v0.z + u * v1.z + v * v2.z);
                }
                moved = rp.x != pp.x || rp.y != pp.y || rp.z != pp.z;
                prev = make_float4(rp.x, rp.y, rp.z, 0.0f);
            }
            const float l = luminance(c);
            f3 hcol = mk(0.0f, 0.0f, 0.0f);
            float h1 = 0.0f, h2 = 0.0f, hlen = 0.0f;
            if (T.history) {
                const Reprojection R(T.prev_view, T.prev_proj, rp);
                if (R.in_front()) {
                    const float fx = R.fx(T.w), fy = R.fy(T.h);
                    // outside this range no tap is inside the image (a NaN is outside)
                    if (fx >= -1.0f && fx < (float)T.w && fy >= -1.0f && fy < (float)T.h) {
                        const float ffx = floorf(fx), ffy = floorf(fy);
                        const int ix = (int)ffx, iy = (int)ffy;
                        const float tx = fx - ffx, ty = fy - ffy;
                        const float lim = T.plane_distance * pp.w;
                        float ws = 0.0f;
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
#pragma unroll
                            for (int i = 0; i < 2; ++i) {
                                const int qx = ix + i, qy = iy + j;
                                if (qx < 0 || qx >= T.w || qy < 0 || qy >= T.h) continue;
                                const size_t q = (size_t)qy * (size_t)T.w + (size_t)qx;
                                const float4 nq = T.pgn[q];
                                if (nq.w == 0.0f) continue;
                                if (!(dot3(nq, np) >= T.normal_cos)) continue;
                                const float4 pq = T.pgp[q];
                                const float4 d = make_float4(rp.x - pq.x, rp.y - pq.y, rp.z - pq.z, 0.0f);
                                if (!(fabsf(dot3(d, np)) <= lim)) continue;
                                const float4 hc = T.hc[q], hm = T.hm[q];
                                if (!(finite(hc.x) && finite(hc.y) && finite(hc.z) && finite(hm.x) && finite(hm.y) &&
                                      finite(hm.z)))
                                    continue;
                                const float wgt = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                                ws += wgt;
                                hcol = mk(hcol.x + hc.x * wgt, hcol.y + hc.y * wgt, hcol.z + hc.z * wgt);
                                h1 += hm.x * wgt;
                                h2 += hm.y * wgt;
                                hlen += hm.z * wgt;
                            }
                        }
                        if (ws >= 0.01f) {
                            accepted = true;
                            hcol = mk(hcol.x / ws, hcol.y / ws, hcol.z / ws);
                            h1 = h1 / ws;
                            h2 = h2 / ws;
                            hlen = hlen / ws;
                        }
                    }
                }
            }
            f3 t = mk(c.x, c.y, c.z);
            float m1 = l, m2 = l * l, N = 1.0f;
            if (accepted) {
                N = hlen + 1.0f;
                if (!(N < T.max_history)) N = T.max_history;
                const float r = 1.0f / N;
                const float a = T.alpha < r ? r : T.alpha, am = T.alpha_moments < r ? r : T.alpha_moments;
                t = mk(hcol.x + (c.x - hcol.x) * a, hcol.y + (c.y - hcol.y) * a, hcol.z + (c.z - hcol.z) * a);
                m1 = h1 + (l - h1) * am;
                m2 = h2 + (l * l - h2) * am;
            }
            const float dv = m2 - m1 * m1;
            tc = make_float4(t.x, t.y, t.z, dv > 0.0f ? dv : 0.0f);
            tm = make_float4(m1, m2, N, 0.0f);
        }
        T.tc[p] = tc;
        T.tm[p] = tm;
        if (MOTION) T.pp[p] = prev;
    }
    // the counters (two, with motion three): the waves' ballots meet in LDS, one atomic per counter and workgroup
    constexpr int kCnt = MOTION ? 3 : 2;
    __shared__ unsigned cnt[kCnt * (kBlock / 64)];
    const unsigned long long ma = __ballot(hit && accepted), mr = __ballot(hit && !accepted);
    if ((threadIdx.x & 63) == 0) {
        cnt[kCnt * (threadIdx.x >> 6)] = (unsigned)__popcll(ma);
        cnt[kCnt * (threadIdx.x >> 6) + 1] = (unsigned)__popcll(mr);
    }
    if (MOTION) {
        const unsigned long long mm = __ballot(hit && moved);
        if ((threadIdx.x & 63) == 0) cnt[kCnt * (threadIdx.x >> 6) + 2] = (unsigned)__popcll(mm);
    }
    __syncthreads();
    if (threadIdx.x < kCnt) {
        const unsigned c = (cnt[threadIdx.x] + cnt[kCnt + threadIdx.x]) + (cnt[2 * kCnt + threadIdx.x] + cnt[3 * kCnt + threadIdx.x]);
        if (c) atomicAdd(T.count + threadIdx.x, (unsigned long long)c);
    }
}

__global__ __launch_bounds__(kBlock) void k_snapshot(const float4* __restrict__ isect, const float4* __restrict__ shade,
                                                     int ntri, float4* __restrict__ snap) {
    const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (t >= ntri) return;
    const float4 a = isect[3 * (size_t)t];
    const int g = __float_as_int(a.w);
    if (g < 0 || g >= ntri) return;
    snap[3 * (size_t)g] = a;
    snap[3 * (size_t)g + 1] = shade[4 * (size_t)t];
    snap[3 * (size_t)g + 2] = shade[4 * (size_t)t + 1];
}

struct ScreenParams {
    float prev_view[16], prev_proj[16];
};

__global__ __launch_bounds__(kBlock) void k_motion_screen(const float4* __restrict__ pp, const float4* __restrict__ gn,
                                                          ScreenParams M, int history, int w, int h, float* __restrict__ out) {
    int x, y;
    tile_pixel(x, y);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    f3 o = mk(0.0f, 0.0f, 0.0f);
    if (history && gn[p].w != 0.0f) {
        const float4 q = pp[p];
        const Reprojection R(M.prev_view, M.prev_proj, mk(q.x, q.y, q.z));
        if (R.in_front()) {
            const float fx = R.fx(w), fy = R.fy(h);
            o = mk(fx - (float)x, fy - (float)y, 1.0f);
        }
    }
    store3(out, p, o);
}

// The 7x7 estimate: 16x16 pixels and their halo of 3, 22^2 records of 48 B (23 KB) in LDS.
__global__ __launch_bounds__(kBlock) void k_temporal_variance(const float4* __restrict__ gn, const float4* __restrict__ gp,
                                                              const float4* __restrict__ tm, float4* __restrict__ tc, int w,
                                                              int h, float inv_n, float inv_p, float vh) {
    constexpr int side = kTile + 6;
    __shared__ float4 sn[side * side], sp[side * side], sm[side * side];
    int x, y;
    tile_pixel(x, y);
    const bool inside = x < w && y < h;
    const size_t p = inside ? (size_t)y * (size_t)w + (size_t)x : 0;
    bool need = false;
    if (inside) need = gn[p].w != 0.0f && tm[p].z < vh;
    if (!__syncthreads_or(need ? 1 : 0)) return;
    const int ox = blockIdx.x * kTile - 3, oy = blockIdx.y * kTile - 3;
    for (int i = threadIdx.x; i < side * side; i += kBlock)
        stage(gn, gp, tm, w, h, ox + i % side, oy + i / side, sn[i], sp[i], sm[i]);
    __syncthreads();
    if (!need) return;
    const int lp = (y - oy) * side + (x - ox);
    const float4 np = sn[lp], pp = sp[lp];
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int dy = -3; dy <= 3; ++dy) {
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int lq = lp + dy * side + dx;
            const float4 nq = sn[lq];
            if (nq.w == 0.0f) continue;
            float wgt = 1.0f;
            if (dx != 0 || dy != 0) wgt = pt_expf_neg(-(d2(nq, np) * inv_n + d2(sp[lq], pp) * inv_p));
            const float4 mq = sm[lq];
            sw += wgt;
            s1 += mq.x * wgt;
            s2 += mq.y * wgt;
        }
    }
    const float mu1 = s1 / sw, mu2 = s2 / sw;
    const float dv = mu2 - mu1 * mu1;
    reinterpret_cast<float*>(tc)[4 * p + 3] = (dv > 0.0f ? dv : 0.0f) * (vh / sm[lp].z);
}

__device__ __forceinline__ float g3(int i) { return i == 1 ? 0.5f : 0.25f; }  // [1/4, 1/2, 1/4]

__global__ __launch_bounds__(kBlock) void k_temporal_lscale(const float4* __restrict__ cin, const float4* __restrict__ gn,
                                                            float* __restrict__ den, int w, int h, float sigma_l) {
    int x, y;
    tile_pixel(x, y);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    float out = 0.0f;
    if (gn[p].w != 0.0f) {
        float sum = 0.0f, ks = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
                if (gn[q].w == 0.0f) continue;
                const float k = g3(dy + 1) * g3(dx + 1);
                sum += cin[q].w * k;
                ks += k;
            }
        }
        out = sigma_l * sqrtf(sum / ks) + 1e-8f;
    }
    den[p] = out;
}

// The luminance term of DESIGN.md §11 step 3 for k_filter / k_filter_rows (pt_atrous.h), over colour |
// variance records: den = the centre's divisor, hist = where the result is stored besides (or NULL).
struct LuminanceTerm {
    struct Params {
        AtrousParams A;
        const float* den;
        float4* hist;
    };
    static __device__ __host__ const AtrousParams& base(const Params& P) { return P.A; }

    f3 out, acc;
    float v, den, lum, vacc, wsum;

    __device__ __forceinline__ explicit LuminanceTerm(float4 cp) : out(mk(cp.x, cp.y, cp.z)), v(cp.w) {}
    __device__ __forceinline__ void begin(const Params& P, size_t p, float4 cp) {
        den = P.den[p];
        lum = luminance(cp);
        acc = mk(0.0f, 0.0f, 0.0f);
        wsum = 0.0f;
        vacc = 0.0f;
    }
    __device__ __forceinline__ void tap(float k, bool centre, float4 cq, float4 nq, float4 pq, float4, float4 np,
                                        float4 pp, const AtrousParams& A) {
        float a = (fabsf(luminance(cq) - lum) / den + d2(nq, np) * A.inv_n) + d2(pq, pp) * A.inv_p;
        if (centre) a = 0.0f;
        if (a != a) return;
        const float w = k * pt_expf_neg(-a);
        acc = mk(acc.x + cq.x * w, acc.y + cq.y * w, acc.z + cq.z * w);
        vacc += cq.w * (w * w);
        wsum += w;
    }
    __device__ __forceinline__ void finish() {
        out = mk(acc.x / wsum, acc.y / wsum, acc.z / wsum);
        v = vacc / (wsum * wsum);
    }
    template <bool LAST>
    __device__ __forceinline__ void store(const Params& P, size_t p, bool valid) {
        if (P.hist) P.hist[p] = make_float4(out.x, out.y, out.z, v);
        filter_store<LAST>(P.A, p, valid, out, v);
    }
};

}  // namespace

hipError_t temporal_blend(const TemporalParams& T, bool motion, hipStream_t stream) {
    if (motion)
        hipLaunchKernelGGL(k_temporal<true>, tile_grid(T.w, T.h), dim3(kBlock), 0, stream, T);
    else
        hipLaunchKernelGGL(k_temporal<false>, tile_grid(T.w, T.h), dim3(kBlock), 0, stream, T);
    return hipGetLastError();
}

hipError_t temporal_snapshot(const float4* isect, const float4* shade, int ntri, float4* snap, hipStream_t stream) {
    if (ntri <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_snapshot, dim3((unsigned)((ntri + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, isect, shade, ntri,
                       snap);
    return hipGetLastError();
}

hipError_t temporal_motion_screen(const float4* pp, const float4* gn, const float* prev_view, const float* prev_proj,
                                  int history, int w, int h, float* out, hipStream_t stream) {
    ScreenParams M;
    for (int i = 0; i < 16; ++i) M.prev_view[i] = prev_view[i], M.prev_proj[i] = prev_proj[i];
    hipLaunchKernelGGL(k_motion_screen, tile_grid(w, h), dim3(kBlock), 0, stream, pp, gn, M, history, w, h, out);
    return hipGetLastError();
}

hipError_t temporal_variance(const float4* gn, const float4* gp, const float4* tm, float4* tc, int w, int h, float inv_n,
                             float inv_p, float variance_history, hipStream_t stream) {
    hipLaunchKernelGGL(k_temporal_variance, tile_grid(w, h), dim3(kBlock), 0, stream, gn, gp, tm, tc, w, h, inv_n, inv_p,
                       variance_history);
    return hipGetLastError();
}

hipError_t temporal_luminance_scale(const float4* cin, const float4* gn, float* den, int w, int h, float sigma_luminance,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(k_temporal_lscale, tile_grid(w, h), dim3(kBlock), 0, stream, cin, gn, den, w, h, sigma_luminance);
    return hipGetLastError();
}

hipError_t temporal_atrous_iteration(const AtrousParams& A, const float* den, float4* hist, bool last, int lds_max_step,
                                     hipStream_t stream) {
    return filter_iteration<LuminanceTerm>({A, den, hist}, last, lds_max_step, stream);
}

}  // namespace pt
