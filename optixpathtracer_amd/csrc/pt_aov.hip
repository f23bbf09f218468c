// pt_aov.hip — first-hit feature buffers (the G-buffer) and the edge-avoiding a-trous wavelet
// filter that they guide (Dammertz et al. 2010, with albedo demodulation).  DESIGN.md §10.
//
// k_gbuffer: one thread per pixel, tiled like k_render_mega (a 256-thread workgroup covers 16x16
// pixels, each wave64 an 8x8 quadrant).  The pixel's unjittered camera ray is traced over the
// radiance ray's interval with the same strict re-trace rule and alpha cut-out, and the hit is
// reconstructed as the first bounce of a path reconstructs it: what it writes equals the debug
// record of that bounce bit for bit; the hit's barycentrics and primitive go into a guide record of
// their own for the motion vectors of pt_temporal.hip.  No queues, no random numbers.
//
// k_atrous / k_atrous_rows: one iteration of the filter, one thread per pixel, ping-pong float4
// colour buffers, no atomics.  Every load is a 16-byte record: the colour and the two guide records
// (normal | valid, position | depth).  The steps 1, 2 and 4 stage a 16x16 tile and its halo in LDS,
// the steps 8 and 16 a tile of rows one step apart, larger steps load every tap from global memory
// (measured: DESIGN.md §10).  The arithmetic is the specification in DESIGN.md §10, operation for
// operation and the same in every variant (the build is -ffp-contract=off);
// tests/test_gpu_denoise.py restates it in numpy and compares bit for bit.
#include "pt_atrous.h"

namespace pt {

namespace {

constexpr int kStack = PT_MK_STACK;

template <bool TEX>
__global__ __launch_bounds__(kBlock) void k_gbuffer(DevScene S, DevLaunch L, AovBuffers B) {
    __shared__ int stack[kStack * kBlock];
    int x, y;
    tile_pixel(x, y);
    const bool inside = x < L.width && y < L.height;
    bool hit = false;
    if (inside) {
        f3 o, d;
        camera_ray(L, x, y, o, d);
        Hit h;
        TravStats ts;
        hit = traverse<false, false, kStack, TEX>(S, o, d, 0.0f, 100.0f, h, stack + threadIdx.x, kBlock, ts);
        const size_t p = (size_t)y * (size_t)L.width + (size_t)x;
        f3 albedo = mk(0.0f, 0.0f, 0.0f), n = albedo, ng = albedo, pos = albedo;
        float depth = 0.0f, rough = 0.0f, metal = 0.0f, bu = 0.0f, bv = 0.0f;
        int prim = -1;
        if (hit) {
            SurfaceHit sf;
            reconstruct<TEX>(S, h, d, sf);
            albedo = sf.albedo;
            n = sf.fr.n;
            ng = sf.ng;
            pos = sf.pos;
            depth = h.t;
            rough = sf.roughness;
            metal = sf.metallic;
            bu = h.u;
            bv = h.v;
            prim = __float_as_int(S.isect[3 * h.tri].w);
        }
        store3(B.albedo, p, albedo);
        store3(B.normal, p, n);
        store3(B.gnormal, p, ng);
        store3(B.position, p, pos);
        B.depth[p] = depth;
        B.prim[p] = prim;
        B.rough_metal[2 * p] = rough;
        B.rough_metal[2 * p + 1] = metal;
        B.guide_n[p] = make_float4(n.x, n.y, n.z, hit ? 1.0f : 0.0f);
        B.guide_p[p] = make_float4(pos.x, pos.y, pos.z, depth);
        B.guide_a[p] = make_float4(albedo.x, albedo.y, albedo.z, 0.0f);
        B.guide_b[p] = make_float4(bu, bv, __int_as_float(prim), 0.0f);
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(B.hits, (unsigned long long)__popcll(m));
}

// c_0: the source (W*H*3 floats, times scale) as 16-byte records, demodulated at the hit pixels.
// The division runs here once per pixel, ahead of iteration 0's 25 loads of the record.
__global__ __launch_bounds__(kBlock) void k_atrous_pack(const float* __restrict__ in, float scale, int demodulate,
                                                        float floor, const float4* __restrict__ gn,
                                                        const float4* __restrict__ ga, float4* __restrict__ c,
                                                        size_t n) {
    const size_t p = blockIdx.x * (size_t)kBlock + threadIdx.x;
    if (p >= n) return;
    f3 v = mk(in[3 * p], in[3 * p + 1], in[3 * p + 2]);
    if (scale != 1.0f) v = v * scale;
    if (demodulate && gn[p].w != 0.0f) {
        const f3 a = albedo_floor(ga[p], floor);
        v = mk(v.x / a.x, v.y / a.y, v.z / a.z);
    }
    c[p] = make_float4(v.x, v.y, v.z, 0.0f);
}

// One tap: q's records against the centre's.
__device__ __forceinline__ void tap(float k, bool centre, float4 cq, float4 nq, float4 pq, float4 cp, float4 np,
                                    float4 pp, const AtrousParams& A, f3& acc, float& wsum) {
    float a = (d2(cq, cp) * A.inv_c + d2(nq, np) * A.inv_n) + d2(pq, pp) * A.inv_p;
    if (centre) a = 0.0f;
    if (a != a) return;
    const float w = k * pt_expf_neg(-a);
    acc = mk(acc.x + cq.x * w, acc.y + cq.y * w, acc.z + cq.z * w);
    wsum += w;
}

// c_{i+1}[p], or after the last iteration the remodulated result in the W*H*3 output.
template <bool LAST>
__device__ __forceinline__ void atrous_store(const AtrousParams& A, size_t p, bool valid, f3 out) {
    if (LAST) {
        if (valid && A.demodulate) out = out * albedo_floor(A.ga[p], A.floor);
        store3(A.out, p, out);
    } else {
        A.cout[p] = make_float4(out.x, out.y, out.z, 0.0f);
    }
}

// LAST: the remodulated result goes to the W*H*3 output instead of the next colour buffer.
// LSTEP > 0: the step is LSTEP, and the workgroup's tile with its halo of 2 * LSTEP pixels, (16 +
// 4 LSTEP)^2 records of 48 B, is staged in LDS first; LSTEP = 0: any step, every tap a global load.
template <bool LAST, int LSTEP>
__global__ __launch_bounds__(kBlock) void k_atrous(AtrousParams A) {
    constexpr bool LDS = LSTEP > 0;
    constexpr int side = kTile + 4 * LSTEP, kRecords = LDS ? side * side : 1;
    __shared__ float4 sc[kRecords], sn[kRecords], sp[kRecords];
    int x, y;
    tile_pixel(x, y);
    const int s = LDS ? LSTEP : A.step;
    const int ox = blockIdx.x * kTile - 2 * s, oy = blockIdx.y * kTile - 2 * s;
    if (LDS) {
        for (int i = threadIdx.x; i < side * side; i += kBlock) {
            const int gx = ox + i % side, gy = oy + i / side;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = c, p = c;  // n.w = 0: no tap outside the image
            if (gx >= 0 && gx < A.w && gy >= 0 && gy < A.h) {
                const size_t g = (size_t)gy * (size_t)A.w + (size_t)gx;
                c = A.cin[g];
                n = A.gn[g];
                p = A.gp[g];
            }
            sc[i] = c;
            sn[i] = n;
            sp[i] = p;
        }
        __syncthreads();
    }
    if (x >= A.w || y >= A.h) return;
    const size_t p = (size_t)y * (size_t)A.w + (size_t)x;
    const int lp = LDS ? (y - oy) * side + (x - ox) : 0;
    const float4 cp = LDS ? sc[lp] : A.cin[p], np = LDS ? sn[lp] : A.gn[p], pp = LDS ? sp[lp] : A.gp[p];
    const bool valid = np.w != 0.0f;
    f3 out = mk(cp.x, cp.y, cp.z);
    if (valid) {
        f3 acc = mk(0.0f, 0.0f, 0.0f);
        float wsum = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + dx * s, qy = y + dy * s;
                const float k = b3(dy + 2) * b3(dx + 2);
                float4 cq, nq, pq;
                if (LDS) {
                    const int lq = (qy - oy) * side + (qx - ox);
                    nq = sn[lq];
                    if (nq.w == 0.0f) continue;
                    cq = sc[lq];
                    pq = sp[lq];
                } else {
                    if (qx < 0 || qx >= A.w || qy < 0 || qy >= A.h) continue;
                    const size_t q = (size_t)qy * (size_t)A.w + (size_t)qx;
                    nq = A.gn[q];
                    if (nq.w == 0.0f) continue;
                    cq = A.cin[q];
                    pq = A.gp[q];
                }
                tap(k, dx == 0 && dy == 0, cq, nq, pq, cp, np, pp, A, acc, wsum);
            }
        }
        out = mk(acc.x / wsum, acc.y / wsum, acc.z / wsum);
    }
    atrous_store<LAST>(A, p, valid, out);
}

// The same iteration for the steps 8 and 16, where a square tile's halo outgrows the LDS: a
// workgroup takes 32 columns of 8 rows that lie `STEP` apart (thread = column + 32 * row), so the
// vertical taps are the neighbouring rows of its tile: (32 + 4 STEP) x 12 records.  blockIdx.y
// counts STEP row phases within each band of 8 * STEP image rows.
template <bool LAST, int STEP>
__global__ __launch_bounds__(kBlock) void k_atrous_rows(AtrousParams A) {
    constexpr int kCols = 32, kRows = 8, side = kCols + 4 * STEP, kRecords = side * (kRows + 4);
    __shared__ float4 sc[kRecords], sn[kRecords], sp[kRecords];
    const int ox = blockIdx.x * kCols - 2 * STEP;
    const int y0 = ((int)blockIdx.y / STEP) * (kRows * STEP) + (int)blockIdx.y % STEP;  // tile row 0
    for (int i = threadIdx.x; i < kRecords; i += kBlock) {
        const int gx = ox + i % side, gy = y0 + (i / side - 2) * STEP;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = c, p = c;  // n.w = 0: no tap outside the image
        if (gx >= 0 && gx < A.w && gy >= 0 && gy < A.h) {
            const size_t g = (size_t)gy * (size_t)A.w + (size_t)gx;
            c = A.cin[g];
            n = A.gn[g];
            p = A.gp[g];
        }
        sc[i] = c;
        sn[i] = n;
        sp[i] = p;
    }
    __syncthreads();
    const int col = threadIdx.x % kCols, row = threadIdx.x / kCols;
    const int x = blockIdx.x * kCols + col, y = y0 + row * STEP;
    if (x >= A.w || y >= A.h) return;
    const size_t p = (size_t)y * (size_t)A.w + (size_t)x;
    const int lp = (row + 2) * side + (x - ox);
    const float4 cp = sc[lp], np = sn[lp], pp = sp[lp];
    const bool valid = np.w != 0.0f;
    f3 out = mk(cp.x, cp.y, cp.z);
    if (valid) {
        f3 acc = mk(0.0f, 0.0f, 0.0f);
        float wsum = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int lq = lp + dy * side + dx * STEP;
                const float4 nq = sn[lq];
                if (nq.w == 0.0f) continue;
                tap(b3(dy + 2) * b3(dx + 2), dx == 0 && dy == 0, sc[lq], nq, sp[lq], cp, np, pp, A, acc, wsum);
            }
        }
        out = mk(acc.x / wsum, acc.y / wsum, acc.z / wsum);
    }
    atrous_store<LAST>(A, p, valid, out);
}

}  // namespace

hipError_t gbuffer_render(const DevScene& S, const DevLaunch& L, const AovBuffers& B, hipStream_t stream) {
    if (S.texinfo)
        hipLaunchKernelGGL(k_gbuffer<true>, tile_grid(L.width, L.height), dim3(kBlock), 0, stream, S, L, B);
    else
        hipLaunchKernelGGL(k_gbuffer<false>, tile_grid(L.width, L.height), dim3(kBlock), 0, stream, S, L, B);
    return hipGetLastError();
}

hipError_t atrous_pack(const float* in, float scale, bool demodulate, float floor, const float4* gn, const float4* ga,
                       float4* c, size_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_atrous_pack, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, in, scale,
                       demodulate ? 1 : 0, floor, gn, ga, c, n);
    return hipGetLastError();
}

template <bool LAST>
static hipError_t atrous_launch(const AtrousParams& A, int lds_max_step, hipStream_t stream) {
    const dim3 grid = tile_grid(A.w, A.h);
    const int lstep = A.step <= std::min(lds_max_step, kAtrousLdsMaxStep) ? A.step : 0;
    // k_atrous_rows: 32 columns per workgroup; per band of 8 * step rows, one workgroup per row phase
    const dim3 rows((unsigned)((A.w + 31) / 32), (unsigned)((A.h + 8 * A.step - 1) / (8 * A.step) * A.step));
    switch (lstep) {
        case 1: hipLaunchKernelGGL((k_atrous<LAST, 1>), grid, dim3(kBlock), 0, stream, A); break;
        case 2: hipLaunchKernelGGL((k_atrous<LAST, 2>), grid, dim3(kBlock), 0, stream, A); break;
        case 4: hipLaunchKernelGGL((k_atrous<LAST, 4>), grid, dim3(kBlock), 0, stream, A); break;
        case 8: hipLaunchKernelGGL((k_atrous_rows<LAST, 8>), rows, dim3(kBlock), 0, stream, A); break;
        case 16: hipLaunchKernelGGL((k_atrous_rows<LAST, 16>), rows, dim3(kBlock), 0, stream, A); break;
        default: hipLaunchKernelGGL((k_atrous<LAST, 0>), grid, dim3(kBlock), 0, stream, A); break;
    }
    return hipGetLastError();
}

hipError_t atrous_iteration(const AtrousParams& A, bool last, int lds_max_step, hipStream_t stream) {
    return last ? atrous_launch<true>(A, lds_max_step, stream) : atrous_launch<false>(A, lds_max_step, stream);
}

}  // namespace pt
