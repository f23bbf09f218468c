// pt_aov.hip — first-hit feature buffers (the G-buffer) and the edge-avoiding a-trous wavelet
// filter that they guide (Dammertz et al. 2010, with albedo demodulation).  DESIGN.md §10.
//
// k_gbuffer: one thread per pixel, tiled like k_render_mega (a 256-thread workgroup covers 16x16
// pixels, each wave64 an 8x8 quadrant).  The pixel's unjittered camera ray is traced over the
// radiance ray's interval with the same acceptance rule (tri_accept_in) and alpha cut-out, and the hit is
// reconstructed as the first bounce of a path reconstructs it: what it writes equals the debug
// record of that bounce bit for bit; the hit's barycentrics and primitive go into a guide record of
// their own for the motion vectors of pt_temporal.hip.  No queues, no random numbers.
//
// ColourTerm: the filter's tap weight and store, run by k_filter / k_filter_rows of pt_atrous.h (the
// tiling and the 25-tap loop, shared with pt_temporal.hip).  The arithmetic is the specification in
// DESIGN.md §10, operation for operation and the same in every variant (the build is
// -ffp-contract=off); tests/test_gpu_denoise.py restates it in numpy and compares bit for bit.
#include "pt_atrous.h"
#include "pt_shade.h"

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

// The colour-distance term of DESIGN.md §10 for k_filter / k_filter_rows (pt_atrous.h).
struct ColourTerm {
    using Params = AtrousParams;
    static __device__ __host__ const AtrousParams& base(const Params& P) { return P; }

    f3 out;
    float wsum;
    f3 acc;

    __device__ __forceinline__ explicit ColourTerm(float4 cp) : out(mk(cp.x, cp.y, cp.z)) {}
    __device__ __forceinline__ void begin(const Params&, size_t, float4) {
        acc = mk(0.0f, 0.0f, 0.0f);
        wsum = 0.0f;
    }
    __device__ __forceinline__ void tap(float k, bool centre, float4 cq, float4 nq, float4 pq, float4 cp, float4 np,
                                        float4 pp, const AtrousParams& A) {
        float a = (d2(cq, cp) * A.inv_c + d2(nq, np) * A.inv_n) + d2(pq, pp) * A.inv_p;
        if (centre) a = 0.0f;
        if (a != a) return;
        const float w = k * pt_expf_neg(-a);
        acc = mk(acc.x + cq.x * w, acc.y + cq.y * w, acc.z + cq.z * w);
        wsum += w;
    }
    __device__ __forceinline__ void finish() { out = mk(acc.x / wsum, acc.y / wsum, acc.z / wsum); }
    template <bool LAST>
    __device__ __forceinline__ void store(const Params& A, size_t p, bool valid) {
        filter_store<LAST>(A, p, valid, out, 0.0f);
    }
};

}  // namespace

hipError_t gbuffer_render(const DevScene& S, const DevLaunch& L, const AovBuffers& B, hipStream_t stream) {
    with_flag(S.texinfo != nullptr, [&](auto tx) {
        hipLaunchKernelGGL(k_gbuffer<tx()>, tile_grid(L.width, L.height), dim3(kBlock), 0, stream, S, L, B);
    });
    return hipGetLastError();
}

hipError_t atrous_pack(const float* in, float scale, bool demodulate, float floor, const float4* gn, const float4* ga,
                       float4* c, size_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_atrous_pack, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, in, scale,
                       demodulate ? 1 : 0, floor, gn, ga, c, n);
    return hipGetLastError();
}

hipError_t atrous_iteration(const AtrousParams& A, bool last, int lds_max_step, hipStream_t stream) {
    return filter_iteration<ColourTerm>(A, last, lds_max_step, stream);
}

}  // namespace pt
