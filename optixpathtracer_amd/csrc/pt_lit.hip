// pt_lit.hip — builds the lit table (pt_lit.h): the per-triangle subdivision on the host at
// pt_create, the (light, cell) bits on the GPU whenever the lights change, and after them the
// occluder candidate of every cell the bits leave to the tracer (k_occ_build); and the skip table
// (pt_skip.h) whenever the triangle records or the BVH change.
#include "pt_internal.h"
#include "pt_shade.h"
#include "pt_skip.h"

namespace pt {

// Per-triangle words from the leaf-ordered isect records (host copy).  False: the scene runs
// without the table (no triangles, a coordinate beyond kLitMaxCoord or not finite, too many cells).
bool lit_subdivide(const float4* isect, int ntri, std::vector<uint32_t>& words, uint32_t* cells, float* diagonal) {
    words.clear();
    *cells = 0;
    *diagonal = 0.0f;
    if (ntri <= 0) return false;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = 0; t < ntri; ++t) {
        const float4 A = isect[3 * t], E1 = isect[3 * t + 1], E2 = isect[3 * t + 2];
        const float v[3][3] = {{A.x, A.y, A.z}, {A.x + E1.x, A.y + E1.y, A.z + E1.z}, {A.x + E2.x, A.y + E2.y, A.z + E2.z}};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                if (!(fabsf(v[k][a]) <= kLitMaxCoord)) return false;  // also NaN
                lo[a] = std::min(lo[a], v[k][a]);
                hi[a] = std::max(hi[a], v[k][a]);
            }
    }
    const double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
    const float diag = (float)std::sqrt(dx * dx + dy * dy + dz * dz);
    if (!(diag > 0.0f)) return false;
    const float target = kLitCellFraction * diag;
    words.resize((size_t)ntri);
    uint64_t n = 0;
    for (int t = 0; t < ntri; ++t) {
        const float4 E1 = isect[3 * t + 1], E2 = isect[3 * t + 2];
        const double a[3] = {E1.x, E1.y, E1.z}, b[3] = {E2.x, E2.y, E2.z}, o[3] = {0.0, 0.0, 0.0};
        LitPlane p;
        int k = kLitNoCells;
        if (lit_plane_through(o, a, b, p)) {
            const double l1 = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
            const double l2 = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
            const double c[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
            const double l3 = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            k = lit_level_for((float)std::max(l1, std::max(l2, l3)), target);
        }
        if (n > kLitMaxCells) return false;
        words[(size_t)t] = lit_word(k, (uint32_t)n);
        n += lit_cells(k);
    }
    if (n == 0 || n > kLitMaxCells) return false;
    *cells = (uint32_t)n;
    *diagonal = diag;
    return true;
}

namespace {

// One wave per block with the walk stack in LDS (entry s of lane l at stk[s * 64 + l], conflict-free):
// the kernel uses no scratch memory.  A private stack made it 400 B per lane, and the runtime's
// scratch for the whole device (hundreds of MB, released again after the launch) moved the free
// device memory under callers that size their allocations by it.
constexpr int kLitBlock = 64;
constexpr int kLitStack = 72;  // an unordered walk holds at most 3 entries per BVH4 level + 1 (pt_create: 3 * depth <= 71)

__global__ __launch_bounds__(kLitBlock) void k_lit_build(DevScene S, const uint32_t* __restrict__ tri_words,
                                                        uint32_t cells, uint32_t words, const DevLight* __restrict__ lights,
                                                        int n_lights, uint32_t* __restrict__ bits, float diag) {
    __shared__ int lds_stack[kLitStack * kLitBlock];
    int* const stack = lds_stack + threadIdx.x;
    const uint64_t id = (uint64_t)blockIdx.x * kLitBlock + threadIdx.x;
    if (id >= (uint64_t)cells * (uint64_t)n_lights) return;
    const int li = (int)(id / cells);
    const uint32_t cell = (uint32_t)(id - (uint64_t)li * cells);
    // the triangle of the cell: the last one whose first cell is <= cell (a triangle without
    // cells shares its successor's first cell and sorts before it)
    int a = 0, b = S.ntri - 1;
    while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (lit_first(tri_words[m]) <= cell) a = m; else b = m - 1;
    }
    const int t = a;
    const uint32_t w = tri_words[t];
    const int k = lit_level(w);
    if (k == kLitNoCells || cell - lit_first(w) >= lit_cells(k)) return;
    const float4 A = S.isect[3 * t], E1 = S.isect[3 * t + 1], E2 = S.isect[3 * t + 2];
    const float v0[3] = {A.x, A.y, A.z}, e1[3] = {E1.x, E1.y, E1.z}, e2[3] = {E2.x, E2.y, E2.z};
    const DevLight lt = lights[li];
    const float lp[3] = {lt.px, lt.py, lt.pz};
    // a light beyond the coordinate bound (or not finite) gets no bits: l - p would round by up to
    // an ulp of l in the shading kernels' fp32 side test, no longer far below kLitDelta (pt_lit.h)
    if (!(fabsf(lp[0]) <= kLitMaxCoord && fabsf(lp[1]) <= kLitMaxCoord && fabsf(lp[2]) <= kLitMaxCoord)) return;
    LitPyramid P;
    const float margin = lit_margin_cell(diag, lit_cell_reach(v0, e1, e2, k, cell - lit_first(w), lp));
    if (!lit_pyramid(v0, e1, e2, k, cell - lit_first(w), lp, kLitDelta, margin, P)) return;
    int sp = 0;
    stack[kLitBlock * sp++] = 0;  // the root is an inner node
    while (sp > 0) {
        const int c = stack[kLitBlock * --sp];
        if (c >= 0) {
            const BNode4 nd = S.nodes[c];
            const float lox[4] = {nd.lox.x, nd.lox.y, nd.lox.z, nd.lox.w}, hix[4] = {nd.hix.x, nd.hix.y, nd.hix.z, nd.hix.w};
            const float loy[4] = {nd.loy.x, nd.loy.y, nd.loy.z, nd.loy.w}, hiy[4] = {nd.hiy.x, nd.hiy.y, nd.hiy.z, nd.hiy.w};
            const float loz[4] = {nd.loz.x, nd.loz.y, nd.loz.z, nd.loz.w}, hiz[4] = {nd.hiz.x, nd.hiz.y, nd.hiz.z, nd.hiz.w};
            const int ch[4] = {nd.child.x, nd.child.y, nd.child.z, nd.child.w};
            for (int q = 0; q < 4; ++q) {
                if (ch[q] == kEmptyChild) continue;
                const double lo[3] = {lox[q], loy[q], loz[q]}, hi[3] = {hix[q], hiy[q], hiz[q]};
                if (lit_box_outside(P, lo, hi)) continue;
                if (sp >= kLitStack) return;  // full stack: the bit stays 0
                stack[kLitBlock * sp++] = ch[q];
            }
        } else {
            const int first = leaf_first(c), cnt = leaf_count(c);
            for (int q = 0; q < cnt; ++q) {
                const int u = first + q;
                const float4 UA = S.isect[3 * u], U1 = S.isect[3 * u + 1], U2 = S.isect[3 * u + 2];
                const double pa[3] = {UA.x, UA.y, UA.z};
                const double pb[3] = {(double)UA.x + U1.x, (double)UA.y + U1.y, (double)UA.z + U1.z};
                const double pc[3] = {(double)UA.x + U2.x, (double)UA.y + U2.y, (double)UA.z + U2.z};
                if (!lit_tri_outside(P, pa, pb, pc)) return;  // a possible occluder (cut-outs count as opaque)
            }
        }
    }
    atomicOr(&bits[(size_t)li * words + (cell >> 5)], 1u << (cell & 31));
}

// The occluder candidate table: one int per (light, cell), laid out light * cells + cell,
// -1 or the leaf-order index of a triangle that probably occludes the cell's shadow rays.  It is a
// hint: the shading kernels test the named triangle with the tracer's own tri_test + tri_accept_in on the
// very ray they would emit, and a passing test is the tracer's "occluded" for ANY triangle (the BVH's
// boxes hold the triangle's padded box, so the any-hit walk reaches it or stops earlier at another
// hit).  A wrong or stale entry costs speed only; the one invariant is -1 <= entry < ntri.
// The candidate is the closest hit of the shadow ray from the cell's centroid, in plain fp32 and with
// no margin.  A cell with its lit bit set, a triangle without cells, a light beyond kLitMaxCoord or not
// more than kLitDelta above the plane get -1, and so does a cut-out triangle (E2.w != 0), so the
// textured kernels never evaluate alpha_cut for a candidate.
// Scratch-free like k_lit_build: trav_step's stack lives in LDS, kOccStack entries per lane.  Its
// spill (stack_spill) moves kOccStack / 2 entries at a time and gives up when they do not fit in
// kSpillDepth: kOccStack / 2 > kSpillDepth, so the spill array is never written or read (it points at
// one LDS word), and 3 * depth <= 71 < kOccStack - 3 (pt_create) never gets that far anyway.
constexpr int kOccStack = 2 * kSpillDepth + 2;
static_assert(kOccStack / 2 > kSpillDepth && kOccStack - 3 > 72, "k_occ_build: the spill must stay unused");

__global__ __launch_bounds__(kLitBlock) void k_occ_build(DevScene S, const uint32_t* __restrict__ tri_words,
                                                        uint32_t cells, uint32_t words, const DevLight* __restrict__ lights,
                                                        int n_lights, const uint32_t* __restrict__ bits,
                                                        int* __restrict__ occ) {
    __shared__ int lds_stack[kOccStack * kLitBlock];
    __shared__ int lds_spill[1];
    const uint64_t id = (uint64_t)blockIdx.x * kLitBlock + threadIdx.x;
    if (id >= (uint64_t)cells * (uint64_t)n_lights) return;
    const int li = (int)(id / cells);
    const uint32_t cell = (uint32_t)(id - (uint64_t)li * cells);
    int cand = -1;
    do {
        if ((bits[(size_t)li * words + (cell >> 5)] >> (cell & 31)) & 1u) break;  // lit: no shadow ray here
        int a = 0, b = S.ntri - 1;  // the triangle of the cell, as k_lit_build
        while (a < b) {
            const int m = (a + b + 1) >> 1;
            if (lit_first(tri_words[m]) <= cell) a = m; else b = m - 1;
        }
        const int t = a;
        const uint32_t w = tri_words[t];
        const int k = lit_level(w);
        if (k == kLitNoCells || cell - lit_first(w) >= lit_cells(k)) break;
        const DevLight lt = lights[li];
        if (!(fabsf(lt.px) <= kLitMaxCoord && fabsf(lt.py) <= kLitMaxCoord && fabsf(lt.pz) <= kLitMaxCoord)) break;
        const float4 A = S.isect[3 * t], E1 = S.isect[3 * t + 1], E2 = S.isect[3 * t + 2];
        int cu[3], cv[3];
        lit_cell_corners(k, cell - lit_first(w), cu, cv);
        const float s = 1.0f / (3.0f * (float)(1 << k));
        const float u = (float)(cu[0] + cu[1] + cu[2]) * s, v = (float)(cv[0] + cv[1] + cv[2]) * s;
        const f3 e1 = mk(E1.x, E1.y, E1.z), e2 = mk(E2.x, E2.y, E2.z);
        const f3 p = mk(A.x, A.y, A.z) + u * e1 + v * e2;
        const f3 n = cross(e1, e2);
        const float nl = length(n);
        if (!(nl > 0.0f)) break;
        f3 ng = n / nl;
        const f3 ldir = mk(lt.px, lt.py, lt.pz) - p;
        float h = dot(ldir, ng);
        if (h < 0.0f) {
            ng = -ng;
            h = -h;
        }
        if (!(h > kLitDelta)) break;  // also NaN
        TravState st;
        TravStats ts;
        f3 so, sdir;
        float stmax;
        shadow_ray(p, ng, ldir, so, sdir, stmax);  // the ray a shading kernel emits from there
        trav_init(st, so, sdir, 0.0f, stmax);
        while (!trav_step<kRayClosest, false, kOccStack, false>(S, st, lds_stack + threadIdx.x, kLitBlock, lds_spill, ts)) {
        }
        if (st.h.tri >= 0 && st.h.tri < S.ntri && __float_as_int(S.isect[3 * st.h.tri + 2].w) == 0) cand = st.h.tri;
    } while (false);
    occ[id] = cand;
}

// The skip table (pt_skip.h): the parent links of the BVH4, then one thread per (side, triangle) --
// side-major, so that neighbouring lanes climb neighbouring paths -- with the walk stack in LDS as in
// k_lit_build.
// node_parent[n_nodes] (zeroed by skip_build) is set when the scene holds a sliver: no box_accept then.
__global__ __launch_bounds__(kLitBlock) void k_skip_parents(const BNode4* __restrict__ nodes,
                                                           const float4* __restrict__ isect, int n_nodes,
                                                           int* __restrict__ node_parent, int* __restrict__ tri_parent) {
    const int i = (int)(blockIdx.x * kLitBlock + threadIdx.x);
    if (i < n_nodes && skip_parents_of(nodes, reinterpret_cast<const float*>(isect), i, node_parent, tri_parent))
        atomicOr(&node_parent[n_nodes], 1);
}

__global__ __launch_bounds__(kLitBlock) void k_skip_build(DevScene S, const int* __restrict__ node_parent,
                                                         const int* __restrict__ tri_parent,
                                                         uint32_t* __restrict__ words) {
    __shared__ int lds_stack[kLitStack * kLitBlock];
    const int id = (int)(blockIdx.x * kLitBlock + threadIdx.x);
    if (id >= 2 * S.ntri) return;
    const int side = id >= S.ntri ? 1 : 0, t = id - side * S.ntri;
    words[2 * t + side] = skip_word(S.nodes, reinterpret_cast<const float*>(S.isect), node_parent, tri_parent, t, side,
                                    lds_stack + threadIdx.x, kLitBlock, kLitStack, node_parent[S.n_nodes] == 0);
}

}  // namespace

// Rebuilds the skip table of the scene's triangles and nodes on `stream`: words[2 t + side];
// node_parent (n_nodes + 1 ints, the last one the scene's sliver flag) and tri_parent (ntri ints) are
// its scratch.
hipError_t skip_build(const DevScene& S, int* node_parent, int* tri_parent, uint32_t* words, hipStream_t stream) {
    if (S.ntri <= 0 || S.n_nodes <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(node_parent + S.n_nodes, 0, sizeof(int), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_skip_parents, dim3((unsigned)((S.n_nodes + kLitBlock - 1) / kLitBlock)), dim3(kLitBlock), 0,
                       stream, S.nodes, S.isect, S.n_nodes, node_parent, tri_parent);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_skip_build, dim3((unsigned)((2 * S.ntri + kLitBlock - 1) / kLitBlock)), dim3(kLitBlock), 0,
                       stream, S, node_parent, tri_parent, words);
    return hipGetLastError();
}

// Rebuilds the occluder candidates of n_lights lights (cells entries each) on `stream`, after the
// lit bits they skip (lit_build on the same stream).
hipError_t occ_build(const DevScene& S, const uint32_t* tri_words, uint32_t cells, uint32_t words,
                     const DevLight* lights, int n_lights, const uint32_t* bits, int* occ, hipStream_t stream) {
    if (n_lights <= 0 || cells == 0) return hipSuccess;
    const uint64_t n = (uint64_t)cells * (uint64_t)n_lights;
    hipLaunchKernelGGL(k_occ_build, dim3((unsigned)((n + kLitBlock - 1) / kLitBlock)), dim3(kLitBlock), 0, stream, S,
                       tri_words, cells, words, lights, n_lights, bits, occ);
    return hipGetLastError();
}

// Clears and rebuilds the bits of n_lights lights (words 32-bit words each) on `stream`; diag: the
// scene box's diagonal (lit_margin_cell).
hipError_t lit_build(const DevScene& S, const uint32_t* tri_words, uint32_t cells, uint32_t words,
                     const DevLight* lights, int n_lights, uint32_t* bits, float diag, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(bits, 0, sizeof(uint32_t) * (size_t)words * (size_t)n_lights, stream);
    if (e != hipSuccess || n_lights <= 0) return e;
    const uint64_t n = (uint64_t)cells * (uint64_t)n_lights;
    hipLaunchKernelGGL(k_lit_build, dim3((unsigned)((n + kLitBlock - 1) / kLitBlock)), dim3(kLitBlock), 0, stream, S,
                       tri_words, cells, words, lights, n_lights, bits, diag);
    return hipGetLastError();
}

}  // namespace pt
