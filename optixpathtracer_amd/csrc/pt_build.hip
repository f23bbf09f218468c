// pt_build.hip — BVH construction on gfx950 (replaces optixAccelBuild + compaction,
// Renderer/OptiX/OptixRenderer.cpp:306-456 of Damo12320/OptixPathtracer).
//
//   1. k_morton   : per triangle AABB centroid -> 30-bit Morton key (10 bits/axis)
//   2. radix sort : (key, triangle) pairs, hipCUB device radix sort
//   3. k_gather   : triangle records into leaf order (isect: v0,e1,e2; shade: v1,v2,normals);
//                   level 0 of an AABB sparse table over the sorted leaves
//   4. k_sparse   : sparse-table level l = union of two level l-1 boxes (log2 N launches)
//   5. k_karras   : binary LBVH, one thread per internal node (Karras 2012 split search);
//                   each node's AABB = O(1) sparse-table range query over its leaf range
//   6. SAH-optimal BVH4 collapse: a bottom-up dynamic programme (k_sah_dp) picks every binary
//                   node's cheapest cover by 1-4 BVH4 children, a top-down pass replays it one
//                   BVH4 level at a time (k_collapse_count -> scan -> k_collapse_emit), numbering
//                   the nodes breadth-first by a prefix sum: the node array is the same on every
//                   build (no atomic slot order), and the top levels are a contiguous prefix.
// Steps 1-5 are the Karras LBVH front end.  bvh_build runs one of four front ends, each of which
// leaves a binary tree (BinaryTree) and the triangle records in leaf order, and then the one back
// end, step 6.  The other front ends: PLOC below, the host binned-SAH tree (pt_sah.cpp) and the same
// tree built on the GPU (pt_sah_gpu.hip), which is the default.  Every stage's scratch is a set of
// DevBufs of its own; bvh_build holds them so that they are freed after the timed window.
// PLOC builder (Meister & Bittner 2018, "Parallel Locally-Ordered Clustering for Bounding
// Volume Hierarchy Construction"): starting from the Morton-sorted leaves, each
// iteration finds every cluster's nearest neighbour (smallest merged surface area) within
// +-kPlocRadius positions, merges mutual pairs and compacts (hipCUB scan).  A top-down pass
// then numbers the leaves in depth-first order, so every subtree is again a contiguous
// leaf range, and the same collapse turns it into BVH4.  Its SAH quality is close to a
// full sweep build, which cuts traversal steps against the Karras tree.
// Apart from the DP's bottom-up hand-off, every kernel reads only what earlier launches wrote.
// The build is deterministic: the same scene gives the same node and triangle arrays bit for
// bit (tests/test_gpu_parity.py::test_bvh_build_deterministic).  The sparse
// table costs N*log2(N)*32 B (~150 MB at 250k triangles) — trivial against 288 GB HBM.
#include <hipcub/hipcub.hpp>

#include <vector>

#include "pt_internal.h"
#include "pt_resource.h"

namespace pt {

namespace {

__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__device__ __forceinline__ void tri_box(const float4* tri, int i, float lo[3], float hi[3]) {
    float4 a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    lo[0] = fminf(fminf(a.x, b.x), c.x);
    lo[1] = fminf(fminf(a.y, b.y), c.y);
    lo[2] = fminf(fminf(a.z, b.z), c.z);
    hi[0] = fmaxf(fmaxf(a.x, b.x), c.x);
    hi[1] = fmaxf(fmaxf(a.y, b.y), c.y);
    hi[2] = fmaxf(fmaxf(a.z, b.z), c.z);
}

// The box the traversal's hit-acceptance rule uses for triangle i (pt_device.h tri_accept): the
// vertices as the hit test sees them (v0, v0 + (v1 - v0), v0 + (v2 - v0)), padded.  The boxes
// stored in the BVH4 nodes are exact unions of these (k_sah_dp's refit), so they contain every
// acceptance box bit for bit; the tree itself (PLOC clustering, SAH choices) is built on the
// plain triangle boxes.
__device__ __forceinline__ void tri_box_accept(const float4* tri, int i, float lo[3], float hi[3]) {
    const float4 a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    const f3 v0 = mk(a.x, a.y, a.z);
    tri_box_padded(v0, mk(b.x - a.x, b.y - a.y, b.z - a.z), mk(c.x - a.x, c.y - a.y, c.z - a.z), lo, hi);
}

__global__ void k_morton(const float4* tri, int n, float3 cmin, float3 cinv, uint32_t* keys, uint32_t* vals) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float lo[3], hi[3];
    tri_box(tri, i, lo, hi);
    float cx = (0.5f * (lo[0] + hi[0]) - cmin.x) * cinv.x;
    float cy = (0.5f * (lo[1] + hi[1]) - cmin.y) * cinv.y;
    float cz = (0.5f * (lo[2] + hi[2]) - cmin.z) * cinv.z;
    uint32_t qx = (uint32_t)fminf(fmaxf(cx * 1024.0f, 0.0f), 1023.0f);
    uint32_t qy = (uint32_t)fminf(fmaxf(cy * 1024.0f, 0.0f), 1023.0f);
    uint32_t qz = (uint32_t)fminf(fmaxf(cz * 1024.0f, 0.0f), 1023.0f);
    keys[i] = (expand_bits(qx) << 2) | (expand_bits(qy) << 1) | expand_bits(qz);
    vals[i] = (uint32_t)i;
}

// Leaf-order gather.  isect: v0|orig, (v1-v0)|material, (v2-v0)|alpha flag — the edge subtraction
// is the same single fp32 op the oracle performs, so the hit arithmetic stays identical.
// shade: v1|n0.x, v2|n0.y, n0.z n1, n2|material.
__global__ void k_gather(const float4* tri_orig, const float4* nrm_orig, const float4* uv_orig, const uint32_t* order,
                         int n, float4* isect, float4* shade, float4* tuv, float4* st0, float4* pleaf) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int i = (int)order[k];
    const float4 a = tri_orig[3 * i], b = tri_orig[3 * i + 1], c = tri_orig[3 * i + 2];
    const float4 na = nrm_orig[3 * i], nb = nrm_orig[3 * i + 1], nc = nrm_orig[3 * i + 2];
    isect[3 * k] = a;
    isect[3 * k + 1] = make_float4(b.x - a.x, b.y - a.y, b.z - a.z, b.w);
    isect[3 * k + 2] = make_float4(c.x - a.x, c.y - a.y, c.z - a.z, c.w);  // w: alpha-cut-out flag
    if (tuv) {
        tuv[2 * k] = uv_orig[2 * i];
        tuv[2 * k + 1] = uv_orig[2 * i + 1];
    }
    shade[4 * k] = make_float4(b.x, b.y, b.z, na.x);
    shade[4 * k + 1] = make_float4(c.x, c.y, c.z, na.y);
    shade[4 * k + 2] = make_float4(na.z, nb.x, nb.y, nb.z);
    shade[4 * k + 3] = make_float4(nc.x, nc.y, nc.z, b.w);  // w: material (as isect's e1.w) for reconstruct
    float lo[3], hi[3];
    tri_box(tri_orig, i, lo, hi);
    st0[2 * k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    st0[2 * k + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    tri_box_accept(tri_orig, i, lo, hi);
    pleaf[2 * k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    pleaf[2 * k + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
}

__global__ void k_sparse(const float4* prev, float4* cur, int count, int half) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float4 a0 = prev[2 * i], a1 = prev[2 * i + 1];
    float4 b0 = prev[2 * (i + half)], b1 = prev[2 * (i + half) + 1];
    cur[2 * i] = make_float4(fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z), 0.0f);
    cur[2 * i + 1] = make_float4(fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y), fmaxf(a1.z, b1.z), 0.0f);
}

struct SparseTable {
    const float4* level[32];
    int n;
};

__device__ __forceinline__ void range_box(const SparseTable& st, int a, int b, float4& lo, float4& hi) {
    int len = b - a + 1;
    int l = 31 - __clz(len);
    const float4* L = st.level[l];
    int c = b - (1 << l) + 1;
    float4 a0 = L[2 * a], a1 = L[2 * a + 1], b0 = L[2 * c], b1 = L[2 * c + 1];
    lo = make_float4(fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z), 0.0f);
    hi = make_float4(fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y), fmaxf(a1.z, b1.z), 0.0f);
}

__device__ __forceinline__ int delta(const uint32_t* keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    uint32_t ki = keys[i], kj = keys[j];
    if (ki == kj) return 32 + __clz((uint32_t)i ^ (uint32_t)j);
    return __clz(ki ^ kj);
}

// Binary LBVH node i: child codes (>= 0 internal, < 0 leaf ~k), leaf range, AABB.
__global__ void k_karras(const uint32_t* keys, int n, SparseTable st, int2* bchild, int2* brange, float4* bbox) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    int dmin = delta(keys, n, i, i - d);
    int lmax = 2;
    while (delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    int j = i + l * d;
    int dnode = delta(keys, n, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    int gamma = i + s * d + (d < 0 ? -1 : 0);
    int first = min(i, j), last = max(i, j);
    int c0 = (first == gamma) ? ~gamma : gamma;
    int c1 = (last == gamma + 1) ? ~(gamma + 1) : (gamma + 1);
    bchild[i] = make_int2(c0, c1);
    brange[i] = make_int2(first, last);
    float4 lo, hi;
    range_box(st, first, last, lo, hi);
    bbox[2 * i] = lo;
    bbox[2 * i + 1] = hi;
}

struct BinTree {
    const int2* child;
    const int2* range;
    const float4* box;  // internal node boxes (2 per node)
    const float4* leafbox;  // sparse table level 0 (2 per leaf)
    const float4* pleaf;  // padded acceptance box per leaf (2 per leaf)
    float4* pbox;         // union of the padded leaf boxes per internal node (k_sah_dp)
};
// Node box for the BVH4: the exact union of the padded acceptance boxes below `code`.
__device__ __forceinline__ void code_box_padded(const BinTree& B, int code, float4& lo, float4& hi) {
    if (code >= 0) {
        lo = B.pbox[2 * code];
        hi = B.pbox[2 * code + 1];
    } else {
        lo = B.pleaf[2 * ~code];
        hi = B.pleaf[2 * ~code + 1];
    }
}

__device__ __forceinline__ void code_box(const BinTree& B, int code, float4& lo, float4& hi) {
    if (code >= 0) {
        lo = B.box[2 * code];
        hi = B.box[2 * code + 1];
    } else {
        lo = B.leafbox[2 * ~code];
        hi = B.leafbox[2 * ~code + 1];
    }
}
__device__ __forceinline__ int code_count(const BinTree& B, int code) {
    if (code < 0) return 1;
    int2 r = B.range[code];
    return r.y - r.x + 1;
}
__device__ __forceinline__ int code_first(const BinTree& B, int code) { return code < 0 ? ~code : B.range[code].x; }
__device__ __forceinline__ float half_area(float4 lo, float4 hi) {
    float x = hi.x - lo.x, y = hi.y - lo.y, z = hi.z - lo.z;
    return x * y + y * z + z * x;
}
// ---- SAH-optimal BVH4 collapse -------------------------------------------------------------
// Bottom-up dynamic programme over the binary tree (the wide-BVH collapse of Ylitie, Karras &
// Laine 2017, "Efficient Incoherent Ray Traversal on GPUs Through Compressed Wide BVHs",
// for 4-wide nodes): cost[n][j] = cheapest SAH cost of covering subtree n with at most j
// BVH4 children, each one a BVH4 node or a leaf of <= kSahLeafMax consecutive triangles:
//   single(n)  = min(A(n) * cTri * count(n)            [leaf, count <= kSahLeafMax],
//                   A(n) * cNode + min_a cost[L][a] + cost[R][4 - a])   [BVH4 node]
//   cost[n][1] = single(n);  cost[n][j] = min(single(n), min_a cost[L][a] + cost[R][j - a])
// The top-down k_collapse_sah then replays the recorded choices.  kSahCNode and kSahCTri:
// pt_internal.h.
#ifndef PT_SAH_LEAF_MAX
#define PT_SAH_LEAF_MAX 4
#endif
constexpr int kSahLeafMax = PT_SAH_LEAF_MAX;
static_assert(kSahLeafMax >= 1 && kSahLeafMax <= 8, "leaf count is encoded in 3 bits");

// Decision word of an internal node: bits 2(j-2)..2(j-2)+1 for j = 2..4 = left pieces a of the
// best split into j (0 = keep single); bits 6..7 = left pieces of the node's own 4-way split;
// bit 8 = single is a leaf.
__device__ __forceinline__ int dp_split(int dec, int j) { return (dec >> (2 * (j - 2))) & 3; }
__device__ __forceinline__ int dp_node_split(int dec) { return (dec >> 6) & 3; }
__device__ __forceinline__ bool dp_is_leaf(int dec) { return (dec >> 8) & 1; }

__global__ void k_parents(const int2* bchild, int nb, int* parent, int* leafparent) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const int2 c = bchild[i];
    if (c.x >= 0) parent[c.x] = i; else leafparent[~c.x] = i;
    if (c.y >= 0) parent[c.y] = i; else leafparent[~c.y] = i;
}

__device__ __forceinline__ float4 dp_load(const float4* p) {
    const float* f = reinterpret_cast<const float*>(p);
    return make_float4(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                       __hip_atomic_load(f + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                       __hip_atomic_load(f + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                       __hip_atomic_load(f + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// One thread per triangle walks up; the second child to finish computes the parent (the
// usual bottom-up refit hand-off through a per-node arrival counter).
__global__ void k_sah_dp(BinTree B, int n, const int* parent, const int* leafparent, int* visits, float4* dpc,
                         int* dpd) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int node = leafparent[t];
    while (node >= 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (atomicAdd(&visits[node], 1) == 0) return;  // the sibling subtree is not done yet
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int2 ch = B.child[node];
        float cl[5], cr[5];
        float4 plo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), phi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
        const int kids[2] = {ch.x, ch.y};
        for (int k = 0; k < 2; ++k) {
            float* c = k == 0 ? cl : cr;
            const int code = kids[k];
            float4 klo, khi;  // the child's padded box
            if (code < 0) {  // one triangle: always a leaf
                float4 lo = B.leafbox[2 * ~code], hi = B.leafbox[2 * ~code + 1];
                float v = half_area(lo, hi) * kSahCTri;
                c[1] = c[2] = c[3] = c[4] = v;
                klo = B.pleaf[2 * ~code];
                khi = B.pleaf[2 * ~code + 1];
            } else {
                float4 v = dp_load(dpc + code);
                c[1] = v.x; c[2] = v.y; c[3] = v.z; c[4] = v.w;
                klo = dp_load(B.pbox + 2 * code);
                khi = dp_load(B.pbox + 2 * code + 1);
            }
            plo = make_float4(fminf(plo.x, klo.x), fminf(plo.y, klo.y), fminf(plo.z, klo.z), 0.0f);
            phi = make_float4(fmaxf(phi.x, khi.x), fmaxf(phi.y, khi.y), fmaxf(phi.z, khi.z), 0.0f);
        }
        B.pbox[2 * node] = plo;
        B.pbox[2 * node + 1] = phi;
        const float area = half_area(B.box[2 * node], B.box[2 * node + 1]);
        const int2 r = B.range[node];
        const int count = r.y - r.x + 1;
        const float inf = __int_as_float(0x7f800000);
        float best4 = inf;
        int a4 = 1;
        for (int a = 1; a <= 3; ++a) {
            const float v = cl[a] + cr[4 - a];
            if (v < best4) { best4 = v; a4 = a; }
        }
        const float node_cost = area * kSahCNode + best4;
        const float leaf_cost = count <= kSahLeafMax ? area * kSahCTri * (float)count : inf;
        const bool leaf = leaf_cost <= node_cost;
        const float single = leaf ? leaf_cost : node_cost;
        float out[5];
        int dec = (a4 << 6) | (leaf ? 256 : 0);
        out[1] = single;
        for (int j = 2; j <= 4; ++j) {
            float bj = single;
            int aj = 0;
            for (int a = 1; a < j; ++a) {
                const float v = cl[a] + cr[j - a];
                if (v < bj) { bj = v; aj = a; }
            }
            out[j] = bj;
            dec |= aj << (2 * (j - 2));
        }
        dpc[node] = make_float4(out[1], out[2], out[3], out[4]);
        dpd[node] = dec;
        node = parent[node];
    }
}

// Children of one BVH4 node (work item: binary code) from the DP choices, in DFS order of the
// binary tree; returns the count (1..4).
__device__ __forceinline__ int collapse_children(const BinTree& B, const int* dpd, int code, int c[4]) {
    int n = 0;
    if (code < 0) {  // degenerate scene: the root is a single leaf
        c[n++] = code;
        return n;
    }
    int st_code[8], st_j[8], sp = 0;
    const int2 ch = B.child[code];
    const int a = dp_node_split(dpd[code]);
    st_code[sp] = ch.y; st_j[sp++] = 4 - a;
    st_code[sp] = ch.x; st_j[sp++] = a;
    while (sp > 0) {
        --sp;
        const int x = st_code[sp], j = st_j[sp];
        const int s = (x < 0 || j < 2) ? 0 : dp_split(dpd[x], j);
        if (s == 0) {
            c[n++] = x;
        } else {
            const int2 xc = B.child[x];
            st_code[sp] = xc.y; st_j[sp++] = j - s;
            st_code[sp] = xc.x; st_j[sp++] = s;
        }
    }
    return n;
}
__device__ __forceinline__ bool child_is_leaf(const BinTree& B, const int* dpd, int code) {
    return code < 0 || dp_is_leaf(dpd[code]);
}

// Top-down collapse, one BVH4 level per launch pair.  k_collapse_count: inner (non-leaf)
// children per work item; an exclusive scan of the counts gives every inner child its slot
// (level base + offset) and its position in the next level's work list, so the numbering is
// breadth-first and the same on every build.
__global__ void k_collapse_count(BinTree B, const int* dpd, const int* work, int nwork, int* cnt) {
    int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwork) return;
    int c[4];
    const int n = collapse_children(B, dpd, work[w], c);
    int inner = 0;
    for (int k = 0; k < n; ++k) inner += child_is_leaf(B, dpd, c[k]) ? 0 : 1;
    cnt[w] = inner;
}

// k_collapse_emit: node of work item w goes to slot level_base + w (the parent assigned it
// in this order), its inner children to next_base + off[w] + j.
__global__ void k_collapse_emit(BinTree B, const int* dpd, const int* work, int nwork, const int* off,
                                int level_base, int next_base, BNode4* out, int* next) {
    int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwork) return;
    int c[4];
    const int n = collapse_children(B, dpd, work[w], c);
    float lo[3][4], hi[3][4];
    int cc[4];
    int j = off[w];
    for (int k = 0; k < 4; ++k) {
        if (k >= n) {
            cc[k] = kEmptyChild;
            // inverted box: misses for every ray direction (the sign-selected slab test of
            // pt_device.h node_eval relies on it instead of testing the child id)
            for (int a = 0; a < 3; ++a) {
                lo[a][k] = __int_as_float(0x7f800000);
                hi[a][k] = -__int_as_float(0x7f800000);
            }
            continue;
        }
        float4 l4, h4;  // the exact union of the padded acceptance boxes below the child
        code_box_padded(B, c[k], l4, h4);
        lo[0][k] = l4.x; lo[1][k] = l4.y; lo[2][k] = l4.z;
        hi[0][k] = h4.x; hi[1][k] = h4.y; hi[2][k] = h4.z;
        if (child_is_leaf(B, dpd, c[k])) {
            cc[k] = ~((code_first(B, c[k]) << 3) | (code_count(B, c[k]) - 1));
        } else {
            cc[k] = next_base + j;
            next[j] = c[k];
            ++j;
        }
    }
    BNode4 nd;
    nd.lox = make_float4(lo[0][0], lo[0][1], lo[0][2], lo[0][3]);
    nd.hix = make_float4(hi[0][0], hi[0][1], hi[0][2], hi[0][3]);
    nd.loy = make_float4(lo[1][0], lo[1][1], lo[1][2], lo[1][3]);
    nd.hiy = make_float4(hi[1][0], hi[1][1], hi[1][2], hi[1][3]);
    nd.loz = make_float4(lo[2][0], lo[2][1], lo[2][2], lo[2][3]);
    nd.hiz = make_float4(hi[2][0], hi[2][1], hi[2][2], hi[2][3]);
    nd.child = make_int4(cc[0], cc[1], cc[2], cc[3]);
    nd.pad = make_int4(0, 0, 0, 0);
    out[level_base + w] = nd;
}

// ---- PLOC ---------------------------------------------------------------------------------
#ifndef PT_PLOC_RADIUS
#define PT_PLOC_RADIUS 8
#endif
constexpr int kPlocRadius = PT_PLOC_RADIUS;

__device__ __forceinline__ float merged_area(float4 alo, float4 ahi, float4 blo, float4 bhi) {
    float x = fmaxf(ahi.x, bhi.x) - fminf(alo.x, blo.x);
    float y = fmaxf(ahi.y, bhi.y) - fminf(alo.y, blo.y);
    float z = fmaxf(ahi.z, bhi.z) - fminf(alo.z, blo.z);
    return x * y + y * z + z * x;
}

// Leaf boxes in Morton order.
__global__ void k_leafbox(const float4* tri_orig, const uint32_t* order, int n, float4* box, int* code, int* cnt) {
    int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    float lo[3], hi[3];
    tri_box(tri_orig, (int)order[m], lo, hi);
    box[2 * m] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    box[2 * m + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    code[m] = ~m;
    cnt[m] = 1;
}

// Nearest neighbour of every cluster within the window.  Ties go to the lower position,
// which makes the globally best pair mutual (progress every iteration).
__global__ void k_ploc_nn(const float4* box, int n, int* nn) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 lo = box[2 * i], hi = box[2 * i + 1];
    unsigned long long best = ~0ull;
    const int a = max(0, i - kPlocRadius), b = min(n - 1, i + kPlocRadius);
    for (int j = a; j <= b; ++j) {
        if (j == i) continue;
        float c = merged_area(lo, hi, box[2 * j], box[2 * j + 1]);
        unsigned long long key = ((unsigned long long)__float_as_uint(c) << 32) | (unsigned)j;
        best = key < best ? key : best;
    }
    nn[i] = (int)(best & 0xffffffffu);
}

// flags: low 32 bits = cluster survives, high 32 bits = cluster creates a node.
__global__ void k_ploc_flags(const int* nn, int n, unsigned long long* flags) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = nn[i];
    const bool mutual = n > 1 && nn[j] == i;
    const bool keep = !(mutual && i > j);
    const bool merge = mutual && i < j;
    flags[i] = ((unsigned long long)(merge ? 1 : 0) << 32) | (keep ? 1ull : 0ull);
}

__global__ void k_ploc_compact(const float4* box, const int* code, const int* cnt, const int* nn,
                               const unsigned long long* scan, const unsigned long long* flags, int n,
                               int node_base, float4* obox, int* ocode, int* ocnt, int2* bchild, float4* bbox,
                               int* bcount) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long f = flags[i];
    if (!(f & 1ull)) return;
    const unsigned long long sc = scan[i];
    const int pos = (int)(sc & 0xffffffffu);
    float4 lo = box[2 * i], hi = box[2 * i + 1];
    int c = code[i], k = cnt[i];
    if (f >> 32) {
        const int j = nn[i];
        const float4 lj = box[2 * j], hj = box[2 * j + 1];
        lo = make_float4(fminf(lo.x, lj.x), fminf(lo.y, lj.y), fminf(lo.z, lj.z), 0.0f);
        hi = make_float4(fmaxf(hi.x, hj.x), fmaxf(hi.y, hj.y), fmaxf(hi.z, hj.z), 0.0f);
        const int node = node_base + (int)(sc >> 32);
        bchild[node] = make_int2(c, code[j]);
        bbox[2 * node] = lo;
        bbox[2 * node + 1] = hi;
        bcount[node] = k + cnt[j];
        c = node;
        k += cnt[j];
    }
    obox[2 * pos] = lo;
    obox[2 * pos + 1] = hi;
    ocode[pos] = c;
    ocnt[pos] = k;
}

// Depth-first leaf numbering, one launch per tree level: item = (node, first leaf).  Writes
// the node's leaf range, rewrites leaf child codes from Morton positions to DFS positions
// and records the triangle order.
__global__ void k_ploc_dfs(const int2* work, int nwork, int2* bchild, const int* bcount, int2* brange,
                           const uint32_t* morton_order, uint32_t* dfs_order, int2* next, int* nnext) {
    int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwork) return;
    const int2 it = work[w];
    const int node = it.x, first = it.y;
    brange[node] = make_int2(first, first + bcount[node] - 1);
    int2 ch = bchild[node];
    int c[2] = {ch.x, ch.y};
    int f = first;
    for (int k = 0; k < 2; ++k) {
        if (c[k] < 0) {
            dfs_order[f] = morton_order[~c[k]];
            c[k] = ~f;
            f += 1;
        } else {
            int q = atomicAdd(nnext, 1);
            next[q] = make_int2(c[k], f);
            f += bcount[c[k]];
        }
    }
    bchild[node] = make_int2(c[0], c[1]);
}

inline unsigned grid_for(int n, int b) { return (unsigned)((n + b - 1) / b); }

__global__ void k_ploc_total(const unsigned long long* scan, const unsigned long long* flags, int n, int* out) {
    const unsigned long long t = scan[n - 1] + flags[n - 1];
    out[0] = (int)(t & 0xffffffffu);  // surviving clusters
    out[1] = (int)(t >> 32);          // nodes created
}

// hipCUB temp storage: at least 16 bytes, since a computed size can be 0.
hipError_t alloc_temp(DevBuf<unsigned char>& temp, size_t bytes) { return temp.alloc(bytes > 0 ? bytes : 16); }

// The device arrays a BinTree points into and the binary root code (node 0, or ~0 when the one
// triangle is the root).  A front end fills everything but pbox, which the back end adds.
struct BinaryTree {
    DevBuf<int2> child, range;
    DevBuf<float4> box, leafbox, pleaf, pbox;
    int root = 0;
    BinTree view() const { return BinTree{child, range, box, leafbox, pleaf, pbox}; }
    // n - 1 internal nodes (one slot at n = 1) and n leaves; `leafboxes`: float4 pairs in leafbox
    hipError_t alloc(int n, size_t leafboxes) {
        const size_t nbin = n > 1 ? n - 1 : 1;
        return first_error({child.alloc(nbin), range.alloc(nbin), box.alloc(2 * nbin), leafbox.alloc(2 * leafboxes),
                            pleaf.alloc(2 * (size_t)n)});
    }
};

// Every front end's last step on the triangles: the records in leaf order into `out`, the leaves'
// plain and padded boxes into the tree.
hipError_t gather_leaves(const BuildInput& in, const uint32_t* order, BuildOutput& out, BinaryTree& T,
                         hipStream_t stream) {
    hipLaunchKernelGGL(k_gather, dim3(grid_for(in.n, 256)), dim3(256), 0, stream, in.tri_orig, in.nrm_orig, in.uv_orig,
                       order, in.n, out.isect, out.shade, out.tuv, T.leafbox.get(), T.pleaf.get());
    return hipGetLastError();
}

// Morton keys of the triangles and the triangles sorted by them: what the LBVH and PLOC front
// ends start from.
struct MortonOrder {
    DevBuf<uint32_t> keys, vals, keys2, vals2;  // keys2 / vals2: the sorted keys and their triangles
    DevBuf<unsigned char> temp;
    size_t temp_bytes = 0;
    hipError_t alloc(int n, hipStream_t stream) {
        hipError_t err = first_error({keys.alloc(n), vals.alloc(n), keys2.alloc(n), vals2.alloc(n)});
        if (err != hipSuccess) return err;
        err = hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, keys.get(), keys2.get(), vals.get(), vals2.get(),
                                                 n, 0, 30, stream);
        return err != hipSuccess ? err : alloc_temp(temp, temp_bytes);
    }
    hipError_t sort(const BuildInput& in, hipStream_t stream) {
        const int n = in.n;
        float3 cmin = make_float3(in.cmin[0], in.cmin[1], in.cmin[2]);
        float ex = in.cmax[0] - in.cmin[0], ey = in.cmax[1] - in.cmin[1], ez = in.cmax[2] - in.cmin[2];
        float3 cinv = make_float3(ex > 0.0f ? 1.0f / ex : 0.0f, ey > 0.0f ? 1.0f / ey : 0.0f,
                                  ez > 0.0f ? 1.0f / ez : 0.0f);
        hipLaunchKernelGGL(k_morton, dim3(grid_for(n, 256)), dim3(256), 0, stream, in.tri_orig, n, cmin, cinv,
                           keys.get(), vals.get());
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
        return hipcub::DeviceRadixSort::SortPairs(temp.get(), temp_bytes, keys.get(), keys2.get(), vals.get(),
                                                  vals2.get(), n, 0, 30, stream);
    }
};

// The front ends.  Each builds the binary tree of `in` into T and writes the triangle records in
// leaf order into `out`.  What it allocates before it records `start` is outside the build's
// timed window.  Its scratch is the caller's, empty on entry: bvh_build releases it after the stop
// event, because a hipFree waits for the device and takes its own time, both of which the window
// would count (at 10^6 triangles PLOC measured 15 ms instead of 10 with the frees inside).

// Karras 2012: the tree over the Morton-sorted triangles, boxes from a sparse table over the leaves
// (T.leafbox holds the whole table; level 0 is the leaf boxes).
hipError_t build_lbvh(const BuildInput& in, BuildOutput& out, hipStream_t stream, hipEvent_t start,
                      MortonOrder& morton, BinaryTree& T) {
    const int n = in.n;
    int levels = 1;
    while ((1 << levels) <= n) ++levels;  // levels 0..levels-1 with 2^l <= n
    hipError_t err;
    if ((err = first_error({morton.alloc(n, stream), T.alloc(n, (size_t)n * (size_t)levels)})) != hipSuccess)
        return err;
    if ((err = hipEventRecord(start, stream)) != hipSuccess) return err;
    if ((err = morton.sort(in, stream)) != hipSuccess) return err;
    if ((err = gather_leaves(in, morton.vals2, out, T, stream)) != hipSuccess) return err;
    SparseTable table{};
    float4* const st = T.leafbox;
    table.n = n;
    table.level[0] = st;
    for (int l = 1; l < levels; ++l) {
        float4* prev = st + 2 * (size_t)n * (size_t)(l - 1);
        float4* cur = st + 2 * (size_t)n * (size_t)l;
        int count = n - (1 << l) + 1;
        hipLaunchKernelGGL(k_sparse, dim3(grid_for(count, 256)), dim3(256), 0, stream, prev, cur, count, 1 << (l - 1));
        if ((err = hipGetLastError()) != hipSuccess) return err;
        table.level[l] = cur;
    }
    if (n > 1) {
        hipLaunchKernelGGL(k_karras, dim3(grid_for(n - 1, 256)), dim3(256), 0, stream, morton.keys2.get(), n, table,
                           T.child.get(), T.range.get(), T.box.get());
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    T.root = n > 1 ? 0 : ~0;
    return hipSuccess;
}

// PLOC's working set: the cluster arrays (two of each, read and written in turn), the iteration's
// neighbour / flag / scan arrays, the nodes' leaf counts, the DFS work lists and the DFS order.
struct PlocScratch {
    DevBuf<float4> box[2];
    DevBuf<int> code[2], ccnt[2], nn, bcount, tot;
    DevBuf<int2> work[2];
    DevBuf<unsigned long long> flags, scan;
    DevBuf<uint32_t> dfs;
    DevBuf<unsigned char> temp;
    size_t temp_bytes = 0;
    hipError_t alloc(int n, hipStream_t stream) {
        const size_t nb = n > 1 ? n - 1 : 1;
        hipError_t err = hipSuccess;
        for (int k = 0; k < 2 && err == hipSuccess; ++k)
            err = first_error({box[k].alloc(2 * (size_t)n), code[k].alloc(n), ccnt[k].alloc(n), work[k].alloc(n)});
        if (err == hipSuccess)
            err = first_error(
                {nn.alloc(n), flags.alloc(n), scan.alloc(n), bcount.alloc(nb), dfs.alloc(n), tot.alloc(2)});
        if (err == hipSuccess)
            err = hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, flags.get(), scan.get(), n, stream);
        return err != hipSuccess ? err : alloc_temp(temp, temp_bytes);
    }
};

// The PLOC iterations: nearest neighbours, mutual pairs merged into nodes, clusters compacted, until
// one cluster is left; *root = its code.  One host sync per iteration (the counts come from the device).
hipError_t ploc_cluster(const BuildInput& in, const uint32_t* morton_order, PlocScratch& S, BinaryTree& T,
                        hipStream_t stream, int* root) {
    const int n = in.n;
    hipError_t err;
    hipLaunchKernelGGL(k_leafbox, dim3(grid_for(n, 256)), dim3(256), 0, stream, in.tri_orig, morton_order, n,
                       S.box[0].get(), S.code[0].get(), S.ccnt[0].get());
    if ((err = hipGetLastError()) != hipSuccess) return err;
    int cur = 0, m = n, node_base = 0;
    while (m > 1) {
        hipLaunchKernelGGL(k_ploc_nn, dim3(grid_for(m, 256)), dim3(256), 0, stream, S.box[cur].get(), m, S.nn.get());
        hipLaunchKernelGGL(k_ploc_flags, dim3(grid_for(m, 256)), dim3(256), 0, stream, S.nn.get(), m, S.flags.get());
        if ((err = hipGetLastError()) != hipSuccess) return err;
        if ((err = hipcub::DeviceScan::ExclusiveSum(S.temp.get(), S.temp_bytes, S.flags.get(), S.scan.get(), m,
                                                    stream)) != hipSuccess)
            return err;
        hipLaunchKernelGGL(k_ploc_compact, dim3(grid_for(m, 256)), dim3(256), 0, stream, S.box[cur].get(),
                           S.code[cur].get(), S.ccnt[cur].get(), S.nn.get(), S.scan.get(), S.flags.get(), m, node_base,
                           S.box[cur ^ 1].get(), S.code[cur ^ 1].get(), S.ccnt[cur ^ 1].get(), T.child.get(),
                           T.box.get(), S.bcount.get());
        hipLaunchKernelGGL(k_ploc_total, dim3(1), dim3(1), 0, stream, S.scan.get(), S.flags.get(), m, S.tot.get());
        if ((err = hipGetLastError()) != hipSuccess) return err;
        int h[2] = {0, 0};
        if ((err = hipMemcpyAsync(h, S.tot, sizeof h, hipMemcpyDeviceToHost, stream)) != hipSuccess) return err;
        if ((err = hipStreamSynchronize(stream)) != hipSuccess) return err;
        if (h[1] <= 0) return hipErrorUnknown;  // cannot happen: the best pair is always mutual
        m = h[0];
        node_base += h[1];
        cur ^= 1;
    }
    if ((err = hipMemcpyAsync(root, S.code[cur], sizeof(int), hipMemcpyDeviceToHost, stream)) != hipSuccess) return err;
    return hipStreamSynchronize(stream);
}

// Depth-first leaf numbering from the root node `rc`, one launch and one host sync per tree level:
// every subtree becomes a contiguous leaf range, S.dfs the triangle of every leaf.
hipError_t ploc_number(int rc, const uint32_t* morton_order, PlocScratch& S, BinaryTree& T, hipStream_t stream) {
    hipError_t err;
    int2 w0 = make_int2(rc, 0);
    int nwork = 1, c = 0;
    int* nnext = S.tot;
    if ((err = hipMemcpyAsync(S.work[0], &w0, sizeof(int2), hipMemcpyHostToDevice, stream)) != hipSuccess) return err;
    while (nwork > 0) {
        if ((err = hipMemsetAsync(nnext, 0, sizeof(int), stream)) != hipSuccess) return err;
        hipLaunchKernelGGL(k_ploc_dfs, dim3(grid_for(nwork, 128)), dim3(128), 0, stream, S.work[c].get(), nwork,
                           T.child.get(), S.bcount.get(), T.range.get(), morton_order, S.dfs.get(), S.work[c ^ 1].get(),
                           nnext);
        if ((err = hipGetLastError()) != hipSuccess) return err;
        if ((err = hipMemcpyAsync(&nwork, nnext, sizeof(int), hipMemcpyDeviceToHost, stream)) != hipSuccess) return err;
        if ((err = hipStreamSynchronize(stream)) != hipSuccess) return err;
        c ^= 1;
    }
    return hipSuccess;
}

// PLOC (Meister & Bittner 2018) over the Morton-sorted triangles.  Also the SAH builders' tree of a
// single triangle.
hipError_t build_ploc(const BuildInput& in, BuildOutput& out, hipStream_t stream, hipEvent_t start,
                      MortonOrder& morton, PlocScratch& S, BinaryTree& T) {
    const int n = in.n;
    hipError_t err;
    if ((err = morton.alloc(n, stream)) != hipSuccess) return err;
    if ((err = hipEventRecord(start, stream)) != hipSuccess) return err;
    if ((err = morton.sort(in, stream)) != hipSuccess) return err;
    if ((err = first_error({S.alloc(n, stream), T.alloc(n, n)})) != hipSuccess) return err;
    int rc = ~0;
    if ((err = ploc_cluster(in, morton.vals2, S, T, stream, &rc)) != hipSuccess) return err;
    if (rc < 0) {  // single triangle
        err = hipMemcpyAsync(S.dfs, morton.vals2, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
        T.root = ~0;
    } else {
        err = ploc_number(rc, morton.vals2, S, T, stream);
        T.root = rc;
    }
    if (err != hipSuccess) return err;
    return gather_leaves(in, S.dfs, out, T, stream);
}

// The SAH front ends' common end: with the tree's nodes and the DFS triangle order `dfs` on the
// device, the leaf gather; then a host sync, after which the caller's host arrays may go.
hipError_t finish_sah(const BuildInput& in, const uint32_t* dfs, BuildOutput& out, BinaryTree& T, hipStream_t stream) {
    const hipError_t err = gather_leaves(in, dfs, out, T, stream);
    if (err != hipSuccess) return err;
    T.root = 0;
    return hipStreamSynchronize(stream);
}

// Host binned SAH (pt_sah.cpp), n >= 2: the tree is built on the host and uploaded.
hipError_t build_sah_host(const BuildInput& in, BuildOutput& out, hipStream_t stream, hipEvent_t start,
                          DevBuf<uint32_t>& dfs, BinaryTree& T) {
    const int n = in.n;
    const size_t nbin = (size_t)n - 1;
    hipError_t err;
    if ((err = hipEventRecord(start, stream)) != hipSuccess) return err;
    std::vector<uint32_t> order;
    std::vector<int2> hchild, hrange;
    std::vector<float4> hbox;
    sah_binary_tree(in.tri_host, n, order, hchild, hrange, hbox);
    if (PT_SAH_REINSERT > 0) {
        // kept only when it cuts the binary tree's cost by 2 % or more: Sponza-class 8.9 % ->
        // +0.5 % Msamples/s; the sphere box 0.13 % -> one level deeper and -1.1 to -1.6 %
        // (profiles/r04u_ab_reinsert_sponza.log)
        std::vector<uint32_t> order2 = order;
        std::vector<int2> child2 = hchild, range2 = hrange;
        std::vector<float4> box2 = hbox;
        if (sah_reinsert(order2, child2, range2, box2, in.tri_host, PT_SAH_REINSERT) >= 0.02) {
            order.swap(order2);
            hchild.swap(child2);
            hrange.swap(range2);
            hbox.swap(box2);
        }
    }
    if ((err = first_error({dfs.alloc(n), T.alloc(n, n)})) != hipSuccess) return err;
    if ((err = first_error(
             {hipMemcpyAsync(dfs, order.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, stream),
              hipMemcpyAsync(T.child, hchild.data(), sizeof(int2) * nbin, hipMemcpyHostToDevice, stream),
              hipMemcpyAsync(T.range, hrange.data(), sizeof(int2) * nbin, hipMemcpyHostToDevice, stream),
              hipMemcpyAsync(T.box, hbox.data(), sizeof(float4) * 2 * nbin, hipMemcpyHostToDevice, stream)})) !=
        hipSuccess)
        return err;
    return finish_sah(in, dfs, out, T, stream);
}

// The same tree built on the GPU (pt_sah_gpu.hip), n >= 2.
hipError_t build_sah_gpu(const BuildInput& in, BuildOutput& out, hipStream_t stream, hipEvent_t start,
                         DevBuf<uint32_t>& dfs, BinaryTree& T) {
    const int n = in.n;
    hipError_t err;
    if ((err = hipEventRecord(start, stream)) != hipSuccess) return err;
    if ((err = first_error({dfs.alloc(n), T.alloc(n, n)})) != hipSuccess) return err;
    if ((err = sah_build_gpu(in.tri_orig, n, dfs, T.child, T.range, T.box, stream)) != hipSuccess) return err;
    return finish_sah(in, dfs, out, T, stream);
}

// The back end's scratch: the level-by-level work lists and the scan's storage, allocated before
// the timed window, and the SAH dynamic programme's arrays, allocated inside it (alloc_dp).
// bvh_build releases all of it after the stop event, as it does the front ends' scratch.
struct CollapseScratch {
    DevBuf<int> work, work2, wcnt, woff;
    DevBuf<unsigned char> temp;
    size_t temp_bytes = 0;
    DevBuf<int> parent, leafparent, visits, dec;
    DevBuf<float4> cost;
    hipError_t alloc(int n, hipStream_t stream) {
        hipError_t err = first_error({work.alloc(n), work2.alloc(n), wcnt.alloc(n), woff.alloc(n)});
        if (err != hipSuccess) return err;
        err = hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, wcnt.get(), woff.get(), n, stream);
        return err != hipSuccess ? err : alloc_temp(temp, temp_bytes);
    }
    hipError_t alloc_dp(int n, BinaryTree& T) {
        const size_t nbin = (size_t)n - 1;
        return first_error({parent.alloc(nbin), leafparent.alloc(n), visits.alloc(nbin), cost.alloc(nbin),
                            dec.alloc(nbin), T.pbox.alloc(2 * nbin)});
    }
};

// The back end, part 1: k_sah_dp picks every binary node's cheapest cover by 1-4 BVH4 children
// (C.dec) and fills T.pbox.  Nothing to do for the tree of a single leaf: C.dec stays empty.
hipError_t sah_dp(BinaryTree& T, int n, CollapseScratch& C, hipStream_t stream) {
    if (T.root < 0) return hipSuccess;
    const int nbin = n - 1;
    hipError_t err;
    if ((err = C.alloc_dp(n, T)) != hipSuccess) return err;
    if ((err = hipMemsetAsync(C.visits, 0, sizeof(int) * nbin, stream)) != hipSuccess) return err;
    if ((err = hipMemsetAsync(C.parent, 0xff, sizeof(int) * nbin, stream)) != hipSuccess) return err;  // root: -1
    const BinTree B = T.view();
    hipLaunchKernelGGL(k_parents, dim3(grid_for(nbin, 256)), dim3(256), 0, stream, B.child, nbin, C.parent.get(),
                       C.leafparent.get());
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(k_sah_dp, dim3(grid_for(n, 256)), dim3(256), 0, stream, B, n, C.parent.get(), C.leafparent.get(),
                       C.visits.get(), C.cost.get(), C.dec.get());
    return hipGetLastError();
}

// The back end: the SAH dynamic programme over the binary tree, then the BVH4 nodes one level at
// a time (count -> scan -> emit, one host sync per level), numbered breadth-first.  Fills
// out.nodes and, on success only, out.n_nodes, out.depth and out.level_base.
hipError_t collapse_bvh4(BinaryTree& T, int n, CollapseScratch& C, BuildOutput& out, hipStream_t stream) {
    hipError_t err;
    if ((err = sah_dp(T, n, C, stream)) != hipSuccess) return err;
    const int* dec = C.dec;
    const BinTree B = T.view();
    int *work = C.work, *work2 = C.work2;
    int nwork = 1, depth = 0, node_count = 1, level_base = 0;
    std::vector<int> bases;
    // level 0: the binary root (or the single leaf ~0) -> BVH4 slot 0
    if ((err = hipMemcpyAsync(work, &T.root, sizeof(int), hipMemcpyHostToDevice, stream)) != hipSuccess) return err;
    while (nwork > 0) {
        bases.push_back(level_base);
        hipLaunchKernelGGL(k_collapse_count, dim3(grid_for(nwork, 128)), dim3(128), 0, stream, B, dec, work,
                           nwork, C.wcnt.get());
        if ((err = hipGetLastError()) != hipSuccess) return err;
        if ((err = hipcub::DeviceScan::ExclusiveSum(C.temp.get(), C.temp_bytes, C.wcnt.get(), C.woff.get(), nwork,
                                                    stream)) != hipSuccess)
            return err;
        hipLaunchKernelGGL(k_collapse_emit, dim3(grid_for(nwork, 128)), dim3(128), 0, stream, B, dec, work, nwork,
                           C.woff.get(), level_base, node_count, out.nodes, work2);
        if ((err = hipGetLastError()) != hipSuccess) return err;
        int tail[2] = {0, 0};  // offset and count of the level's last item: the next level's size
        if ((err = first_error(
                 {hipMemcpyAsync(&tail[0], C.woff + nwork - 1, sizeof(int), hipMemcpyDeviceToHost, stream),
                  hipMemcpyAsync(&tail[1], C.wcnt + nwork - 1, sizeof(int), hipMemcpyDeviceToHost, stream),
                  hipStreamSynchronize(stream)})) != hipSuccess)
            return err;
        nwork = tail[0] + tail[1];
        level_base = node_count;
        node_count += nwork;
        ++depth;
        std::swap(work, work2);
    }
    bases.push_back(node_count);
    out.n_nodes = node_count;
    out.depth = depth;
    out.level_base.swap(bases);
    return hipSuccess;
}

}  // namespace

hipError_t bvh_build(const BuildInput& in, BuildOutput& out, hipStream_t stream, float* ms) {
    const int n = in.n;
    if (ms) *ms = 0.0f;
    out.n_nodes = 0;
    out.depth = 0;
    out.level_base.clear();
    if (n <= 0) return hipSuccess;
    Event e0, e1;
    MortonOrder morton;    // the front ends' scratch, each one's own
    PlocScratch ploc;
    DevBuf<uint32_t> dfs;  // the SAH builders' triangle order
    CollapseScratch scratch;
    BinaryTree tree;
    StreamIdle idle(stream);  // declared last: the stream is idle before anything above is freed
    hipError_t err = first_error({e0.ensure(), e1.ensure(), scratch.alloc(n, stream)});
    if (err != hipSuccess) return err;
    // a single triangle has no SAH split: the SAH builders take the PLOC path for it
    switch ((n > 1 || in.builder == kBuilderLBVH) ? in.builder : kBuilderPLOC) {
        case kBuilderLBVH: err = build_lbvh(in, out, stream, e0, morton, tree); break;
        case kBuilderSAH: err = build_sah_host(in, out, stream, e0, dfs, tree); break;
        case kBuilderSAHGPU: err = build_sah_gpu(in, out, stream, e0, dfs, tree); break;
        default: err = build_ploc(in, out, stream, e0, morton, ploc, tree); break;
    }
    if (err == hipSuccess) err = collapse_bvh4(tree, n, scratch, out, stream);
    if (err == hipSuccess) err = hipEventRecord(e1, stream);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    if (err == hipSuccess && ms) err = hipEventElapsedTime(ms, e0, e1);
    if (err != hipSuccess) {
        out.n_nodes = 0;
        out.depth = 0;
        out.level_base.clear();
    }
    return err;
}

}  // namespace pt
