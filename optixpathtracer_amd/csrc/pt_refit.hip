// pt_refit.hip — geometry updates on a live renderer (pt_commit_geometry): re-bake the moved
// meshes' triangle records on the device, recompute every BVH4 node box bottom-up for the tree's
// present topology, and reduce the tree's SAH cost.
//
//   1. k_rebake      : one thread per leaf-ordered triangle; a triangle of a dirty mesh takes its
//                      three object-space vertices (and, for a kNormalBaked mesh, normals) through
//                      mat4_mul_vec4 (the host bake's function, so the same bits) and rewrites its
//                      isect / shade records in k_gather's layout.  The w tags and the texcoords stay.
//   2. k_refit_level : one launch per BVH4 level, deepest first (the nodes are numbered
//                      breadth-first, so a level is a contiguous range).  A leaf child's box is the
//                      union of tri_box_padded over its triangles, an inner child's the union of
//                      that node's four child boxes.  fminf / fmaxf unions are exact and
//                      order-independent, and a padded bound is never -0, so the boxes are the ones
//                      a build would store for this topology, bit for bit.
//   3. k_sah_partial : per-block fp64 partial sums of the SAH cost, summed on the host in block
//                      order.
// As in pt_build.hip, every launch reads only what earlier launches wrote: no hand-off between
// workgroups and no waiting.  A single-launch refit with per-node arrival counters (k_sah_dp's
// pattern) was not built: at 250k triangles the level launches are a small part of a commit
// (DESIGN.md §9 has the measurement).
#include "pt_internal.h"

namespace pt {

namespace {

constexpr int kRefitBlock = 256;

__global__ void k_rebake(const RefitMesh* meshes, const float4* overts, const float4* onorms, const int4* tidx, int n,
                         float4* isect, float4* shade) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float4 A = isect[3 * k], E1 = isect[3 * k + 1], E2 = isect[3 * k + 2];
    const int orig = __float_as_int(A.w), mesh = __float_as_int(E1.w);
    const RefitMesh& M = meshes[mesh];
    if (!M.dirty) return;
    const int4 id = tidx[orig];
    const int vi[3] = {id.x, id.y, id.z};
    float wv[3][4], wn[3][4];
    for (int c = 0; c < 3; ++c) {
        const float4 v = overts[vi[c]];
        const float in4[4] = {v.x, v.y, v.z, 1.0f};
        mat4_mul_vec4(M.m, in4, wv[c]);
        wn[c][0] = wn[c][1] = wn[c][2] = 0.0f;  // a mesh without normals bakes zeros
        if (M.normal_mode != 0) {
            const float4 nn = onorms[vi[c]];
            const float n4[4] = {nn.x, nn.y, nn.z, 0.0f};
            if (M.normal_mode == 1) {  // kNormalBaked: world space here
                mat4_mul_vec4(M.m, n4, wn[c]);
            } else {  // kNormalObject: reconstruct applies the matrix
                wn[c][0] = nn.x;
                wn[c][1] = nn.y;
                wn[c][2] = nn.z;
            }
        }
    }
    const float mat_w = shade[4 * k + 3].w;
    isect[3 * k] = make_float4(wv[0][0], wv[0][1], wv[0][2], A.w);
    isect[3 * k + 1] = make_float4(wv[1][0] - wv[0][0], wv[1][1] - wv[0][1], wv[1][2] - wv[0][2], E1.w);
    isect[3 * k + 2] = make_float4(wv[2][0] - wv[0][0], wv[2][1] - wv[0][1], wv[2][2] - wv[0][2], E2.w);
    shade[4 * k] = make_float4(wv[1][0], wv[1][1], wv[1][2], wn[0][0]);
    shade[4 * k + 1] = make_float4(wv[2][0], wv[2][1], wv[2][2], wn[0][1]);
    shade[4 * k + 2] = make_float4(wn[0][2], wn[1][0], wn[1][1], wn[1][2]);
    shade[4 * k + 3] = make_float4(wn[2][0], wn[2][1], wn[2][2], mat_w);
}

__device__ __forceinline__ float min4(float4 v) { return fminf(fminf(v.x, v.y), fminf(v.z, v.w)); }
__device__ __forceinline__ float max4(float4 v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }
__device__ __forceinline__ void set_lane(float4& v, int k, float x) {
    if (k == 0) v.x = x;
    else if (k == 1) v.y = x;
    else if (k == 2) v.z = x;
    else v.w = x;
}

// Nodes base .. base + count - 1 (one level).  Empty slots keep their inverted box; `child` is
// never written.
__global__ void k_refit_level(BNode4* nodes, const float4* isect, int base, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    BNode4* nd = nodes + base + i;
    const int4 ch = nd->child;
    const int cc[4] = {ch.x, ch.y, ch.z, ch.w};
    float4 lox = nd->lox, hix = nd->hix, loy = nd->loy, hiy = nd->hiy, loz = nd->loz, hiz = nd->hiz;
    for (int k = 0; k < 4; ++k) {
        const int c = cc[k];
        if (c == kEmptyChild) continue;
        const float inf = __int_as_float(0x7f800000);
        float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
        if (c < 0) {
            const int first = leaf_first(c), cnt = leaf_count(c);
            for (int t = 0; t < cnt; ++t) {
                const float4 A = isect[3 * (first + t)], E1 = isect[3 * (first + t) + 1],
                             E2 = isect[3 * (first + t) + 2];
                float tl[3], th[3];
                tri_box_padded(mk(A.x, A.y, A.z), mk(E1.x, E1.y, E1.z), mk(E2.x, E2.y, E2.z), tl, th);
                for (int a = 0; a < 3; ++a) {
                    lo[a] = fminf(lo[a], tl[a]);
                    hi[a] = fmaxf(hi[a], th[a]);
                }
            }
        } else {  // a node of a deeper level: an earlier launch refitted it
            const BNode4* cn = nodes + c;
            lo[0] = min4(cn->lox);
            hi[0] = max4(cn->hix);
            lo[1] = min4(cn->loy);
            hi[1] = max4(cn->hiy);
            lo[2] = min4(cn->loz);
            hi[2] = max4(cn->hiz);
        }
        set_lane(lox, k, lo[0]);
        set_lane(hix, k, hi[0]);
        set_lane(loy, k, lo[1]);
        set_lane(hiy, k, hi[1]);
        set_lane(loz, k, lo[2]);
        set_lane(hiz, k, hi[2]);
    }
    nd->lox = lox;
    nd->hix = hix;
    nd->loy = loy;
    nd->hiy = hiy;
    nd->loz = loz;
    nd->hiz = hiz;
}

__device__ __forceinline__ double half_area64(float lx, float ly, float lz, float hx, float hy, float hz) {
    const double x = (double)hx - (double)lx, y = (double)hy - (double)ly, z = (double)hz - (double)lz;
    return x * y + y * z + z * x;
}
__device__ __forceinline__ float lane(float4 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// partial[b] = sum over block b's nodes of their children's cost: half area x kSahCNode for an
// inner child, x kSahCTri x triangles for a leaf.  Node 0 adds the root itself (the union of its
// child boxes) and writes the root's half area to partial[gridDim.x].  The block's tree reduction
// has a fixed order, so the same node array always gives the same partials.
__global__ void k_sah_partial(const BNode4* nodes, int n_nodes, double* partial) {
    __shared__ double red[kRefitBlock];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double s = 0.0;
    if (i < n_nodes) {
        const BNode4 nd = nodes[i];
        const int cc[4] = {nd.child.x, nd.child.y, nd.child.z, nd.child.w};
        const float inf = __int_as_float(0x7f800000);
        float rl[3] = {inf, inf, inf}, rh[3] = {-inf, -inf, -inf};
        for (int k = 0; k < 4; ++k) {
            if (cc[k] == kEmptyChild) continue;
            const float lx = lane(nd.lox, k), ly = lane(nd.loy, k), lz = lane(nd.loz, k);
            const float hx = lane(nd.hix, k), hy = lane(nd.hiy, k), hz = lane(nd.hiz, k);
            const double w = cc[k] < 0 ? (double)kSahCTri * (double)leaf_count(cc[k]) : (double)kSahCNode;
            s += half_area64(lx, ly, lz, hx, hy, hz) * w;
            rl[0] = fminf(rl[0], lx); rl[1] = fminf(rl[1], ly); rl[2] = fminf(rl[2], lz);
            rh[0] = fmaxf(rh[0], hx); rh[1] = fmaxf(rh[1], hy); rh[2] = fmaxf(rh[2], hz);
        }
        if (i == 0) {
            const double root = half_area64(rl[0], rl[1], rl[2], rh[0], rh[1], rh[2]);
            s += root * (double)kSahCNode;
            partial[gridDim.x] = root;
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = kRefitBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

}  // namespace

hipError_t refit_rebake(const RefitMesh* meshes, const float4* overts, const float4* onorms, const int4* tidx, int n,
                        float4* isect, float4* shade, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rebake, dim3((n + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, stream, meshes,
                       overts, onorms, tidx, n, isect, shade);
    return hipGetLastError();
}

hipError_t refit_levels(BNode4* nodes, const float4* isect, const std::vector<int>& level_base, hipStream_t stream) {
    for (int l = (int)level_base.size() - 2; l >= 0; --l) {
        const int base = level_base[(size_t)l], count = level_base[(size_t)l + 1] - base;
        if (count <= 0) continue;
        hipLaunchKernelGGL(k_refit_level, dim3((count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, stream,
                           nodes, isect, base, count);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

int sah_partial_blocks(int n_nodes) { return n_nodes > 0 ? (n_nodes + kRefitBlock - 1) / kRefitBlock : 0; }

hipError_t sah_partial_launch(const BNode4* nodes, int n_nodes, double* partial, hipStream_t stream) {
    if (n_nodes <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sah_partial, dim3(sah_partial_blocks(n_nodes)), dim3(kRefitBlock), 0, stream, nodes, n_nodes,
                       partial);
    return hipGetLastError();
}

}  // namespace pt
