// pt_skip.h — the skip table: per (triangle, side) one BVH4 subtree that an extension ray leaving that
// side of the triangle cannot hit, so k_trace_pair drops it from the traversal unvisited.
//
// A continuation ray leaves triangle T (leaf order) from o = p + 1e-3 * Ng on one side of T's plane and
// goes up from it.  Its origin lies inside every box on the root-to-leaf path of T, so the ordered
// traversal first descends into T's own neighbourhood and tests T's neighbours before it leaves; on a
// closed, locally convex mesh all of them lie at or below T's plane.  The table holds two 32-bit words per
// triangle, word[2 t + side]; side 0 is the side of the stored winding's normal e1 x e2, side 1 the
// other.  A word is 0 ("none": every other writer of the ray record's fourth word stores 0.0f) or the
// child link -- an inner node's index or a leaf's code, as BNode4::child holds it -- of the highest
// link on T's path whose whole subtree is "below" T on that side (skip_tri_below for every triangle
// under it).  A link is never 0 (the root is nobody's child) and names one subtree only.  The shading
// kernels store the word with a continuation ray only when fp32 dot(d, off) > kSkipMinCos for the
// normalised direction d they write and off = the unit vector along the origin offset; k_trace_pair's
// lanes drop the named link when it turns up in TravState::cur (trav_node_step).
//
// Why the images do not change.  The wavefront's closest hit is the (t, original index) minimum over
// the hits that fp32 tri_test + tri_accept_in take (pt_device.h), whatever the visiting order, so leaving
// out triangles that can produce no such hit leaves every hit record as it was; tri_accept_in's box
// and range tests and the alpha cut-outs of the textured kernels only remove hits.  Its clamp does
// not: it can turn a t outside [0, best] into one inside, which "the clamped t" below deals with.
// With h(x) the height over T's plane on the ray's side (n the unit normal, exact arithmetic):
//   * the ray.  p is the fp32 combination of T's vertices with accepted (u, v), off = +-1e-3 * Ng, and
//     tri_test subtracts v0 from o once more: together below 6e-5 of position error for coordinates up
//     to kLitMaxCoord = 128 (ulp 7.6e-6), counted as a shift of the whole ray.  T's fp32 normal is
//     within 1e-4 rad of n because T is no sliver (aspect = smallest height / longest edge >=
//     kSkipMinAspectT; a T below that has no words).  So h(o) >= 9.4e-4, d . n >= 2^-6 - 1e-4 > 1/65,
//     and h(o + t d) >= 9.4e-4 + t / 65 for every t >= 0, tmax = 100 included: the whole ray is more
//     than 4.4e-4 above kLitDelta = 5e-4, and climbing.  This is the statement pt_lit.h relies on for
//     shadow rays ("T itself, coplanar neighbours, everything behind T cannot be hit"), here with a
//     lower bound on the climb as well.
//   * the exact test.  Moller-Trumbore solves o + t d = (1 - u - v) a + u b + v c for a triangle U;
//     taking heights, h(o) + t (d . n) = (1 - u - v) h(a) + u h(b) + v h(c).  With all three heights
//     <= kLitDelta and s their spread, the right side is at most kLitDelta + s mu, mu = the amount by
//     which (u, v) violates u >= 0, v >= 0, u + v <= 1.  For t >= 0 the left side is at least
//     9.4e-4 + t / 65, so mu >= (4.4e-4 + t / 65) / s: the exact test rejects, by a margin that grows
//     with t.  A coplanar U (s = 0: T itself, the other half of a wall) has no solution at all.
//   * the fp32 test.  det = e1 . (d x e2) = +-Lmax hmin cos (hmin, Lmax: U's smallest height and
//     longest edge, cos: between d and U's normal) carries at most 8 e Lmax^2 of rounding, e = 2^-24,
//     and the numerators of u and v 8 e R Lmax, R = the largest distance from the origin to a vertex
//     of U.  While that is an eighth of det or less, the computed (u, v) differ from the exact ones by
//     at most 1.2 ((1 + mu) 8 e Lmax^2 + 8 e R Lmax) / |det| each, and passing all three tests with
//     them needs mu <= 96 e (Lmax + R) / (hmin |cos|) + 5 e.  Against mu >= 4.4e-4 / s that is
//     impossible for |cos| >= 0.013 s (Lmax + R) / hmin: on the benchmark's spheres (s <= 0.04,
//     Lmax + R <= 0.45, hmin >= 0.007 at the poles) for every ray more than 2 degrees off U's plane.
//   * the clamped t.  The bullets above exclude a pass of (u, v) with t >= 0.  A pass with t < 0 used to
//     end at tri_test's own range test; now the range test follows tri_accept's clamp, and U's
//     axis-aligned box may well cross T's plane, so its slab interval [tn, tf] can reach past 0.  Take a
//     U below T whose fp32 (u, v) pass, under the premise of the last bullet (|cos| above its bound).
//     In exact arithmetic the ray's line then meets U itself (were the exact (u, v) outside by mu, the
//     point would be mu Lmax beside U, and the same argument runs with that many units of slack); the
//     point's height is <= kLitDelta, so by the heights t_exact <= -4.4e-4 / (d . n) <= -4.4e-4.
//     (i) The point lies in U, hence in U's padded box, so tn <= t_exact: tn is negative, and a t
//     clamped up to tn fails 0 <= t.  (ii) The fp32 t differs from t_exact by a relative e (Lmax + R) /
//     (hmin |cos|) times a small count, far below 1 under the premise, so it is negative too: left
//     unclamped it fails 0 <= t, and it can never exceed tf K with tf >= 0, which a t clamped down to an
//     accepted tf would need.  So no t of a U below T, clamped or not, passes the range test.
//   * what is assumed.  For a ray closer to U's plane than that bound the worst-case rounding above no
//     longer excludes a hit, although the ray stays 4.4e-4 -- 58 ulps of the largest coordinate, about
//     2000 of the benchmark's -- away from every point of U.  This is the premise the lit table's
//     kLitDelta rests on, no weaker here.  It needs U's hmin to mean something, so U counts as below
//     only with aspect >= kSkipMinAspect: a sliver (or a triangle without a plane) simply does not
//     count and blocks the skip at its subtree.  tests/test_gpu_skip_table.py holds the table to
//     bit-identical accumulators, and profiles/skip_table_counters.jsonl records the same comparison
//     on the headline batch (1.2 G rays with a skip).
// So U counts as below T (skip_tri_below) when all three of its vertices have h <= kLitDelta and its
// aspect is at least kSkipMinAspect.  The predicates run in fp64 on the fp32 scene data, like the lit
// table's, so their own rounding is far below every constant.  A scene with a vertex beyond
// kLitMaxCoord has no table (skip_tri_in_bounds): 1e-3 is then no longer far above an ulp.
//
// The table depends on the triangle records and the BVH numbering alone; it is rebuilt after every BVH
// build, refit and mesh move.  In a scene without slivers a box wholly below the plane passes as a whole
// (box_accept); with one, every triangle is looked at.  A walk examines at most kSkipMaxTris triangles
// per (triangle, side) and keeps the link proven so far when that runs out, which bounds the build on
// scenes with large flat regions (every triangle of a floor sees the whole scene below its outer side).
//
// This header also compiles for the host alone (tests/skip_host_check.cpp).
#pragma once
#include "pt_lit.h"

namespace pt {

constexpr float kSkipMinCos = 0.015625f;       // 2^-6: the use condition on dot(d, off)
constexpr double kSkipMinAspectT = 0.0009765625;  // 2^-10: T's own aspect, for its fp32 normal
constexpr double kSkipMinAspect = 0.015625;       // 2^-6: below it U is a sliver and blocks the skip
constexpr int kSkipMaxTris = 4096;             // triangles one walk examines before it stops climbing
constexpr uint32_t kSkipNone = 0u;

// A BVH4 node as 32 words: lox[4] hix[4] loy[4] hiy[4] loz[4] hiz[4] child[4] pad[4] (pt_device.h BNode4).
constexpr int kSkipNodeWords = 32;
constexpr int kSkipEmptyChild = (int)0x80000000;
PT_LIT_HD int skip_leaf_first(int c) { return (~c) >> 3; }
PT_LIT_HD int skip_leaf_count(int c) { return ((~c) & 7) + 1; }

// Triangle t of the leaf-ordered isect records (v0 | e1 | e2, 12 floats) as the hit test sees it.
PT_LIT_HD void skip_tri_vertices(const float* isect, int t, double a[3], double b[3], double c[3]) {
    const float* r = isect + 12 * (size_t)t;
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)r[k];
        b[k] = (double)r[k] + (double)r[4 + k];
        c[k] = (double)r[k] + (double)r[8 + k];
    }
}

// Longest edge and aspect (smallest height / longest edge) of a triangle; 0 for a degenerate one.
PT_LIT_HD double skip_aspect(const double a[3], const double b[3], const double c[3], double* lmax) {
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double e3[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
    const double nv[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double l2 = fmax(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2],
                           fmax(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2], e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]));
    *lmax = sqrt(l2);
    if (!(l2 > 0.0)) return 0.0;
    return sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]) / l2;
}

// T on one side: its plane with the normal toward that side.
struct SkipOrigin {
    LitPlane plane;
};
// False: T has no words (degenerate, a sliver, or not finite).
PT_LIT_HD bool skip_origin(const float* isect, int t, int side, SkipOrigin& T) {
    double a[3], b[3], c[3], lmax;
    skip_tri_vertices(isect, t, a, b, c);
    if (!lit_plane_through(a, b, c, T.plane)) return false;
    if (!(skip_aspect(a, b, c, &lmax) >= kSkipMinAspectT)) return false;
    if (side) {
        for (int k = 0; k < 3; ++k) T.plane.n[k] = -T.plane.n[k];
        T.plane.d = -T.plane.d;
    }
    return true;
}

// True: the triangle a, b, c counts as below T's plane on T's side (the header's argument).
PT_LIT_HD bool skip_tri_below(const SkipOrigin& T, const double a[3], const double b[3], const double c[3]) {
    const double ha = lit_dist(T.plane, a), hb = lit_dist(T.plane, b), hc = lit_dist(T.plane, c);
    if (!(ha <= (double)kLitDelta && hb <= (double)kLitDelta && hc <= (double)kLitDelta)) return false;  // also NaN
    double lmax;
    return skip_aspect(a, b, c, &lmax) >= kSkipMinAspect;  // a sliver does not count
}

// Every triangle of the leaf `code` is below T; *budget counts the triangles examined.
PT_LIT_HD bool skip_leaf_below(const SkipOrigin& T, const float* isect, int code, int* budget) {
    const int first = skip_leaf_first(code), cnt = skip_leaf_count(code);
    for (int q = 0; q < cnt; ++q) {
        double a[3], b[3], c[3];
        skip_tri_vertices(isect, first + q, a, b, c);
        --*budget;
        if (!skip_tri_below(T, a, b, c)) return false;
    }
    return true;
}

// Every triangle under the child link `link` is below T.  A box wholly above the plane fails at once (it
// holds a vertex).  box_accept (the scene has no sliver, skip_tri_sliver): a box wholly at or below the
// plane + kLitDelta passes without a look at its triangles -- they all lie in it and none fails the
// aspect; otherwise every box descends to the triangles, whose aspect no box can answer.  stk: the
// walk's stack, entry s at stk[s * stride], `cap` entries; a full stack or a spent budget fails.
PT_LIT_HD bool skip_subtree_below(const SkipOrigin& T, const void* nodes, const float* isect, int link, int* stk,
                                  int stride, int cap, int* budget, bool box_accept) {
    int sp = 0;
    stk[0] = link;
    sp = 1;
    while (sp > 0) {
        const int c = stk[(size_t)(--sp) * stride];
        if (*budget <= 0) return false;
        if (c < 0) {
            if (!skip_leaf_below(T, isect, c, budget)) return false;
            continue;
        }
        const float* f = (const float*)nodes + (size_t)kSkipNodeWords * c;
        const int* ch = (const int*)nodes + (size_t)kSkipNodeWords * c + 24;
        for (int q = 0; q < 4; ++q) {
            if (ch[q] == kSkipEmptyChild) continue;
            const double lo[3] = {f[q], f[8 + q], f[16 + q]}, hi[3] = {f[4 + q], f[12 + q], f[20 + q]};
            if (lit_box_min(T.plane, lo, hi) > (double)kLitDelta) return false;
            if (box_accept && lit_box_max(T.plane, lo, hi) <= (double)kLitDelta) continue;
            if (sp >= cap) return false;
            stk[(size_t)(sp++) * stride] = ch[q];
        }
    }
    return true;
}

// True: triangle t would fail skip_tri_below's aspect wherever it lies (a sliver, degenerate, not finite).
PT_LIT_HD bool skip_tri_sliver(const float* isect, int t) {
    double a[3], b[3], c[3], lmax;
    skip_tri_vertices(isect, t, a, b, c);
    return !(skip_aspect(a, b, c, &lmax) >= kSkipMinAspect);
}

// Parent links: node_parent[i] = parent node << 2 | slot (-1 for the root), tri_parent[t] the same for
// the leaf that holds triangle t.  One call per node (the build kernel: one thread each).  True: one of
// the node's leaf triangles is a sliver (the scene then gets no box_accept).
PT_LIT_HD bool skip_parents_of(const void* nodes, const float* isect, int ni, int* node_parent, int* tri_parent) {
    bool sliver = false;
    const int* ch = (const int*)nodes + (size_t)kSkipNodeWords * ni + 24;
    if (ni == 0) node_parent[0] = -1;
    for (int q = 0; q < 4; ++q) {
        const int c = ch[q];
        if (c == kSkipEmptyChild) continue;
        if (c >= 0) {
            node_parent[c] = (ni << 2) | q;
        } else {
            const int first = skip_leaf_first(c), cnt = skip_leaf_count(c);
            for (int k = 0; k < cnt; ++k) {
                tri_parent[first + k] = (ni << 2) | q;
                sliver = sliver || skip_tri_sliver(isect, first + k);
            }
        }
    }
    return sliver;
}

// The word of (triangle t, side): climbs T's path from its leaf; a link passes when the link below it
// passed and every sibling of that one is below T.
PT_LIT_HD uint32_t skip_word(const void* nodes, const float* isect, const int* node_parent, const int* tri_parent,
                             int t, int side, int* stk, int stride, int cap, bool box_accept) {
    SkipOrigin T;
    if (!skip_origin(isect, t, side, T)) return kSkipNone;
    int budget = kSkipMaxTris;
    int at = tri_parent[t];  // node << 2 | slot of the link being decided
    const int* ch = (const int*)nodes + (size_t)kSkipNodeWords * (at >> 2) + 24;
    if (!skip_leaf_below(T, isect, ch[at & 3], &budget)) return kSkipNone;
    uint32_t best = (uint32_t)ch[at & 3];
    for (int level = 0; level < 64; ++level) {  // a tree is far shallower (pt_create: 3 * depth <= 71)
        const int ni = at >> 2, slot = at & 3;
        if (ni == 0) break;  // a child of the root is the highest link there is
        const float* f = (const float*)nodes + (size_t)kSkipNodeWords * ni;
        ch = (const int*)nodes + (size_t)kSkipNodeWords * ni + 24;
        bool ok = true;
        for (int q = 0; q < 4 && ok; ++q) {
            if (q == slot || ch[q] == kSkipEmptyChild) continue;
            const double lo[3] = {f[q], f[8 + q], f[16 + q]}, hi[3] = {f[4 + q], f[12 + q], f[20 + q]};
            if (lit_box_min(T.plane, lo, hi) > (double)kLitDelta) ok = false;
            else if (box_accept && lit_box_max(T.plane, lo, hi) <= (double)kLitDelta) ok = true;
            else ok = skip_subtree_below(T, nodes, isect, ch[q], stk, stride, cap, &budget, box_accept);
        }
        if (!ok) break;
        at = node_parent[ni];
        best = (uint32_t)ni;  // the link to node ni is that node's index
    }
    return best;
}

// The scene bound of the table: every vertex finite and within kLitMaxCoord.
PT_LIT_HD bool skip_tri_in_bounds(const float* isect, int t) {
    const float* r = isect + 12 * (size_t)t;
    for (int k = 0; k < 3; ++k) {
        if (!(fabsf(r[k]) <= kLitMaxCoord && fabsf(r[k] + r[4 + k]) <= kLitMaxCoord && fabsf(r[k] + r[8 + k]) <= kLitMaxCoord))
            return false;
    }
    return true;
}

}  // namespace pt
