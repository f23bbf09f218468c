// pt_lit.h — the camera-independent lit table: cells, their index and the plane predicates.
//
// Every triangle T (leaf order, the index of a hit record) is cut into N x N barycentric
// sub-triangles ("cells"), N = 2^k from T's longest edge against a target cell size; the cut is
// shared by all lights.  The table holds one bit per (light, cell).  A set bit states: every
// shadow ray the shading kernels build from a point p of that cell toward that light -- origin
// p + 1e-3 * Ng on the light's side of T, direction normalize(l - p), tmax = |l - p| -- is
// unoccluded for the tracer.  The shading kernels then add the light's contribution at once and
// emit no shadow ray (pt_wavefront.hip lit_cell, lit_bit).
//
// The sufficient test behind a set bit (lit_pyramid, lit_tri_outside, lit_box_outside; all in
// fp64 on the fp32 scene data, so the predicates' own rounding is far below every constant here):
//   * the light lies more than kLitDelta above T's plane;
//   * every other triangle U is rejected by one separating plane of the pyramid P = hull(l, cell)
//     grown by the margin m: U lies wholly at or below T's plane + kLitDelta, or wholly more
//     than m outside one of P's three side planes, or P's four vertices lie more than m to one
//     side of U's own plane, or the boxes of U and of P grown by m are disjoint.
// Candidates come from a walk of the BVH4 with the same rejections on the node boxes.  A triangle
// that is not rejected clears the bit, as does a degenerate cell or a full walk stack.
//
// kLitDelta = 5e-4 < 1e-3: the origin offset puts every point of such a shadow ray at least
// 1e-3 above T's plane (the ray climbs from 1e-3 to the light's height + 1e-3), so a triangle
// wholly below T's plane + 5e-4 -- T itself, coplanar neighbours, everything behind T -- cannot
// be hit; the 5e-4 between the two is ~500 ulps of a coordinate below kLitMaxCoord.  The shading
// kernels use the table only when dot(l - p, Ng) > kLitDelta in fp32, i.e. when the offset side
// is the light's side; rounding there is a few ulps of the largest coordinate involved, vertex or
// light, at most ~5e-5 = kLitDelta / 10 below kLitMaxCoord = 128 (ulp 1.5e-5), so it cannot name the
// wrong side.  The bound holds for both: lit_subdivide turns the table off for a scene with a vertex
// beyond it, and the build sets no bit for a light beyond it (a distant "sun" point light is traced).
//
// The margin of one (light, cell) is m = 2e-3 + 1.01 * 2^-12 * (min(reach, diag) + 2e-3)
// (lit_margin_cell; reach = the largest distance from the cell's corners to the light, lit_cell_reach;
// diag = the scene box's diagonal), never more than the scene-wide lit_margin(diag) = 2e-3 +
// diag * 2^-10 that the table used before.  The two terms:
//   * 2e-3: the 1e-3 origin offset -- origin and end point (l + ~1e-3 * Ng, the tmax overshoot) are
//     within 1e-3 of p and l, so the whole ray is within 1e-3 of the segment p-l inside P -- plus
//     1e-3 for everything that is small and fixed: the box pad of tri_accept (~1e-6 + 1e-6 |x|,
//     at most 1.3e-4 below kLitMaxCoord) and the fp32 rounding of p from (u, v), of (u, v) against a
//     cell border (lit_cell_index scales by a power of two, exactly; only fu + fv > 1 rounds) and
//     of the ray itself, together below 2e-4 (kDarkEta below counts them); a border point may land
//     in the neighbouring cell, whose pyramid grown by m still contains it;
//   * the tracer's acceptance (pt_device.h tri_accept_in, kSlabWiden): a hit counts only with its
//     point inside U's padded box stretched by t * 2^-12 along the ray (a t outside that is clamped
//     to the box's own interval, which lies inside it).  t passed t <= tmax =
//     |l - p| <= reach, and the hit lies in the scene box like the origin (within 1e-3), so
//     t <= min(reach, diag) + 2e-3; the factor 1.01 rounds the bound up over the fp32 rounding of
//     t and tmax (a few 1e-7 relative).  The stretch is taken once: lit_margin(diag) took it four
//     times over the whole diagonal.
//
// The dark proof (lit_tri_covers).  The opposite statement for one (light, cell): every such shadow
// ray IS occluded for the tracer, so a shading kernel could skip both the add and the ray.  The table
// on the GPU does NOT hold such bits: the host probe (tools/lit_cover_probe.cpp) found
// that the proof converts too little of the unproven cell area to pay for a second plane.  The
// predicate stays here for that probe and its host check (tests/lit_dark_check.cpp), so the number
// can be re-measured when cells or meshes change.  A cell can never pass both proofs (a covering
// triangle is not rejected).  The sufficient test names ONE triangle U that every ray of the cell hits.
// No union of triangles is ever used: Moller-Trumbore in fp32 is not watertight across a shared
// edge, so a ray aimed at the seam of two triangles may miss both, and a cover by two or more
// triangles proves nothing.  U is never a triangle of an albedo-textured mesh (alpha_cut can remove
// its hits; "cut-outs count as opaque" is only safe for the lit proof; the caller's to exclude), and
// the proof needs the lit proof's preconditions with the light more than the cell's margin above
// T's plane (lit_dark_possible) and within kLitMaxCoord.
//   The rays: for p in the cell the ideal ray is the segment from p' = p + 1e-3 n to l' = l + 1e-3 n
// (n = T's unit normal on the light's side): the pyramid P' = P translated by 1e-3 n.  The ray the
// kernels build (fp32 p, Ng, l - p, normalize, tmax) stays within kDarkEta = 2e-4 of that segment:
// p from (u, v) and p + 1e-3 Ng round by a few ulps of a coordinate (<= 4e-5 below kLitMaxCoord,
// ulp 1.5e-5; this also covers a border point that belongs to the neighbouring cell), l - p by
// another 2.6e-5, and the normalisation by ~2e-7 * tmax <= 8e-5 for tmax <= 443, in sum < 1.8e-4.
//   With s(x) the signed distance to U's plane, U covers the cell if
//   (a) U is no sliver: aspect = hmin / Lmax >= kDarkMinAspect (hmin its smallest height, Lmax its
//       longest edge; the sine of every corner angle is >= aspect);
//   (b) its plane separates l' from the three corners of P' with g = min |s| over the four points;
//   (c) cb = min_i (|s(l')| + |s(c_i')|) / max_i |l' - c_i'| >= kDarkMinCos = 1/8: a ray direction is
//       a convex combination of the three edge directions, so cb bounds |cos| between every ray of
//       the bundle and U's normal from below; it keeps det = A cos and t well conditioned;
//   (d) the three edge rays c_i' -> l' meet U's plane at barycentrics u >= eps, v >= eps,
//       u + v <= 1 - 2 eps.  The map from p' to the hit point is a perspective map, so by convexity
//       every ideal ray of the bundle hits inside the same region;
//   (e) g - eta >= 2^-12 * Tmax and 2^-20 * (R / (g - eta) + 1 / cb) / aspect <= 2^-13, with
//       Tmax = max_i |l' - c_i'| and R = the largest distance from a corner of P' to a vertex of U.
// Why these suffice for fp32 tri_test + tri_accept_in (pt_device.h), with e = 2^-24.  They show that
// t passes unclamped and inside (0, tmax); tri_accept_in leaves such a t as it is:
//   * u, v: tri_test forms u = (tv . (d x e2)) / det, det = e1 . (d x e2) = +-A cos.  Six roundings
//     reach the numerator (tv, the cross product, the dot product), each <= e |tv| |e2|, and the
//     same count reaches det relative to |e1| |e2|; with |e2| / A <= 1 / hmin and |u| <= 1 the error
//     of u (and of v alike) is below 6 e (R + Lmax) / (hmin cos) < 2^-20 (R + Lmax) / (hmin cb):
//     2^-20 = 16 e leaves a factor 2.6.  The real ray is within eta of the ideal one, which moves
//     its hit point in U's plane by at most eta + eta / cos <= 2 eta / cb, i.e. 2 eta / (hmin cb) in
//     barycentric units.  eps = (2 eta + 2^-20 (R + Lmax)) / (hmin cb) is their sum; the second
//     eps at u + v <= 1 covers the rounding of the fp32 sum and the two errors adding.
//   * t: t = (e2 . (tv x e1)) / det, the numerator is +-A times the origin's distance to U's plane,
//     which is >= g - eta, against rounding of 6 e |tv| |e1| |e2|: relative error <= 6 e R /
//     ((g - eta) aspect), plus det's 6 e / (aspect cb); (e) keeps the sum below 2^-13.  The true hit
//     parameter lies in [g - eta, tmax - (g - eta)] because both ends of the real ray are that far
//     from U's plane on opposite sides; t (1 +- 2^-13) stays inside (0, tmax) by (e)'s first part.
//   * tri_accept: the true hit point lies in U, inside U's unpadded box.  Each slab distance is
//     fma(plane, inv, -io) with three roundings (inv, io = o inv, the fma); |o| <= |plane| +
//     |plane - o| turns them into 3 e |a| + e |plane| |inv| for a slab distance a; the second term
//     is below a fifteenth of the pad (1e-6 + 9.5e-7 |plane|) |inv|.  So tn <= t* (1 + 2e-7) and
//     tf >= t* (1 - 2e-7) for the true parameter t*, and with t within 2^-13 of t* the three
//     inequalities tn <= t K, t <= tf K, tn <= tf K (K = 1 + 2^-12) hold.  A zero direction
//     component (inv = +-1e30) leaves that axis' slab at -+huge by the same bound.
//   The boxes of the BVH contain U's padded box, so the walk reaches U unless another hit ends the
// any-hit ray first -- occluded either way.  T itself and its coplanar neighbours never pass (b):
// all of P' lies above T's plane.
// Scenes with a vertex coordinate beyond kLitMaxCoord (1e-3 is then no longer >> an ulp), more than
// kLitMaxLights lights or more than kLitMaxCells cells run without the table; a light beyond
// kLitMaxCoord has no bits.
//
// This header also compiles for the host alone (tests/lit_host_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PT_LIT_HD __host__ __device__ inline
#else
#define PT_LIT_HD inline
#endif

namespace pt {

constexpr int kLitMaxLights = 16;
constexpr uint32_t kLitMaxCells = 1u << 23;  // per light
constexpr int kLitMaxLevel = 8;              // N <= 256
constexpr int kLitNoCells = 0xff;            // level tag of a degenerate triangle: no cells, never lit
constexpr float kLitDelta = 5e-4f;
constexpr float kLitMaxCoord = 128.0f;
constexpr float kLitCellFraction = 0.005f;  // target cell size / scene diagonal
PT_LIT_HD float lit_margin(float diag) { return 2e-3f + diag * 0.0009765625f; }
// The margin of one (light, cell); reach: lit_cell_reach.  Never above lit_margin(diag).
PT_LIT_HD float lit_margin_cell(float diag, double reach) {
    const double t = fmin(reach, (double)diag) + 2e-3;
    const double m = 2e-3 + 1.01 * 0.000244140625 * t;
    return fminf((float)m * 1.0000002f, lit_margin(diag));  // the conversion to fp32 rounds up
}
constexpr double kLitOffset = 1e-3;          // the shadow ray's origin offset along Ng
constexpr double kDarkEta = 2e-4;            // real ray against the ideal segment p' - l'
constexpr double kDarkMinCos = 0.125;        // bundle against U's normal
constexpr double kDarkMinAspect = 0.0625;    // U's smallest height / longest edge
constexpr double kDarkFp = 9.5367431640625e-7;  // 2^-20 = 16 fp32 roundings

// Per-triangle word: level k (or kLitNoCells) << 24 | first cell.
PT_LIT_HD uint32_t lit_word(int k, uint32_t first) { return ((uint32_t)k << 24) | first; }
PT_LIT_HD int lit_level(uint32_t w) { return (int)(w >> 24); }
PT_LIT_HD uint32_t lit_first(uint32_t w) { return w & 0xffffffu; }
PT_LIT_HD uint32_t lit_cells(int k) { return k == kLitNoCells ? 0u : 1u << (2 * k); }

// Level of a triangle with longest edge `edge` for cells of about `target`.
PT_LIT_HD int lit_level_for(float edge, float target) {
    int k = 0;
    while (k < kLitMaxLevel && edge > target * (float)(1 << k)) ++k;
    return k;
}

// Cell of the barycentric point (u, v) (u weights v1, v weights v2) at level k, in [0, N^2).
// Row j = floor(v N) holds 2 (N - j) - 1 cells from offset j (2 N - j): lower (i, j) at 2 i,
// upper at 2 i + 1.  u N and v N are exact (power of two), as are their fractions.
PT_LIT_HD uint32_t lit_cell_index(int k, float u, float v) {
    const int N = 1 << k;
    const float top = (float)(N - 1);
    const float su = u * (float)N, sv = v * (float)N;
    const int j = (int)fminf(fmaxf(sv, 0.0f), top);  // fmaxf drops a NaN
    int i = (int)fminf(fmaxf(su, 0.0f), top);
    const int imax = N - 1 - j;
    int up = 0;
    if (i >= imax)
        i = imax;  // the last cell of a row has no upper neighbour
    else
        up = (su - (float)i) + (sv - (float)j) > 1.0f ? 1 : 0;
    return (uint32_t)(j * (2 * N - j) + 2 * i + up);
}

// The three corners of cell c at level k in grid units (u N, v N).
PT_LIT_HD void lit_cell_corners(int k, uint32_t c, int cu[3], int cv[3]) {
    const int N = 1 << k;
    const int r = N * N - (int)c;  // (N - j)^2 >= r > (N - j - 1)^2
    int s = (int)sqrt((double)r);
    while (s * s < r) ++s;
    while ((s - 1) * (s - 1) >= r) --s;
    const int j = N - s;
    const int rem = (int)c - j * (2 * N - j);
    const int i = rem >> 1;
    if (rem & 1) {
        cu[0] = i + 1; cv[0] = j;
        cu[1] = i + 1; cv[1] = j + 1;
        cu[2] = i;     cv[2] = j + 1;
    } else {
        cu[0] = i;     cv[0] = j;
        cu[1] = i + 1; cv[1] = j;
        cu[2] = i;     cv[2] = j + 1;
    }
}

struct LitPlane {  // n . x - d with |n| = 1
    double n[3], d;
};
PT_LIT_HD double lit_dist(const LitPlane& p, const double x[3]) {
    return p.n[0] * x[0] + p.n[1] * x[1] + p.n[2] * x[2] - p.d;
}
// Largest / smallest signed distance over a box.
PT_LIT_HD double lit_box_max(const LitPlane& p, const double lo[3], const double hi[3]) {
    double s = -p.d;
    for (int a = 0; a < 3; ++a) s += p.n[a] * (p.n[a] > 0.0 ? hi[a] : lo[a]);
    return s;
}
PT_LIT_HD double lit_box_min(const LitPlane& p, const double lo[3], const double hi[3]) {
    double s = -p.d;
    for (int a = 0; a < 3; ++a) s += p.n[a] * (p.n[a] > 0.0 ? lo[a] : hi[a]);
    return s;
}
PT_LIT_HD bool lit_plane_through(const double a[3], const double b[3], const double c[3], LitPlane& p) {
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double l2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const double s1 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], s2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
    // a sliver (sine of the corner angle below 1e-6) has no usable normal; !(>) also catches NaN
    if (!(l2 > 1e-12 * s1 * s2) || !(l2 > 0.0)) return false;
    const double inv = 1.0 / sqrt(l2);
    for (int k = 0; k < 3; ++k) p.n[k] = n[k] * inv;
    p.d = p.n[0] * a[0] + p.n[1] * a[1] + p.n[2] * a[2];
    return true;
}

// The pyramid of one (light, cell): base plane with its normal toward the light, three side
// planes with their normals outward, the four vertices and their box.
struct LitPyramid {
    LitPlane base, side[3];
    double vtx[4][3];  // cell corners, apex
    double lo[3], hi[3];
    double delta, margin;
};

// v0, e1, e2: the triangle as the tracer holds it (isect record).  False: no bit for this cell
// (degenerate triangle or cell, or the light not more than delta above the plane).
PT_LIT_HD bool lit_pyramid(const float v0[3], const float e1[3], const float e2[3], int k, uint32_t cell,
                           const float light[3], float delta, float margin, LitPyramid& P) {
    int cu[3], cv[3];
    lit_cell_corners(k, cell, cu, cv);
    const double inv = 1.0 / (double)(1 << k);
    for (int c = 0; c < 3; ++c)
        for (int a = 0; a < 3; ++a)
            P.vtx[c][a] = (double)v0[a] + (double)cu[c] * inv * (double)e1[a] + (double)cv[c] * inv * (double)e2[a];
    for (int a = 0; a < 3; ++a) P.vtx[3][a] = (double)light[a];
    P.delta = (double)delta;
    P.margin = (double)margin;
    if (!lit_plane_through(P.vtx[0], P.vtx[1], P.vtx[2], P.base)) return false;
    double h = lit_dist(P.base, P.vtx[3]);
    if (h < 0.0) {
        for (int a = 0; a < 3; ++a) P.base.n[a] = -P.base.n[a];
        P.base.d = -P.base.d;
        h = -h;
    }
    if (!(h > P.delta)) return false;
    for (int s = 0; s < 3; ++s) {
        const int a = s, b = (s + 1) % 3, c = (s + 2) % 3;
        if (!lit_plane_through(P.vtx[3], P.vtx[a], P.vtx[b], P.side[s])) return false;
        if (lit_dist(P.side[s], P.vtx[c]) > 0.0) {  // the third corner is inside
            for (int q = 0; q < 3; ++q) P.side[s].n[q] = -P.side[s].n[q];
            P.side[s].d = -P.side[s].d;
        }
    }
    for (int a = 0; a < 3; ++a) {
        P.lo[a] = fmin(fmin(P.vtx[0][a], P.vtx[1][a]), fmin(P.vtx[2][a], P.vtx[3][a])) - P.margin;
        P.hi[a] = fmax(fmax(P.vtx[0][a], P.vtx[1][a]), fmax(P.vtx[2][a], P.vtx[3][a])) + P.margin;
    }
    return true;
}

// True: no shadow ray of the cell can hit a triangle inside the box [lo, hi].
PT_LIT_HD bool lit_box_outside(const LitPyramid& P, const double lo[3], const double hi[3]) {
    for (int a = 0; a < 3; ++a)
        if (lo[a] > P.hi[a] || hi[a] < P.lo[a]) return true;
    if (lit_box_max(P.base, lo, hi) <= P.delta) return true;
    for (int s = 0; s < 3; ++s)
        if (lit_box_min(P.side[s], lo, hi) > P.margin) return true;
    return false;
}

// True: no shadow ray of the cell can hit the triangle a, b, c.
PT_LIT_HD bool lit_tri_outside(const LitPyramid& P, const double a[3], const double b[3], const double c[3]) {
    for (int q = 0; q < 3; ++q) {
        const double l = fmin(fmin(a[q], b[q]), c[q]), h = fmax(fmax(a[q], b[q]), c[q]);
        if (l > P.hi[q] || h < P.lo[q]) return true;
    }
    if (lit_dist(P.base, a) <= P.delta && lit_dist(P.base, b) <= P.delta && lit_dist(P.base, c) <= P.delta) return true;
    for (int s = 0; s < 3; ++s)
        if (lit_dist(P.side[s], a) > P.margin && lit_dist(P.side[s], b) > P.margin && lit_dist(P.side[s], c) > P.margin)
            return true;
    LitPlane u;
    if (lit_plane_through(a, b, c, u)) {
        double mn = lit_dist(u, P.vtx[0]), mx = mn;
        for (int q = 1; q < 4; ++q) {
            const double d = lit_dist(u, P.vtx[q]);
            mn = fmin(mn, d);
            mx = fmax(mx, d);
        }
        if (mn > P.margin || mx < -P.margin) return true;
    }
    return false;
}

// Largest distance from the corners of cell `cell` to the light (lit_margin_cell's reach).
PT_LIT_HD double lit_cell_reach(const float v0[3], const float e1[3], const float e2[3], int k, uint32_t cell,
                                const float light[3]) {
    int cu[3], cv[3];
    lit_cell_corners(k, cell, cu, cv);
    const double inv = 1.0 / (double)(1 << k);
    double r2 = 0.0;
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double x = (double)v0[a] + (double)cu[c] * inv * (double)e1[a] + (double)cv[c] * inv * (double)e2[a];
            s += ((double)light[a] - x) * ((double)light[a] - x);
        }
        r2 = fmax(r2, s);
    }
    return sqrt(r2);
}

// The dark proof's precondition on the pyramid itself: the light more than the margin above T.
PT_LIT_HD bool lit_dark_possible(const LitPyramid& P) { return lit_dist(P.base, P.vtx[3]) > P.margin; }

// True: every shadow ray of the cell hits the triangle a, b, c for the tracer (the header's dark
// proof; lit_dark_possible(P) and a light within kLitMaxCoord are the caller's to check).
PT_LIT_HD bool lit_tri_covers(const LitPyramid& P, const double a[3], const double b[3], const double c[3]) {
    LitPlane u;
    if (!lit_plane_through(a, b, c, u)) return false;
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double nv[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double A2 = nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2];
    const double l1 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], l2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
    const double l3 = (c[0] - b[0]) * (c[0] - b[0]) + (c[1] - b[1]) * (c[1] - b[1]) + (c[2] - b[2]) * (c[2] - b[2]);
    const double Lmax = sqrt(fmax(l1, fmax(l2, l3)));
    const double hmin = sqrt(A2) / Lmax, aspect = hmin / Lmax;
    if (!(aspect >= kDarkMinAspect)) return false;  // (a); also NaN
    double q[4][3], s[4];  // the corners of P' and its apex, their signed distances
    for (int i = 0; i < 4; ++i) {
        for (int k = 0; k < 3; ++k) q[i][k] = P.vtx[i][k] + kLitOffset * P.base.n[k];
        s[i] = lit_dist(u, q[i]);
    }
    const double sg = s[3] > 0.0 ? 1.0 : -1.0;
    double g = sg * s[3], Tmax = 0.0, span = INFINITY, R = 0.0;
    for (int i = 0; i < 3; ++i) {
        if (!(sg * s[i] < 0.0)) return false;  // (b)
        g = fmin(g, -sg * s[i]);
        span = fmin(span, sg * (s[3] - s[i]));
        const double d[3] = {q[3][0] - q[i][0], q[3][1] - q[i][1], q[3][2] - q[i][2]};
        Tmax = fmax(Tmax, sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
        const double* w[3] = {a, b, c};
        for (int j = 0; j < 3; ++j) {
            const double x = q[i][0] - w[j][0], y = q[i][1] - w[j][1], z = q[i][2] - w[j][2];
            R = fmax(R, sqrt(x * x + y * y + z * z));
        }
    }
    const double cb = span / Tmax;
    if (!(cb >= kDarkMinCos)) return false;  // (c)
    const double gm = g - kDarkEta;
    if (!(gm > 0.0) || !(gm >= Tmax * 0.000244140625)) return false;  // (e)
    if (!(kDarkFp * (R / gm + 1.0 / cb) / aspect <= 0.0001220703125)) return false;
    const double eps = (2.0 * kDarkEta + kDarkFp * (R + Lmax)) / (hmin * cb);
    if (!(eps < 0.25)) return false;
    for (int i = 0; i < 3; ++i) {  // (d)
        const double t = s[i] / (s[i] - s[3]);
        const double w[3] = {q[i][0] + t * (q[3][0] - q[i][0]) - a[0], q[i][1] + t * (q[3][1] - q[i][1]) - a[1],
                             q[i][2] + t * (q[3][2] - q[i][2]) - a[2]};
        const double we2[3] = {w[1] * e2[2] - w[2] * e2[1], w[2] * e2[0] - w[0] * e2[2], w[0] * e2[1] - w[1] * e2[0]};
        const double e1w[3] = {e1[1] * w[2] - e1[2] * w[1], e1[2] * w[0] - e1[0] * w[2], e1[0] * w[1] - e1[1] * w[0]};
        const double bu = (we2[0] * nv[0] + we2[1] * nv[1] + we2[2] * nv[2]) / A2;
        const double bv = (e1w[0] * nv[0] + e1w[1] * nv[1] + e1w[2] * nv[2]) / A2;
        if (!(bu >= eps && bv >= eps && bu + bv <= 1.0 - 2.0 * eps)) return false;
    }
    return true;
}

// True: the segment from `o` to `e` misses the box [lo, hi] grown by 1e-6 (the probe's walk for a
// cell's central ray).
PT_LIT_HD bool lit_box_misses_segment(const double o[3], const double e[3], const double lo[3], const double hi[3]) {
    double t0 = 0.0, t1 = 1.0;
    for (int a = 0; a < 3; ++a) {
        const double d = e[a] - o[a], l = lo[a] - 1e-6 - o[a], h = hi[a] + 1e-6 - o[a];
        if (d == 0.0) {
            if (l > 0.0 || h < 0.0) return true;
            continue;
        }
        const double x = l / d, y = h / d;
        t0 = fmax(t0, fmin(x, y));
        t1 = fmin(t1, fmax(x, y));
    }
    return t0 > t1;
}

}  // namespace pt
