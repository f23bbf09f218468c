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
// The margin m = 2e-3 + diag * 2^-10 (lit_margin; diag = the scene box's diagonal) covers, with
// room to spare:
//   * the 1e-3 origin offset: origin and end point (l + ~1e-3 * Ng, the tmax overshoot) are
//     within 1e-3 of p and l, so the whole ray is within 1e-3 of the segment p-l inside P;
//   * the tracer's acceptance (pt_device.h tri_accept, kSlabWiden): a hit counts only with its
//     point inside U's padded box stretched by t * 2^-12 <= diag * 2^-12 along the ray, a quarter
//     of the second term; the box pad itself is ~1e-6;
//   * fp32 rounding of p from (u, v) and of (u, v) against a cell border (lit_cell_index scales
//     by a power of two, exactly; only fu + fv > 1 rounds): ~1e-7 * diag, a border point may land
//     in the neighbouring cell, whose pyramid grown by m still contains it.
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

}  // namespace pt
