// Host check of the lit table's cell index and plane predicates (optixpathtracer_amd/csrc/pt_lit.h,
// compiled as plain C++).  Prints one JSON line; "bad" counts violations.
//   * every level k: the cells 0 .. N^2 - 1 are distinct triangles of the N x N barycentric grid,
//     and a cell's centroid maps back to it;
//   * (u, v) on and around every grid vertex and edge midpoint lands in a cell that contains the
//     point up to kTol grid units, i.e. in the exact cell or one that shares the border with it;
//   * the predicates on a floor cell: an occluder inside the pyramid is kept, occluders aside of
//     it, below the floor plane or behind a wall plane are rejected.
#include <cmath>
#include <cstdio>
#include <set>
#include <tuple>

#include "pt_lit.h"

using namespace pt;

namespace {

constexpr double kTol = 1e-4;  // grid units: fp32 rounding of u + v at N = 256 is ~3e-5

// distance-like violation of point (su, sv) (grid units) against cell c: <= 0 inside
double outside(int k, uint32_t c, double su, double sv) {
    int cu[3], cv[3];
    lit_cell_corners(k, c, cu, cv);
    const double x0 = cu[0], y0 = cv[0], x1 = cu[1], y1 = cv[1], x2 = cu[2], y2 = cv[2];
    const double det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
    const double a = ((su - x0) * (y2 - y0) - (x2 - x0) * (sv - y0)) / det;
    const double b = ((x1 - x0) * (sv - y0) - (su - x0) * (y1 - y0)) / det;
    return std::fmax(std::fmax(-a, -b), a + b - 1.0);
}

}  // namespace

int main() {
    long bad = 0, checked = 0;
    for (int k = 0; k <= kLitMaxLevel; ++k) {
        const int N = 1 << k;
        std::set<std::tuple<int, int, int, int, int, int>> seen;
        if (lit_cells(k) != (uint32_t)(N * N)) ++bad;
        for (uint32_t c = 0; c < lit_cells(k); ++c) {
            int cu[3], cv[3];
            lit_cell_corners(k, c, cu, cv);
            for (int q = 0; q < 3; ++q)
                if (cu[q] < 0 || cv[q] < 0 || cu[q] + cv[q] > N) ++bad;
            const int area2 = (cu[1] - cu[0]) * (cv[2] - cv[0]) - (cu[2] - cu[0]) * (cv[1] - cv[0]);
            if (area2 != 1) ++bad;  // a unit cell, counter-clockwise
            seen.insert({cu[0], cv[0], cu[1], cv[1], cu[2], cv[2]});
            const float u = (float)((cu[0] + cu[1] + cu[2]) / 3.0 / N), v = (float)((cv[0] + cv[1] + cv[2]) / 3.0 / N);
            if (lit_cell_index(k, u, v) != c) ++bad;
            ++checked;
        }
        if (seen.size() != (size_t)(N * N)) ++bad;
        // grid vertices and edge midpoints (in half grid units), nudged by ulps and by 1e-7
        const int step = N > 64 ? 7 : 1;  // the large levels: every 7th line (and the last ones)
        for (int a = 0; a <= 2 * N; a += (a + step > 2 * N && a < 2 * N) ? 1 : step)
            for (int b = 0; a + b <= 2 * N; b += (a + b + step > 2 * N && a + b < 2 * N) ? 1 : step) {
                const float u0 = (float)(a * 0.5 / N), v0 = (float)(b * 0.5 / N);
                for (int du = -2; du <= 2; ++du)
                    for (int dv = -2; dv <= 2; ++dv) {
                        float u = u0, v = v0;
                        for (int s = 0; s < std::abs(du); ++s) u = std::nextafterf(u, du > 0 ? 2.0f : -1.0f);
                        for (int s = 0; s < std::abs(dv); ++s) v = std::nextafterf(v, dv > 0 ? 2.0f : -1.0f);
                        if (std::abs(du) == 2) u = u0 + (du > 0 ? 1e-7f : -1e-7f);
                        if (std::abs(dv) == 2) v = v0 + (dv > 0 ? 1e-7f : -1e-7f);
                        // the tracer's barycentrics: u, v >= 0 and u + v <= 1 in fp32
                        if (u < 0.0f || v < 0.0f || u > 1.0f || u + v > 1.0f) continue;
                        const uint32_t c = lit_cell_index(k, u, v);
                        ++checked;
                        if (c >= lit_cells(k) || outside(k, c, (double)u * N, (double)v * N) > kTol) ++bad;
                    }
            }
    }
    // words
    if (lit_level(lit_word(7, 123456u)) != 7 || lit_first(lit_word(7, 123456u)) != 123456u) ++bad;
    if (lit_cells(kLitNoCells) != 0u || lit_level(lit_word(kLitNoCells, 5u)) != kLitNoCells) ++bad;
    if (lit_level_for(1.0f, 0.3f) != 2 || lit_level_for(0.1f, 0.3f) != 0 || lit_level_for(1e9f, 0.3f) != kLitMaxLevel) ++bad;

    // predicates: a floor triangle (y = 0) of 4 x 4 units at level 2, the light 2 above its middle
    const float v0[3] = {0, 0, 0}, e1[3] = {0, 0, 4}, e2[3] = {4, 0, 0}, light[3] = {1, 2, 1};
    const float m = lit_margin(8.0f);
    LitPyramid P;
    const uint32_t cell = lit_cell_index(2, 0.3f, 0.3f);
    if (!lit_pyramid(v0, e1, e2, 2, cell, light, kLitDelta, m, P)) ++bad;
    {
        const double a[3] = {0.9, 1, 0.9}, b[3] = {1.5, 1, 0.9}, c[3] = {0.9, 1, 1.5};  // between cell and light
        if (lit_tri_outside(P, a, b, c)) ++bad;
        const double lo[3] = {0.9, 0.9, 0.9}, hi[3] = {1.5, 1.1, 1.5};
        if (lit_box_outside(P, lo, hi)) ++bad;
    }
    {
        const double a[3] = {3, 1, 3}, b[3] = {3.5, 1, 3}, c[3] = {3, 1, 3.5};  // aside
        if (!lit_tri_outside(P, a, b, c)) ++bad;
        const double lo[3] = {3, 0.9, 3}, hi[3] = {3.5, 1.1, 3.5};
        if (!lit_box_outside(P, lo, hi)) ++bad;
    }
    {
        const double a[3] = {0, 0, 0}, b[3] = {0, 0, 4}, c[3] = {4, 0, 0};  // the floor itself
        if (!lit_tri_outside(P, a, b, c)) ++bad;
        const double d[3] = {1, -1, 1}, e[3] = {2, 0.0004, 1}, f[3] = {1, -1, 2};  // up to delta above it
        if (!lit_tri_outside(P, d, e, f)) ++bad;
        const double g[3] = {1, -1, 1}, h[3] = {1.2, 0.5, 1.2}, i[3] = {1, -1, 2};  // pierces the floor inside the cell
        if (lit_tri_outside(P, g, h, i)) ++bad;
    }
    {
        const double a[3] = {-0.5, -1, -10}, b[3] = {-0.5, 9, -10}, c[3] = {-0.5, -1, 10};  // a large wall behind
        if (!lit_tri_outside(P, a, b, c)) ++bad;
    }
    {  // light below delta, and a degenerate triangle: no pyramid
        const float low[3] = {1, 0.0004f, 1}, z[3] = {0, 0, 0};
        if (lit_pyramid(v0, e1, e2, 2, cell, low, kLitDelta, m, P)) ++bad;
        if (lit_pyramid(v0, e1, z, 0, 0, light, kLitDelta, m, P)) ++bad;
        const float under[3] = {1, -2, 1};  // the other side of the plane: a pyramid on that side
        if (!lit_pyramid(v0, e1, e2, 2, cell, under, kLitDelta, m, P) || P.base.n[1] > 0.0) ++bad;
    }
    std::printf("{\"bad\": %ld, \"checked\": %ld}\n", bad, checked);
    return bad ? 1 : 0;
}
