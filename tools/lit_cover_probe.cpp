// lit_cover_probe.cpp — host-only coverage probe of the lit table's proofs (pt_lit.h), no GPU.
//
//   c++ -O2 -std=c++17 -pthread -Ioptixpathtracer_amd/csrc tools/lit_cover_probe.cpp -o lit_cover_probe
//   lit_cover_probe scene.bin [cell fraction ...]        (scene.bin: tools/lit_cover_probe.py export)
//
// For every (light, cell) whose light lies more than kLitDelta above the cell's plane ("facing") it
// evaluates the scene-margin lit proof (lit_margin(diag), the table before the per-cell margin), the
// per-cell-margin lit proof and the dark proof (lit_tri_covers), and classifies the cell's centroid
// shadow ray with an fp64 any-hit over all triangles (a median-split BVH only skips boxes the
// segment misses, the answer is the brute-force one).  Shares are area-weighted.  One JSON object per
// cell fraction on stdout.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "pt_lit.h"

using namespace pt;

struct Tri {
    float v0[3], e1[3], e2[3];
    double a[3], b[3], c[3];
};
struct Node {
    double lo[3], hi[3];
    int left, right, first, count;  // count > 0: leaf
};
static std::vector<Tri> tris;
static std::vector<Node> nodes;

static int build(std::vector<int>& ids, int first, int count) {
    Node n;
    for (int k = 0; k < 3; ++k) n.lo[k] = INFINITY, n.hi[k] = -INFINITY;
    for (int i = first; i < first + count; ++i) {
        const Tri& t = tris[ids[i]];
        for (int k = 0; k < 3; ++k) {
            n.lo[k] = fmin(n.lo[k], fmin(t.a[k], fmin(t.b[k], t.c[k])));
            n.hi[k] = fmax(n.hi[k], fmax(t.a[k], fmax(t.b[k], t.c[k])));
        }
    }
    n.left = n.right = -1;
    n.first = first;
    n.count = count;
    const int me = (int)nodes.size();
    nodes.push_back(n);
    if (count > 4) {
        int ax = 0;
        for (int k = 1; k < 3; ++k)
            if (n.hi[k] - n.lo[k] > n.hi[ax] - n.lo[ax]) ax = k;
        auto key = [&](int id) { return tris[id].a[ax] + tris[id].b[ax] + tris[id].c[ax]; };
        std::nth_element(ids.begin() + first, ids.begin() + first + count / 2, ids.begin() + first + count,
                         [&](int x, int y) { return key(x) < key(y); });
        const int l = build(ids, first, count / 2), r = build(ids, first + count / 2, count - count / 2);
        nodes[me].left = l;
        nodes[me].right = r;
        nodes[me].count = 0;
    }
    return me;
}

// fp64 Moller-Trumbore on the segment o -> e, closed interval
static bool seg_hits(const double o[3], const double e[3], const Tri& t) {
    const double d[3] = {e[0] - o[0], e[1] - o[1], e[2] - o[2]};
    const double e1[3] = {t.b[0] - t.a[0], t.b[1] - t.a[1], t.b[2] - t.a[2]}, e2[3] = {t.c[0] - t.a[0], t.c[1] - t.a[1], t.c[2] - t.a[2]};
    const double p[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const double det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (det == 0.0) return false;
    const double tv[3] = {o[0] - t.a[0], o[1] - t.a[1], o[2] - t.a[2]};
    const double u = (tv[0] * p[0] + tv[1] * p[1] + tv[2] * p[2]) / det;
    if (u < 0.0 || u > 1.0) return false;
    const double q[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    const double v = (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) / det;
    if (v < 0.0 || u + v > 1.0) return false;
    const double s = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) / det;
    return s >= 0.0 && s <= 1.0;
}

struct Sums {
    double facing = 0, lit_old = 0, lit_new = 0, occluded = 0, dark = 0, dark_wrong = 0;
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[2];
    if (fread(hd, 4, 2, f) != 2) return 2;
    const int ntri = hd[0], nl = hd[1];
    std::vector<float> tv((size_t)ntri * 9), lv((size_t)nl * 3);
    if (fread(tv.data(), 4, tv.size(), f) != tv.size() || fread(lv.data(), 4, lv.size(), f) != lv.size()) return 2;
    fclose(f);
    tris.resize(ntri);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = 0; t < ntri; ++t) {
        Tri& T = tris[t];
        const float* v = &tv[(size_t)t * 9];
        for (int k = 0; k < 3; ++k) {
            T.v0[k] = v[k];
            T.e1[k] = v[3 + k] - v[k];  // one fp32 subtraction, as the tracer's records
            T.e2[k] = v[6 + k] - v[k];
            T.a[k] = T.v0[k];
            T.b[k] = (double)T.v0[k] + T.e1[k];
            T.c[k] = (double)T.v0[k] + T.e2[k];
            for (int j = 0; j < 3; ++j) lo[k] = fmin(lo[k], v[3 * j + k]), hi[k] = fmax(hi[k], v[3 * j + k]);
        }
    }
    const float diag = (float)sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    std::vector<int> ids(ntri);
    for (int t = 0; t < ntri; ++t) ids[t] = t;
    nodes.reserve((size_t)ntri);
    build(ids, 0, ntri);
    std::vector<float> fractions;
    for (int i = 2; i < argc; ++i) fractions.push_back((float)atof(argv[i]));
    if (fractions.empty()) fractions.push_back(kLitCellFraction);
    const unsigned nthreads = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    for (float fraction : fractions) {
        const float target = fraction * diag;
        std::vector<int> level(ntri);
        uint64_t cells = 0;
        for (int t = 0; t < ntri; ++t) {
            const Tri& T = tris[t];
            const double o[3] = {0, 0, 0}, a[3] = {T.e1[0], T.e1[1], T.e1[2]}, b[3] = {T.e2[0], T.e2[1], T.e2[2]};
            LitPlane p;
            level[t] = kLitNoCells;
            if (lit_plane_through(o, a, b, p)) {
                const double l1 = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), l2 = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
                const double l3 = sqrt((b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1]) + (b[2] - a[2]) * (b[2] - a[2]));
                level[t] = lit_level_for((float)fmax(l1, fmax(l2, l3)), target);
            }
            cells += lit_cells(level[t]);
        }
        std::vector<Sums> per((size_t)nl * nthreads);
        std::atomic<int> next{0};
        auto work = [&](unsigned tid) {
            std::vector<int> stack;
            for (;;) {
                const int t = next.fetch_add(1);
                if (t >= ntri) break;
                const Tri& T = tris[t];
                const int k = level[t];
                if (k == kLitNoCells) continue;
                const double e1[3] = {T.e1[0], T.e1[1], T.e1[2]}, e2[3] = {T.e2[0], T.e2[1], T.e2[2]};
                const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
                const double area = 0.5 * sqrt(cx * cx + cy * cy + cz * cz) / (double)lit_cells(k);
                for (int li = 0; li < nl; ++li) {
                    Sums& S = per[(size_t)li * nthreads + tid];
                    const float* lp = &lv[(size_t)li * 3];
                    for (uint32_t cell = 0; cell < lit_cells(k); ++cell) {
                        LitPyramid P[2];
                        const float m_old = lit_margin(diag);
                        const float m_new = lit_margin_cell(diag, lit_cell_reach(T.v0, T.e1, T.e2, k, cell, lp));
                        if (!lit_pyramid(T.v0, T.e1, T.e2, k, cell, lp, kLitDelta, m_old, P[0])) continue;
                        if (!lit_pyramid(T.v0, T.e1, T.e2, k, cell, lp, kLitDelta, m_new, P[1])) continue;
                        S.facing += area;
                        bool lit[2] = {true, true}, dark = false;
                        for (int v = 0; v < 2; ++v) {
                            const bool may_dark = v == 1 && lit_dark_possible(P[1]);
                            stack.assign(1, 0);
                            while (!stack.empty() && (lit[v] || (may_dark && !dark))) {
                                const Node& n = nodes[stack.back()];
                                stack.pop_back();
                                if (lit_box_outside(P[v], n.lo, n.hi)) continue;
                                if (n.count == 0) {
                                    stack.push_back(n.left);
                                    stack.push_back(n.right);
                                    continue;
                                }
                                for (int i = n.first; i < n.first + n.count; ++i) {
                                    const Tri& U = tris[ids[i]];
                                    if (lit_tri_outside(P[v], U.a, U.b, U.c)) continue;
                                    lit[v] = false;
                                    if (may_dark && lit_tri_covers(P[1], U.a, U.b, U.c)) dark = true;
                                }
                            }
                        }
                        // the centroid's ideal shadow ray
                        double o[3], e[3];
                        for (int a = 0; a < 3; ++a) {
                            o[a] = (P[1].vtx[0][a] + P[1].vtx[1][a] + P[1].vtx[2][a]) / 3.0 + kLitOffset * P[1].base.n[a];
                            e[a] = P[1].vtx[3][a] + kLitOffset * P[1].base.n[a];
                        }
                        bool occ = false;
                        stack.assign(1, 0);
                        while (!stack.empty() && !occ) {
                            const Node& n = nodes[stack.back()];
                            stack.pop_back();
                            if (lit_box_misses_segment(o, e, n.lo, n.hi)) continue;
                            if (n.count == 0) {
                                stack.push_back(n.left);
                                stack.push_back(n.right);
                                continue;
                            }
                            for (int i = n.first; i < n.first + n.count && !occ; ++i) occ = seg_hits(o, e, tris[ids[i]]);
                        }
                        if (lit[0]) S.lit_old += area;
                        if (lit[1]) S.lit_new += area;
                        if (occ) S.occluded += area;
                        if (dark) S.dark += area;
                        if (dark && !occ) S.dark_wrong += area;  // must stay 0
                    }
                }
            }
        };
        std::vector<std::thread> th;
        for (unsigned i = 0; i < nthreads; ++i) th.emplace_back(work, i);
        for (auto& x : th) x.join();
        printf("{\"cell_fraction\": %g, \"cells_per_light\": %llu, \"table_bytes_per_plane\": %llu, \"margin_scene\": %.6g, \"lights\": [",
               fraction, (unsigned long long)cells, (unsigned long long)((cells + 31) / 32 * 4 * kLitMaxLights), lit_margin(diag));
        Sums tot;
        for (int li = 0; li <= nl; ++li) {
            Sums s;
            if (li < nl) {
                for (unsigned i = 0; i < nthreads; ++i) {
                    const Sums& q = per[(size_t)li * nthreads + i];
                    s.facing += q.facing, s.lit_old += q.lit_old, s.lit_new += q.lit_new, s.occluded += q.occluded;
                    s.dark += q.dark, s.dark_wrong += q.dark_wrong;
                }
                tot.facing += s.facing, tot.lit_old += s.lit_old, tot.lit_new += s.lit_new, tot.occluded += s.occluded;
                tot.dark += s.dark, tot.dark_wrong += s.dark_wrong;
            } else {
                s = tot;
                printf("], \"all\": ");
            }
            const double unproven = s.facing - s.lit_old;
            printf("%s{\"facing_area\": %.6g, \"lit_share_scene_margin\": %.4f, \"lit_share_cell_margin\": %.4f, "
                   "\"occluded_centroid_share\": %.4f, \"dark_share_of_occluded\": %.4f, \"dark_with_clear_centroid_area\": %.3g, "
                   "\"unproven_share_converted\": %.4f, \"converted_by_margin\": %.4f, \"converted_by_dark\": %.4f}",
                   li > 0 && li < nl ? ", " : "", s.facing, s.lit_old / s.facing, s.lit_new / s.facing, s.occluded / s.facing,
                   s.occluded > 0 ? s.dark / s.occluded : 0.0, s.dark_wrong,
                   unproven > 0 ? (s.lit_new - s.lit_old + s.dark) / unproven : 0.0,
                   unproven > 0 ? (s.lit_new - s.lit_old) / unproven : 0.0, unproven > 0 ? s.dark / unproven : 0.0);
        }
        printf("}\n");
        fflush(stdout);
    }
    return 0;
}
