// Host check of the skip table's builder (optixpathtracer_amd/csrc/pt_skip.h), built by
// tests/test_skip_host.py with hipcc --cuda-host-only (no GPU), once plain and once under
// AddressSanitizer and UBSan.  For each scene -- a tetrahedron, a 12-triangle cube, an 8x4 UV sphere,
// two such spheres 0.07 apart, a concave L-prism, one planar quad, a soup of 200 random triangles (one
// of them a sliver) -- it builds the binned-SAH binary tree of pt_sah.cpp, collapses it into a BVH4 in
// the tracer's node layout, runs skip_parents_of and skip_word for every (triangle, side) and checks
// the word by brute force over the subtrees' triangle ranges, in fp64:
//   (a) the named link is on the triangle's root-to-leaf path;
//   (b) every triangle under it lies at or below the plane + kLitDelta on that side (heights
//       recomputed here, not taken from the header) and passes skip_tri_below;
//   (c) the next link up the path holds a triangle that does not pass;
//   (d) "none" only where T has no origin record or a triangle of T's own leaf does not pass.
// On the closed convex scenes (tetrahedron, cube, sphere) no outward side may be "none", so the
// sphere's outward words cover at least their own leaf.
// Four floor scenes (check_floor: a planar floor of 4608 or 18432 triangles under one sphere, with and
// without a sliver) take the walk to kSkipMaxTris: every word is safe against brute force and no lower
// than the budget allows, and without a sliver box_accept takes the floor's downward sides to a child of
// the root.
// Prints one JSON line: pairs checked, violations, and per scene the words that are "none".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "pt_internal.h"
#include "pt_skip.h"

namespace {

struct V {
    double x, y, z;
};
struct Tri {
    V a, b, c;
};

// outward = the stored winding's normal points away from `centre`
void push_outward(std::vector<Tri>& out, V a, V b, V c, V centre) {
    const V e1{b.x - a.x, b.y - a.y, b.z - a.z}, e2{c.x - a.x, c.y - a.y, c.z - a.z};
    const V n{e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
    const V m{(a.x + b.x + c.x) / 3 - centre.x, (a.y + b.y + c.y) / 3 - centre.y, (a.z + b.z + c.z) / 3 - centre.z};
    if (n.x * m.x + n.y * m.y + n.z * m.z < 0) std::swap(b, c);
    out.push_back({a, b, c});
}

std::vector<Tri> tetrahedron() {
    const V p[4] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
    std::vector<Tri> t;
    const int f[4][3] = {{0, 1, 2}, {0, 3, 1}, {0, 2, 3}, {1, 3, 2}};
    for (auto& q : f) push_outward(t, p[q[0]], p[q[1]], p[q[2]], {0, 0, 0});
    return t;
}

std::vector<Tri> cube(V lo, V hi) {
    std::vector<Tri> t;
    const V c{(lo.x + hi.x) / 2, (lo.y + hi.y) / 2, (lo.z + hi.z) / 2};
    auto P = [&](int i) { return V{i & 1 ? hi.x : lo.x, i & 2 ? hi.y : lo.y, i & 4 ? hi.z : lo.z}; };
    const int q[6][4] = {{0, 1, 3, 2}, {4, 5, 7, 6}, {0, 1, 5, 4}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 3, 7, 5}};
    for (auto& f : q) {
        push_outward(t, P(f[0]), P(f[1]), P(f[2]), c);
        push_outward(t, P(f[0]), P(f[2]), P(f[3]), c);
    }
    return t;
}

std::vector<Tri> uv_sphere(V c, double r, int seg, int rings) {
    std::vector<Tri> t;
    auto P = [&](int i, int j) {
        const double th = M_PI * j / rings, ph = 2 * M_PI * (i % seg) / seg;
        return V{c.x + r * std::sin(th) * std::cos(ph), c.y + r * std::sin(th) * std::sin(ph), c.z + r * std::cos(th)};
    };
    for (int j = 0; j < rings; ++j)
        for (int i = 0; i < seg; ++i) {
            if (j > 0) push_outward(t, P(i, j), P(i + 1, j), P(i + 1, j + 1), c);
            if (j + 1 < rings) push_outward(t, P(i, j), P(i + 1, j + 1), P(i, j + 1), c);
        }
    return t;
}

// An L-shaped prism: the L in the xy plane (a 2 x 2 square less its upper right quarter, listed
// counter-clockwise), height 1: six side rectangles and two caps of three unit squares each.
std::vector<Tri> l_prism() {
    std::vector<Tri> t;
    const double xs[7] = {0, 2, 2, 1, 1, 0, 0}, ys[7] = {0, 0, 1, 1, 2, 2, 0};
    for (int k = 0; k < 6; ++k) {
        const V p0{xs[k], ys[k], 0}, p1{xs[k + 1], ys[k + 1], 0}, p2{xs[k + 1], ys[k + 1], 1}, p3{xs[k], ys[k], 1};
        const double dx = p1.x - p0.x, dy = p1.y - p0.y, len = std::sqrt(dx * dx + dy * dy);
        // a point just inside the L next to this side: the inward normal of a counter-clockwise edge
        const V in{(p0.x + p1.x) / 2 - 1e-3 * dy / len, (p0.y + p1.y) / 2 + 1e-3 * dx / len, 0.5};
        push_outward(t, p0, p1, p2, in);
        push_outward(t, p0, p2, p3, in);
    }
    const double sq[3][2] = {{0, 0}, {1, 0}, {0, 1}};
    for (auto& s : sq)
        for (int z = 0; z < 2; ++z) {
            const V p0{s[0], s[1], (double)z}, p1{s[0] + 1, s[1], (double)z}, p2{s[0] + 1, s[1] + 1, (double)z},
                p3{s[0], s[1] + 1, (double)z};
            const V in{s[0] + 0.5, s[1] + 0.5, 0.5};
            push_outward(t, p0, p1, p2, in);
            push_outward(t, p0, p2, p3, in);
        }
    return t;
}

std::vector<Tri> quad() { return {{{0, 0, 0}, {1, 0, 0}, {1, 1, 0}}, {{0, 0, 0}, {1, 1, 0}, {0, 1, 0}}}; }

std::vector<Tri> soup(int n) {
    std::mt19937 g(12345);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::normal_distribution<double> s(0.0, 0.15);
    std::vector<Tri> t;
    for (int k = 0; k < n; ++k) {
        const V c{u(g), u(g), u(g)};
        auto p = [&] { return V{c.x + s(g), c.y + s(g), c.z + s(g)}; };
        t.push_back({p(), p(), p()});
    }
    t[7].c = V{t[7].a.x + (t[7].b.x - t[7].a.x) * 0.5, t[7].a.y + (t[7].b.y - t[7].a.y) * 0.5 + 1e-6,
               t[7].a.z + (t[7].b.z - t[7].a.z) * 0.5};  // a sliver: it must block every skip over it
    return t;
}

struct Node {  // pt_device.h BNode4 as plain words
    float lox[4], hix[4], loy[4], hiy[4], loz[4], hiz[4];
    int child[4], pad[4];
};
static_assert(sizeof(Node) == 4 * pt::kSkipNodeWords, "the node layout pt_skip.h walks");

struct Bvh4 {
    std::vector<Node> nodes;
    std::vector<float> isect;  // 12 floats per leaf-order triangle
    std::vector<int> lo, hi;   // per node: its leaf-order triangle range [lo, hi]
    int ntri = 0;
};

Bvh4 build(const std::vector<Tri>& tris) {
    const int n = (int)tris.size();
    std::vector<float4> t4(3 * (size_t)n);
    for (int k = 0; k < n; ++k) {
        const V* p[3] = {&tris[k].a, &tris[k].b, &tris[k].c};
        for (int v = 0; v < 3; ++v) t4[3 * (size_t)k + v] = make_float4((float)p[v]->x, (float)p[v]->y, (float)p[v]->z, 0.0f);
    }
    std::vector<uint32_t> order;
    std::vector<int2> child, range;
    std::vector<float4> box;
    pt::sah_binary_tree(t4.data(), n, order, child, range, box);
    Bvh4 B;
    B.ntri = n;
    B.isect.resize(12 * (size_t)n);
    for (int k = 0; k < n; ++k) {
        const float4 a = t4[3 * (size_t)order[k]], b = t4[3 * (size_t)order[k] + 1], c = t4[3 * (size_t)order[k] + 2];
        const float r[12] = {a.x, a.y, a.z, 0, b.x - a.x, b.y - a.y, b.z - a.z, 0, c.x - a.x, c.y - a.y, c.z - a.z, 0};
        std::memcpy(&B.isect[12 * (size_t)k], r, sizeof r);
    }
    auto lo_of = [&](int c) { return c >= 0 ? range[c].x : ~c; };
    auto hi_of = [&](int c) { return c >= 0 ? range[c].y : ~c; };
    auto is_leaf = [&](int c) { return c < 0 || hi_of(c) - lo_of(c) + 1 <= 3; };  // leaves of 1 to 3 triangles
    // breadth-first: binary node b becomes BVH4 node q[b]
    std::vector<int> work = {0};
    B.nodes.push_back(Node{});
    B.lo.push_back(0);
    B.hi.push_back(n - 1);
    for (size_t w = 0; w < work.size(); ++w) {
        std::vector<int> kids = {child[work[w]].x, child[work[w]].y};
        while (kids.size() < 4) {  // open the inner child with the most triangles
            int best = -1, bn = 0;
            for (size_t k = 0; k < kids.size(); ++k)
                if (!is_leaf(kids[k]) && hi_of(kids[k]) - lo_of(kids[k]) > bn) {
                    bn = hi_of(kids[k]) - lo_of(kids[k]);
                    best = (int)k;
                }
            if (best < 0) break;
            const int c = kids[(size_t)best];
            kids[(size_t)best] = child[c].x;
            kids.push_back(child[c].y);
        }
        Node nd;
        for (int q = 0; q < 4; ++q) {
            nd.lox[q] = nd.loy[q] = nd.loz[q] = INFINITY;  // an empty slot's inverted box
            nd.hix[q] = nd.hiy[q] = nd.hiz[q] = -INFINITY;
            nd.child[q] = pt::kSkipEmptyChild;
            nd.pad[q] = 0;
        }
        for (size_t q = 0; q < kids.size(); ++q) {
            const int c = kids[q], first = lo_of(c), cnt = hi_of(c) - first + 1;
            for (int k = first; k < first + cnt; ++k) {  // the union of the padded triangle boxes
                const float* r = &B.isect[12 * (size_t)k];
                float l[3], h[3];
                pt::tri_box_padded(pt::mk(r[0], r[1], r[2]), pt::mk(r[4], r[5], r[6]), pt::mk(r[8], r[9], r[10]), l, h);
                nd.lox[q] = std::fmin(nd.lox[q], l[0]); nd.hix[q] = std::fmax(nd.hix[q], h[0]);
                nd.loy[q] = std::fmin(nd.loy[q], l[1]); nd.hiy[q] = std::fmax(nd.hiy[q], h[1]);
                nd.loz[q] = std::fmin(nd.loz[q], l[2]); nd.hiz[q] = std::fmax(nd.hiz[q], h[2]);
            }
            if (is_leaf(c)) {
                nd.child[q] = ~((first << 3) | (cnt - 1));
            } else {
                nd.child[q] = (int)B.nodes.size();
                B.nodes.push_back(Node{});
                B.lo.push_back(first);
                B.hi.push_back(first + cnt - 1);
                work.push_back(c);
            }
        }
        B.nodes[w] = nd;
    }
    return B;
}

// Heights over T's plane on `side`, from scratch: the plane through the three vertices as the hit test
// sees them, unit normal e1 x e2 (negated for side 1).
bool heights_below(const Bvh4& B, int t, int side, int u) {
    double a[3], b[3], c[3], ua[3], ub[3], uc[3];
    pt::skip_tri_vertices(B.isect.data(), t, a, b, c);
    pt::skip_tri_vertices(B.isect.data(), u, ua, ub, uc);
    const long double e1[3] = {(long double)b[0] - a[0], (long double)b[1] - a[1], (long double)b[2] - a[2]};
    const long double e2[3] = {(long double)c[0] - a[0], (long double)c[1] - a[1], (long double)c[2] - a[2]};
    long double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const long double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(len > 0)) return false;
    for (auto& x : n) x = (side ? -x : x) / len;
    const double* p[3] = {ua, ub, uc};
    for (auto q : p) {
        const long double h = n[0] * (q[0] - a[0]) + n[1] * (q[1] - a[1]) + n[2] * (q[2] - a[2]);
        if (!(h <= (long double)pt::kLitDelta + 1e-12L)) return false;
    }
    return true;
}

struct Result {
    long checked = 0, bad = 0, none = 0, none_outward = 0;
};

Result check(const char* name, const std::vector<Tri>& tris, bool convex) {
    Result R;
    const Bvh4 B = build(tris);
    const int n = B.ntri, nn = (int)B.nodes.size();
    auto fail = [&](const char* what, int t, int side) {
        if (R.bad++ < 8) std::fprintf(stderr, "%s: %s at triangle %d side %d\n", name, what, t, side);
    };
    std::vector<int> node_parent((size_t)nn, -2), tri_parent((size_t)n, -2);
    bool sliver = false;  // a scene with a sliver takes the walk without box_accept (the soup does)
    for (int i = 0; i < nn; ++i)
        sliver = pt::skip_parents_of(B.nodes.data(), B.isect.data(), i, node_parent.data(), tri_parent.data()) || sliver;
    if (sliver != (std::string(name) == "soup")) fail("the sliver flag", -1, 0);
    std::vector<int> stack(72);
    // the triangle range of a link
    auto range_of = [&](int link, int& lo, int& hi) {
        if (link >= 0) {
            lo = B.lo[(size_t)link];
            hi = B.hi[(size_t)link];
        } else {
            lo = pt::skip_leaf_first(link);
            hi = lo + pt::skip_leaf_count(link) - 1;
        }
    };
    auto all_pass = [&](const pt::SkipOrigin& T, int lo, int hi) {
        for (int u = lo; u <= hi; ++u) {
            double a[3], b[3], c[3];
            pt::skip_tri_vertices(B.isect.data(), u, a, b, c);
            if (!pt::skip_tri_below(T, a, b, c)) return false;
        }
        return true;
    };
    for (int t = 0; t < n; ++t)
        for (int side = 0; side < 2; ++side) {
            ++R.checked;
            const uint32_t w = pt::skip_word(B.nodes.data(), B.isect.data(), node_parent.data(), tri_parent.data(), t,
                                             side, stack.data(), 1, (int)stack.size(), !sliver);
            pt::SkipOrigin T;
            const bool has_origin = pt::skip_origin(B.isect.data(), t, side, T);
            const int at = tri_parent[(size_t)t];
            if (at < 0 || (at >> 2) >= nn) {
                fail("triangle without a leaf", t, side);
                continue;
            }
            const int leaf = B.nodes[(size_t)(at >> 2)].child[at & 3];
            if (w == pt::kSkipNone) {
                ++R.none;
                if (side == 0) ++R.none_outward;
                int lo, hi;
                range_of(leaf, lo, hi);
                if (has_origin && all_pass(T, lo, hi)) fail("(d) none although the leaf passes", t, side);
                if (convex && side == 0) fail("an outward side of a convex scene is none", t, side);
                continue;
            }
            if (!has_origin) {
                fail("a word for a triangle without an origin record", t, side);
                continue;
            }
            const int link = (int)w;
            int lo, hi;
            // (a) on the path: the link is a real link whose range holds t
            bool real = false;
            int holder = -1;
            for (int i = 0; i < nn && !real; ++i)
                for (int q = 0; q < 4; ++q)
                    if (B.nodes[(size_t)i].child[q] == link && link != pt::kSkipEmptyChild) {
                        real = true;
                        holder = i;
                    }
            if (!real) {
                fail("(a) the word is no link of the tree", t, side);
                continue;
            }
            range_of(link, lo, hi);
            if (t < lo || t > hi) fail("(a) the link is not on the triangle's path", t, side);
            // (b)
            for (int u = lo; u <= hi; ++u)
                if (!heights_below(B, t, side, u)) {
                    fail("(b) a triangle under the link is above the plane", t, side);
                    break;
                }
            if (!all_pass(T, lo, hi)) fail("(b) a triangle under the link does not pass", t, side);
            // (c) the next link up is the holder node's own link (the root has none)
            if (holder != 0 && all_pass(T, B.lo[(size_t)holder], B.hi[(size_t)holder]))
                fail("(c) a higher link passes", t, side);
        }
    std::printf("\"%s\": {\"triangles\": %d, \"nodes\": %d, \"none\": %ld, \"none_outward\": %ld}, ", name, n, nn, R.none,
                R.none_outward);
    return R;
}

// A planar floor of quads x quads squares over [-2.4, 2.4]^2 at z = 0 (stored normals +z), one 8x4 sphere
// above its middle and, with `sliver`, one triangle of aspect 2^-8 away from both.
std::vector<Tri> floor_scene(int quads, bool sliver) {
    std::vector<Tri> t;
    const double s = 4.8 / quads;
    for (int i = 0; i < quads; ++i)
        for (int j = 0; j < quads; ++j) {
            const double x = -2.4 + s * i, y = -2.4 + s * j;
            push_outward(t, {x, y, 0}, {x + s, y, 0}, {x + s, y + s, 0}, {x, y, -1});
            push_outward(t, {x, y, 0}, {x + s, y + s, 0}, {x, y + s, 0}, {x, y, -1});
        }
    const std::vector<Tri> ball = uv_sphere({0, 0, 0.5}, 0.2, 8, 4);
    t.insert(t.end(), ball.begin(), ball.end());
    if (sliver) t.push_back({{3.5, 0, 1}, {4.5, 0, 1}, {4.0, 0.00390625, 1}});
    return t;
}

// The floor scenes: large flat regions, where one walk can meet more than kSkipMaxTris triangles.  For
// every `stride`-th triangle and both sides, the predicate is restated here for all triangles under the
// path's highest link (heights in long double from the vertices, aspect as smallest height over longest
// edge) and counted in prefix sums, so that every link of the path is decided by brute force:
//   (a) the word is on the triangle's path; (b) it is not above the highest link that passes, and the
//   header's own predicate passes for every triangle under it; (e) it is not below the highest passing
//   link with at most kSkipMaxTris - 1 triangles under it -- one walk looks at a triangle once, so the
//   budget cannot run out at or below that link.
// Counted for the caller: the floor's downward sides and how many of them name a child of the root
// (all of them without a sliver: box_accept spends no budget), and the words the budget kept lower than
// the link brute force allows.
struct FloorResult {
    Result r;
    long down = 0, down_root_child = 0, kept_low = 0;
};

FloorResult check_floor(const char* name, const std::vector<Tri>& tris, bool with_sliver, int stride) {
    FloorResult F;
    Result& R = F.r;
    const Bvh4 B = build(tris);
    const int n = B.ntri, nn = (int)B.nodes.size();
    auto fail = [&](const char* what, int t, int side) {
        if (R.bad++ < 8) std::fprintf(stderr, "%s: %s at triangle %d side %d\n", name, what, t, side);
    };
    std::vector<int> node_parent((size_t)nn, -2), tri_parent((size_t)n, -2);
    bool sliver = false;
    for (int i = 0; i < nn; ++i)
        sliver = pt::skip_parents_of(B.nodes.data(), B.isect.data(), i, node_parent.data(), tri_parent.data()) || sliver;
    if (sliver != with_sliver) fail("the sliver flag", -1, 0);
    // every triangle once: vertices, whether it counts (aspect >= 2^-6), whether it has words (>= 2^-10)
    std::vector<double> vtx(9 * (size_t)n);
    std::vector<char> counts((size_t)n), origin((size_t)n), on_floor((size_t)n);
    for (int u = 0; u < n; ++u) {
        double* p = &vtx[9 * (size_t)u];
        pt::skip_tri_vertices(B.isect.data(), u, p, p + 3, p + 6);
        long double len[3], area2;
        {
            const long double e1[3] = {(long double)p[3] - p[0], (long double)p[4] - p[1], (long double)p[5] - p[2]};
            const long double e2[3] = {(long double)p[6] - p[0], (long double)p[7] - p[1], (long double)p[8] - p[2]};
            const long double e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
            const long double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            area2 = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            len[0] = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
            len[1] = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
            len[2] = std::sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
        }
        const long double longest = std::fmax(len[0], std::fmax(len[1], len[2]));
        const long double aspect = longest > 0 ? (area2 / longest) / longest : 0;  // smallest height / longest edge
        counts[(size_t)u] = aspect >= 0.015625L;
        origin[(size_t)u] = aspect >= 0.0009765625L;
        on_floor[(size_t)u] = p[2] == 0 && p[5] == 0 && p[8] == 0;
    }
    auto range_of = [&](int link, int& lo, int& hi) {
        if (link >= 0) {
            lo = B.lo[(size_t)link];
            hi = B.hi[(size_t)link];
        } else {
            lo = pt::skip_leaf_first(link);
            hi = lo + pt::skip_leaf_count(link) - 1;
        }
    };
    std::vector<int> stack(72), pre((size_t)n + 1), path;
    for (int t = 0; t < n; t += stride)
        for (int side = 0; side < 2; ++side) {
            ++R.checked;
            const uint32_t w = pt::skip_word(B.nodes.data(), B.isect.data(), node_parent.data(), tri_parent.data(), t,
                                             side, stack.data(), 1, (int)stack.size(), !sliver);
            path.clear();  // the links from the leaf up to the root's child
            for (int at = tri_parent[(size_t)t];; at = node_parent[(size_t)(at >> 2)]) {
                path.push_back(B.nodes[(size_t)(at >> 2)].child[at & 3]);
                if ((at >> 2) == 0) break;
            }
            const double* a = &vtx[9 * (size_t)t];
            const long double e1[3] = {(long double)a[3] - a[0], (long double)a[4] - a[1], (long double)a[5] - a[2]};
            const long double e2[3] = {(long double)a[6] - a[0], (long double)a[7] - a[1], (long double)a[8] - a[2]};
            long double nr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const long double len = std::sqrt(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
            const bool has = origin[(size_t)t] && len > 0;
            for (auto& x : nr) x = (side ? -x : x) / (len > 0 ? len : 1);
            const long double top = nr[0] * a[0] + nr[1] * a[1] + nr[2] * a[2] + (long double)pt::kLitDelta;
            int first, last, passed = 0;  // every link of the path lies inside the highest one's range
            range_of(path.back(), first, last);
            const double* q = &vtx[9 * (size_t)first];
            pre[(size_t)first] = 0;
            for (int u = first; u <= last; ++u, q += 9) {
                bool ok = has && counts[(size_t)u];
                for (int k = 0; k < 9 && ok; k += 3) ok = nr[0] * q[k] + nr[1] * q[k + 1] + nr[2] * q[k + 2] <= top;
                pre[(size_t)u + 1] = passed += ok ? 1 : 0;
            }
            int allowed = -1, floor = -1, got = -1;  // heights on the path, -1 = none
            for (int k = 0; k < (int)path.size(); ++k) {
                int lo, hi;
                range_of(path[(size_t)k], lo, hi);
                if (pre[(size_t)hi + 1] - pre[(size_t)lo] != hi - lo + 1) break;
                allowed = k;
                if (hi - lo + 1 <= pt::kSkipMaxTris - 1) floor = k;
            }
            if (w != pt::kSkipNone) {
                for (int k = 0; k < (int)path.size(); ++k)
                    if (path[(size_t)k] == (int)w) got = k;
                if (got < 0) {
                    fail("(a) the word is not on the triangle's path", t, side);
                    continue;
                }
                pt::SkipOrigin T;
                int lo, hi;
                range_of((int)w, lo, hi);
                bool pass = pt::skip_origin(B.isect.data(), t, side, T);
                for (int u = lo; u <= hi && pass; ++u)
                    pass = pt::skip_tri_below(T, &vtx[9 * (size_t)u], &vtx[9 * (size_t)u + 3], &vtx[9 * (size_t)u + 6]);
                if (!pass) fail("(b) a triangle under the link does not pass the header's predicate", t, side);
            } else {
                ++R.none;
                if (side == 0) ++R.none_outward;
            }
            if (got > allowed) fail("(b) a triangle under the link is not below", t, side);
            if (got < floor) fail("(e) the word is lower than the budget allows", t, side);
            if (got < allowed) ++F.kept_low;
            if (on_floor[(size_t)t] && nr[2] < 0) {  // nr points to `side`
                ++F.down;
                if (got == (int)path.size() - 1) ++F.down_root_child;
            }
        }
    std::printf("\"%s\": {\"triangles\": %d, \"nodes\": %d, \"none\": %ld, \"none_outward\": %ld, \"checked\": %ld, "
                "\"down\": %ld, \"down_root_child\": %ld, \"kept_low\": %ld}, ",
                name, n, nn, R.none, R.none_outward, R.checked, F.down, F.down_root_child, F.kept_low);
    return F;
}

}  // namespace

int main() {
    std::printf("{");
    Result tot;
    auto add = [&](Result r) {
        tot.checked += r.checked;
        tot.bad += r.bad;
        tot.none += r.none;
    };
    add(check("tetrahedron", tetrahedron(), true));
    add(check("cube", cube({-1, -1, -1}, {1, 1, 1}), true));
    add(check("sphere", uv_sphere({0, 0, 0}, 0.2, 8, 4), true));
    std::vector<Tri> two = uv_sphere({0, 0, 0}, 0.2, 8, 4);
    const std::vector<Tri> other = uv_sphere({0.47, 0, 0}, 0.2, 8, 4);  // 0.07 between the surfaces
    two.insert(two.end(), other.begin(), other.end());
    add(check("two_spheres", two, false));
    add(check("l_prism", l_prism(), false));
    add(check("quad", quad(), false));
    add(check("soup", soup(200), false));
    // 4608 floor triangles: more than kSkipMaxTris in the scene, every triangle and side
    add(check_floor("floor", floor_scene(48, false), false, 1).r);
    add(check_floor("floor_sliver", floor_scene(48, true), true, 1).r);
    // 18432: more than kSkipMaxTris under one child of the root, where the budget does run out; every 31st
    add(check_floor("wide_floor", floor_scene(96, false), false, 31).r);
    add(check_floor("wide_floor_sliver", floor_scene(96, true), true, 31).r);
    std::printf("\"checked\": %ld, \"none\": %ld, \"bad\": %ld}\n", tot.checked, tot.none, tot.bad);
    return tot.bad ? 1 : 0;
}
