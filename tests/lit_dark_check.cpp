// Host check of the lit table's single-triangle cover predicate (pt_lit.h lit_tri_covers) and of the
// per-cell margin (lit_margin_cell), plain C++ without device code.  Build with -ffp-contract=off:
// the fp32 replica below keeps the tracer's operation order (pt_device.h tri_test, tri_accept,
// tri_box_padded, ray_inv; pt_math.h normalize, length; the shading kernels' shadow ray).
//
// Wherever the predicate says "covered", every shadow ray of the cell must hit for the replica:
// several thousand rays per case from random points of the cell, its corners, and points on its
// border moved one ulp outward.  Prints one JSON line; "bad" must be 0.
#include <cstdio>
#include <cstring>
#include <random>

#include "pt_lit.h"

using namespace pt;

struct V3 {
    float x, y, z;
};
static V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
static V3 operator*(float s, V3 a) { return {a.x * s, a.y * s, a.z * s}; }
static float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V3 normalize(V3 a) { return a * (1.0f / sqrtf(dot(a, a))); }
static float length(V3 a) { return sqrtf(dot(a, a)); }

static float box_pad(float x) { return fabsf(x) * 9.5367431640625e-7f + 1e-6f; }
static float ray_inv(float d) { return d != 0.0f ? 1.0f / d : copysignf(1e30f, d); }

// tri_test followed by tri_accept_in (t clamped into the triangle's slab interval, then 0 <= t <= tmax)
static bool tracer_hits(V3 v0, V3 e1, V3 e2, V3 o, V3 d, float tmax) {
    const V3 p = cross(d, e2);
    const float det = dot(e1, p);
    const float inv = 1.0f / det;
    const V3 tv = o - v0;
    const float u = dot(tv, p) * inv;
    const V3 q = cross(tv, e1);
    const float v = dot(d, q) * inv;
    float t = dot(e2, q) * inv;
    const bool hit = (det != 0.0f) & !(u < 0.0f || u > 1.0f) & !(v < 0.0f || u + v > 1.0f);
    if (!hit) return false;
    const float a[3] = {v0.x, v0.y, v0.z}, b[3] = {e1.x, e1.y, e1.z}, c[3] = {e2.x, e2.y, e2.z};
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        const float p1 = a[k] + b[k], p2 = a[k] + c[k];
        const float l = fminf(fminf(a[k], p1), p2), h = fmaxf(fmaxf(a[k], p1), p2);
        lo[k] = l - box_pad(l);
        hi[k] = h + box_pad(h);
    }
    const V3 iv = {ray_inv(d.x), ray_inv(d.y), ray_inv(d.z)};
    const V3 io = {o.x * iv.x, o.y * iv.y, o.z * iv.z};
    const float ax = fmaf(lo[0], iv.x, -io.x), bx = fmaf(hi[0], iv.x, -io.x);
    const float ay = fmaf(lo[1], iv.y, -io.y), by = fmaf(hi[1], iv.y, -io.y);
    const float az = fmaf(lo[2], iv.z, -io.z), bz = fmaf(hi[2], iv.z, -io.z);
    const float K = 1.000244140625f;
    const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
    const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    const float tfk = tf * K;
    if (!(tn <= tfk) || !(fabsf(t) <= 3.4028235e38f)) return false;
    t = !(tn <= t * K) ? tn : (!(t <= tfk) ? tf : t);
    return t >= 0.0f && t <= tmax;
}

// The shading kernels' shadow ray from the barycentric point (u, v) of T (reconstruct, k_shade_fused).
// False: the kernels would not use the table there (the light not above the offset side).
static bool shadow_ray(V3 v0, V3 v1, V3 v2, float u, float v, V3 l, V3& o, V3& d, float& tmax) {
    const V3 e1 = v1 - v0, e2 = v2 - v0;
    const float w = 1.0f - u - v;
    const V3 p = {w * v0.x + u * v1.x + v * v2.x, w * v0.y + u * v1.y + v * v2.y, w * v0.z + u * v1.z + v * v2.z};
    V3 ng = cross(e1, e2);
    const V3 ldir = l - p;
    if (dot(ldir, ng) < 0.0f) ng = ng * -1.0f;  // the viewer sits on the light's side of T
    ng = normalize(ng);
    if (!(dot(ldir, ng) > kLitDelta)) return false;
    o = p + 1e-3f * ng;
    d = normalize(ldir);
    tmax = length(ldir);
    return true;
}

static std::mt19937_64 rng(20241);
static double uni(double a, double b) { return a + (b - a) * std::uniform_real_distribution<double>(0.0, 1.0)(rng); }

struct Case {
    V3 v0, v1, v2;  // T
    int k;
    uint32_t cell;
    V3 l;
    V3 u0, u1, u2;  // U
};

static bool covers(const Case& c, LitPyramid& P, float diag) {
    const V3 e1 = c.v1 - c.v0, e2 = c.v2 - c.v0;
    const float a0[3] = {c.v0.x, c.v0.y, c.v0.z}, a1[3] = {e1.x, e1.y, e1.z}, a2[3] = {e2.x, e2.y, e2.z};
    const float lp[3] = {c.l.x, c.l.y, c.l.z};
    const float m = lit_margin_cell(diag, lit_cell_reach(a0, a1, a2, c.k, c.cell, lp));
    if (!lit_pyramid(a0, a1, a2, c.k, c.cell, lp, kLitDelta, m, P) || !lit_dark_possible(P)) return false;
    const V3 f1 = c.u1 - c.u0, f2 = c.u2 - c.u0;  // U as the tracer holds it: v0 and two fp32 edges
    const double a[3] = {c.u0.x, c.u0.y, c.u0.z};
    const double b[3] = {(double)c.u0.x + f1.x, (double)c.u0.y + f1.y, (double)c.u0.z + f1.z};
    const double cc[3] = {(double)c.u0.x + f2.x, (double)c.u0.y + f2.y, (double)c.u0.z + f2.z};
    return lit_tri_covers(P, a, b, cc);
}

// Rays of the cell against U; returns the number that miss.
static long shoot(const Case& c, int n, long& shot) {
    int cu[3], cv[3];
    lit_cell_corners(c.k, c.cell, cu, cv);
    const float N = (float)(1 << c.k);
    const V3 f1 = c.u1 - c.u0, f2 = c.u2 - c.u0;
    long miss = 0;
    for (int i = 0; i < n; ++i) {
        double w[3];
        if (i < 3) {
            w[0] = i == 0, w[1] = i == 1, w[2] = i == 2;
        } else if (i % 4 == 0) {  // on a border
            const int s = (i / 4) % 3;
            const double t = uni(0, 1);
            w[s] = t, w[(s + 1) % 3] = 1 - t, w[(s + 2) % 3] = 0;
        } else {
            double a = uni(0, 1), b = uni(0, 1);
            if (a + b > 1) a = 1 - a, b = 1 - b;
            w[0] = a, w[1] = b, w[2] = 1 - a - b;
        }
        float u = (float)((w[0] * cu[0] + w[1] * cu[1] + w[2] * cu[2]) / N);
        float v = (float)((w[0] * cv[0] + w[1] * cv[1] + w[2] * cv[2]) / N);
        if (i % 4 == 0 && i >= 3) {  // one ulp outward, whichever way that is for this border
            const int s = (i / 8) % 4;
            u = nextafterf(u, (s & 1) ? 2.0f : -1.0f);
            v = nextafterf(v, (s & 2) ? 2.0f : -1.0f);
            if (u < 0.0f || v < 0.0f || u + v > 1.0f) continue;  // not a hit the tracer can report
            // the point must still belong to this cell or to one that shares the border: the kernels
            // read the bit of the cell lit_cell_index names, so only rays of this cell count
            if (lit_cell_index(c.k, u, v) != c.cell) continue;
        } else if (lit_cell_index(c.k, u, v) != c.cell) {
            continue;
        }
        V3 o, d;
        float tmax;
        if (!shadow_ray(c.v0, c.v1, c.v2, u, v, c.l, o, d, tmax)) continue;
        ++shot;
        if (!tracer_hits(c.u0, f1, f2, o, d, tmax)) ++miss;
    }
    return miss;
}

static V3 rnd_dir() {
    for (;;) {
        const V3 d = {(float)uni(-1, 1), (float)uni(-1, 1), (float)uni(-1, 1)};
        const float l = length(d);
        if (l > 0.1f && l < 1.0f) return d * (1.0f / l);
    }
}

int main() {
    long bad = 0, covered = 0, tried = 0, shot = 0, refused_ok = 0;
    const float diag = 12.0f;
    // ---- random cells, lights and single triangles
    for (int it = 0; it < 25000; ++it) {
        Case c;
        const float S = (float)uni(-40, 40) * (it % 3 == 0);  // some cases far from the origin: larger ulps
        const V3 base = {S + (float)uni(-2, 2), S * 0.5f + (float)uni(-2, 2), (float)uni(-2, 2)};
        c.v0 = base;
        c.v1 = base + rnd_dir() * (float)uni(0.2, 3.0);
        c.v2 = base + rnd_dir() * (float)uni(0.2, 3.0);
        c.k = (int)uni(0, 8.99);
        c.cell = (uint32_t)uni(0, (double)lit_cells(c.k) - 0.01);
        const V3 n = normalize(cross(c.v1 - c.v0, c.v2 - c.v0));
        if (!(length(cross(c.v1 - c.v0, c.v2 - c.v0)) > 0.02f)) continue;
        int cu[3], cv[3];
        lit_cell_corners(c.k, c.cell, cu, cv);
        const float N = (float)(1 << c.k);
        const float gu = (cu[0] + cu[1] + cu[2]) / (3 * N), gv = (cv[0] + cv[1] + cv[2]) / (3 * N);
        const V3 g = c.v0 + (c.v1 - c.v0) * gu + (c.v2 - c.v0) * gv;
        const V3 dir = normalize(n * (float)uni(0.3, 1.0) + rnd_dir() * (float)uni(0.0, 0.8));
        if (dot(dir, n) < 0.05f) continue;
        c.l = g + dir * (float)uni(0.05, 6.0);
        // U: a triangle around a point of the central ray, from tiny against the bundle to much larger
        const V3 x = g + (c.l - g) * (float)uni(0.02, 0.98);
        const float width = length(c.v1 - c.v0) / N;
        const float size = width * (float)std::exp(uni(std::log(0.3), std::log(40.0)));
        const V3 un = normalize(dir * (float)uni(0.0, 1.0) + rnd_dir() * (float)uni(0.0, 1.0));
        V3 t1 = cross(un, rnd_dir());
        if (length(t1) < 0.1f) continue;
        t1 = normalize(t1);
        const V3 t2 = cross(un, t1);
        const double a0 = uni(0, 6.28), a1 = a0 + uni(1.2, 2.9), a2 = a1 + uni(1.2, 2.9);
        const V3 off = (t1 * (float)uni(-0.3, 0.3) + t2 * (float)uni(-0.3, 0.3)) * size;
        c.u0 = x + off + (t1 * (float)cos(a0) + t2 * (float)sin(a0)) * size;
        c.u1 = x + off + (t1 * (float)cos(a1) + t2 * (float)sin(a1)) * size;
        c.u2 = x + off + (t1 * (float)cos(a2) + t2 * (float)sin(a2)) * size;
        ++tried;
        LitPyramid P;
        if (!covers(c, P, diag)) continue;
        ++covered;
        const long miss = shoot(c, covered <= 400 ? 4000 : 200, shot);
        if (miss) {
            ++bad;
            fprintf(stderr, "covered case %d: %ld rays miss\n", it, miss);
        }
    }
    // ---- cases that must be refused, on a floor cell under a light at height 2
    {
        Case c;
        c.v0 = {0, 0, 0}, c.v1 = {1, 0, 0}, c.v2 = {0, 1, 0};
        c.k = 3, c.cell = 0;  // corners (0,0) (1/8,0) (0,1/8)
        c.l = {0.04f, 0.04f, 2.0f};
        LitPyramid P;
        auto U = [&](V3 a, V3 b, V3 d) { c.u0 = a, c.u1 = b, c.u2 = d; return covers(c, P, diag); };
        // a generous blocker at z = 1 covers (the refusals below are not vacuous)
        if (!U({-2, -2, 1}, {3, -2, 1}, {-2, 3, 1})) ++bad, fprintf(stderr, "plain blocker refused\n"); else ++refused_ok;
        // the bundle straddles an edge of U (x = 0.03 at z = 1 cuts the bundle, which spans x in [0.02, 0.0825])
        if (U({0.03f, -2, 1}, {3, -2, 1}, {0.03f, 3, 1})) ++bad, fprintf(stderr, "straddling accepted\n"); else ++refused_ok;
        // U behind the light
        if (U({-2, -2, 2.5f}, {3, -2, 2.5f}, {-2, 3, 2.5f})) ++bad, fprintf(stderr, "behind the light accepted\n"); else ++refused_ok;
        // U closer to the origin plane than the clearance (the origins sit at z = 1e-3)
        if (U({-2, -2, 1.1e-3f}, {3, -2, 1.1e-3f}, {-2, 3, 1.1e-3f})) ++bad, fprintf(stderr, "no clearance accepted\n"); else ++refused_ok;
        // ... and closer to the light's end than the clearance
        if (U({-2, -2, 2.001f}, {3, -2, 2.001f}, {-2, 3, 2.001f})) ++bad, fprintf(stderr, "no end clearance accepted\n"); else ++refused_ok;
        // grazing: a steep plane x cos a + z sin a = c through the bundle of a smaller cell, the rays
        // nearly vertical, so |cos| between rays and U's normal is ~sin a: 0.1 is below the bound of
        // 1/8 and refused, the same construction at 0.3 is accepted
        auto steep = [&](double sa, double cc_) {
            const double ca = sqrt(1 - sa * sa);
            auto pt = [&](double s, double r) { return V3{(float)(cc_ * ca - r * sa), (float)s, (float)(cc_ * sa + r * ca)}; };
            return U(pt(-1.5, -1.5), pt(1.5, -1.5), pt(0, 2));
        };
        c.k = 5, c.l = {0.01f, 0.01f, 2.0f};
        if (steep(0.1, 0.12)) ++bad, fprintf(stderr, "grazing accepted\n"); else ++refused_ok;
        if (!steep(0.3, 0.3)) ++bad, fprintf(stderr, "cos 0.3 refused\n"); else ++refused_ok;
        c.k = 3, c.l = {0.04f, 0.04f, 2.0f};
        // degenerate U: collinear vertices, and a sliver
        if (U({-2, -2, 1}, {0, 0, 1}, {2, 2, 1})) ++bad, fprintf(stderr, "degenerate accepted\n"); else ++refused_ok;
        if (U({-20, 0.04f, 1}, {20, 0.04f - 0.05f, 1}, {20, 0.04f + 0.05f, 1})) ++bad, fprintf(stderr, "sliver accepted\n"); else ++refused_ok;
        // a light within the margin of the surface
        c.l = {0.04f, 0.04f, 1.5e-3f};
        if (U({-2, -2, 1e-3f + 2.5e-4f}, {3, -2, 1e-3f + 2.5e-4f}, {-2, 3, 1e-3f + 2.5e-4f})) ++bad, fprintf(stderr, "low light accepted\n"); else ++refused_ok;
    }
    // ---- the per-cell margin
    long margins = 0;
    for (int it = 0; it < 20000; ++it) {
        const float dg = (float)std::exp(uni(std::log(1e-3), std::log(440.0)));
        const double reach = std::exp(uni(std::log(1e-4), std::log(450.0)));
        const float m = lit_margin_cell(dg, reach);
        ++margins;
        if (!(m <= lit_margin(dg)) || !(m > 2e-3f)) ++bad, fprintf(stderr, "margin %g of diag %g reach %g\n", m, dg, reach);
        // the derived bound: tri_accept's stretch t 2^-12 once, t <= min(reach, diag) + the 1e-3 overshoot
        const double need = 2e-3 + (fmin(reach, (double)dg) + 1e-3) / 4096.0;
        if (dg > 1e-2f && !((double)m >= need)) ++bad, fprintf(stderr, "margin %g below %g\n", m, need);
    }
    {  // cells at the far corners of a 100 x 80 x 60 box against a light in the opposite corner
        const float box[3] = {100, 80, 60};
        const float dg = sqrtf(box[0] * box[0] + box[1] * box[1] + box[2] * box[2]);
        for (int corner = 0; corner < 8; ++corner) {
            const float s[3] = {corner & 1 ? 1.f : -1.f, corner & 2 ? 1.f : -1.f, corner & 4 ? 1.f : -1.f};
            const float v0[3] = {s[0] * box[0] / 2, s[1] * box[1] / 2, s[2] * box[2] / 2};
            const float e1[3] = {-s[0] * 0.5f, 0, 0}, e2[3] = {0, -s[1] * 0.5f, 0};
            const float lp[3] = {-v0[0], -v0[1], -v0[2]};
            for (uint32_t cell = 0; cell < lit_cells(2); ++cell) {
                const double reach = lit_cell_reach(v0, e1, e2, 2, cell, lp);
                const float m = lit_margin_cell(dg, reach);
                ++margins;
                if (!(reach > dg * 0.99 && reach <= dg * 1.000001)) ++bad, fprintf(stderr, "reach %g\n", reach);
                if (!((double)m >= 2e-3 + (fmin(reach, (double)dg) + 1e-3) / 4096.0) || !(m <= lit_margin(dg))) ++bad, fprintf(stderr, "corner margin %g\n", m);
            }
        }
    }
    printf("{\"bad\": %ld, \"tried\": %ld, \"covered\": %ld, \"rays\": %ld, \"refusals\": %ld, \"margins\": %ld}\n", bad, tried, covered,
           shot, refused_ok, margins);
    return bad ? 1 : 0;
}
