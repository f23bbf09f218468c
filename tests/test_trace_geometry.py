"""The oracle's traced hits against float64 geometry (tests/trace_ref.py) on adversarial scenes
(tests/trace_scenes.py).  No GPU; never skips.

Every other trace test asks GPU == oracle, and both share one hit rule (fp32 Moller-Trumbore, then
tri_accept with its pad and slack).  This module asks what that cannot: whether the rule returns
the triangle the ray actually hits, at large coordinates, tiny and huge scales, through a model
matrix, on slivers, axis-aligned walls, coplanar duplicates and triangles without area.

Run with -s to see the worst error / (2^-24 cond) ratios per variant and ray set; the overall worst
stand in trace_ref's docstring and in DESIGN.md section 2.
"""
import ctypes as C

import numpy as np
import pytest

import trace_ref
import trace_scenes

CASES = [(v, k) for v in trace_scenes.VARIANTS for k in trace_scenes.RAY_SETS]


@pytest.fixture(scope="module")
def oracle_scenes():
    from oracle.oracle import OracleScene

    made = {}

    def get(name):
        if name not in made:
            made[name] = OracleScene(trace_scenes.make(name)[0])
        return made[name]

    yield get
    for o in made.values():
        o.close()


@pytest.mark.parametrize("variant,kind", CASES, ids=[f"{v}-{k}" for v, k in CASES])
def test_oracle_trace_meets_float64_contract(oracle_scenes, variant, kind):
    """slivers-interior is the case that found the dropped hit: until tri_accept clamped t into the
    triangle's slab interval instead of rejecting it, rays 370 and 696 went through slivers 75 and 12
    (m = 0.145 and 0.174 against bounds 0.090 and 0.014; 101.8 in units of 2^-24 cond_m against C = 8),
    because a grazing hit's fp32 t was off by 7e-4 relative, more than the slack K - 1 = 2.4e-4 on a
    slab interval 5e-4 long."""
    o = oracle_scenes(variant)
    sc = trace_scenes.make(variant)[0]
    tris = trace_scenes.world_triangles(sc)
    rays = trace_scenes.ray_set(variant, kind)
    assert len(rays) <= 2000 and len(tris) <= 2000
    closest = o.trace(rays)
    any_hit = o.trace(rays, any_hit=True)[0] >= 0
    trace_ref.assert_contract(tris, rays, closest, any_hit, f"oracle {variant}/{kind}")


@pytest.mark.parametrize("variant", trace_scenes.VARIANTS)
def test_oracle_answers_do_not_depend_on_the_bvh(oracle_scenes, variant):
    """The structure-independence the oracle claims: with the cull check on, every closest-hit trace
    is repeated without culling boxes by the running best t, and none may disagree."""
    o = oracle_scenes(variant)
    lib = o.lib
    lib.orc_set_cull_check.argtypes = [C.c_int32]
    lib.orc_cull_check_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    rays = np.concatenate([trace_scenes.ray_set(variant, k) for k in trace_scenes.RAY_SETS])
    plain = o.trace(rays)
    lib.orc_set_cull_check(1)
    try:
        checked = o.trace(rays)
        st, first = (C.c_uint64 * 2)(), (C.c_float * 16)()
        lib.orc_cull_check_stats(st, first)
    finally:
        lib.orc_set_cull_check(0)
    assert st[0] == len(rays)
    assert st[1] == 0, f"{st[1]} of {st[0]} traces change without the cull; first: {list(first)}"
    for a, b in zip(plain, checked):
        np.testing.assert_array_equal(a, b)


def test_reference_rejects_a_rule_without_pad_or_slack():
    """The check has teeth: a tracer that drops every hit on an axis-aligned wall (what tri_accept does
    with a zero pad and K = 1, whose boxes there have no thickness) fails clause 1 and clause 4."""
    sc = trace_scenes.make("aligned")[0]
    tris = trace_scenes.world_triangles(sc)
    rays = trace_scenes.ray_set("aligned", "interior")
    n = len(rays)
    miss = (np.full(n, -1, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32),
            np.zeros(n, np.int32))
    rep = trace_ref.check_closest(tris, rays, miss)
    assert len(rep.violations["skipped"]) > 0.9 * n
    assert len(trace_ref.check_any(tris, rays, np.zeros(n, bool)).violations["any_hit"]) > 0.9 * n


def test_reference_contract_on_known_answers():
    """One triangle, hand-made rays: a centre hit, a clear miss, a wrong t, a wrong backface."""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    rays = np.array([[0.25, 0.25, 1, 0, 0, -1, 0, 10], [2, 2, 1, 0, 0, -1, 0, 10]], np.float32)
    E = trace_ref.exact_hits(tri, rays)
    assert E["t"][0, 0] == 1.0 and E["u"][0, 0] == 0.25 and E["v"][0, 0] == 0.25 and E["m"][0, 0] == 0.25
    assert E["det"][0, 0] > 0 and E["m"][1, 0] < 0
    f, i = np.float32, np.int32
    good = (i([0, -1]), f([1, 0]), f([0.25, 0]), f([0.25, 0]), i([0, 0]))
    assert trace_ref.check_closest(tri, rays, good).ok()
    for bad, clause in (((i([-1, -1]), f([0, 0]), f([0, 0]), f([0, 0]), i([0, 0])), "skipped"),
                        ((i([0, 0]), f([1, 1]), f([0.25, 2]), f([0.25, 2]), i([0, 0])), "returned"),
                        ((i([0, -1]), f([1.001, 0]), f([0.25, 0]), f([0.25, 0]), i([0, 0])), "returned"),
                        ((i([0, -1]), f([1, 0]), f([0.25, 0]), f([0.25, 0]), i([1, 0])), "returned")):
        assert trace_ref.check_closest(tri, rays, bad).violations[clause]
    assert trace_ref.check_any(tri, rays, [True, False]).ok()
    assert trace_ref.check_any(tri, rays, [False, False]).violations["any_hit"]
    assert trace_ref.check_any(tri, rays, [True, True]).violations["any_miss"]
    # ties: of two bit-equal triangles only the lower index may come back
    two = np.concatenate([tri, tri])
    assert trace_ref.check_closest(two, rays, good).ok()
    dup = (i([1, -1]),) + good[1:]
    assert trace_ref.check_closest(two, rays, dup).violations["ties"]


def test_candidate_cull_agrees_with_the_exhaustive_pass():
    """Above trace_ref.CULL_ABOVE triangles the reference looks only at triangles whose bounding sphere a
    ray's line passes.  On a 34570-triangle scene: every triangle that float64 hits or nearly hits
    (m >= -bound) is among the candidates, and the culled check reports what the un-culled one does --
    on the oracle's answers, and on answers spoiled so that every clause has something to report."""
    from helpers import shared_edge_rays
    from optixpathtracer_amd import scenes
    from oracle.oracle import OracleScene

    sc = scenes.sphere_in_box("diffuse")
    tris = trace_scenes.world_triangles(sc)
    assert len(tris) > trace_ref.CULL_ABOVE
    rays = np.concatenate([shared_edge_rays(sc, 24, seed=5), shared_edge_rays(sc, 8, seed=6, far=True)])
    E = trace_ref.exact_hits(tris, rays)
    with np.errstate(all="ignore"):
        near = E["m"] >= -trace_ref.bound(E["cond_m"])
    ids = trace_ref._candidates(tris.astype(np.float64), rays)
    assert len(ids) < len(tris) // 4 and np.isin(np.nonzero(near.any(axis=0))[0], ids).all()
    o = OracleScene(sc)
    good = o.trace(rays)
    any_hit = o.trace(rays, any_hit=True)[0] >= 0
    o.close()
    spoiled = (np.where(np.arange(len(rays)) % 3 == 0, -1, good[0]).astype(np.int32),) + tuple(good[1:])
    for closest, anys in ((good, any_hit), (spoiled, ~any_hit)):
        a, b = trace_ref.check_closest(tris, rays, closest), trace_ref.check_closest(tris, rays, closest, cull=False)
        c, d = trace_ref.check_any(tris, rays, anys), trace_ref.check_any(tris, rays, anys, cull=False)
        for x, y in ((a, b), (c, d)):
            assert x.violations == y.violations and x.left_out == y.left_out and x.ratios == y.ratios
            assert x.passed_between == y.passed_between
    assert b.violations["skipped"] and d.violations["any_hit"]
