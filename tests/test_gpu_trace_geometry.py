"""The kernels' traced hits against float64 geometry, and the product kernels on the same scenes.

Two statements per (builder, variant), on every ray set of tests/trace_scenes.py:
  A. pt_trace_rays (k_trace), closest and any-hit, meets the float64 contract of tests/trace_ref.py.
     The triangles are the device's own records (bvh_arrays: v0, e1, e2) and the verdict uses no
     oracle code.
  B. The same answers equal the oracle's bit for bit.
A failure says which of the two broke.

The product kernels (k_trace_pair, k_extend, k_shadow_vis, with the lit, occluder and skip tables)
have no ray interface; they are held to bit-identical images: the wavefront as shipped, the wavefront
with all three tables off, the megakernel and the oracle, on every variant, in Lambert and Layered
modes, on one and two streams.  The comparison with the tables means something only where a table is
in use, and the test asserts where that is.  `far`, `huge` and `model` have a vertex beyond kLitMaxCoord =
128, so the library builds none of the three tables there and "as shipped" equals "tables off" by
construction: those variants test the trace kernels, the megakernel and the oracle against each other,
not the tables.  On the six in-bounds variants the occluder table is built, and the skip table in
Lambert mode (Layered never carries it); the lit table answers NEE tests on all of them but `tiny`,
whose 3e-3 box is smaller than the table's absolute 2e-3 margin, so no cell is ever proven lit (the
margin costs the table there, it does not break it); the occluder table answers on all but `slivers`.
`huge` is thin for the path kernels too: path rays end at t = 100, so only the ceiling next to the
camera is ever hit (a third of the pixels, asserted).
"""
import numpy as np
import pytest

import trace_ref
import trace_scenes

pytestmark = pytest.mark.gpu

BUILDERS = {"ploc": 3, "lbvh": 1, "sah": 2, "sah_gpu": 4}
TRACE_CASES = [(v, b) for v in trace_scenes.VARIANTS for b in BUILDERS]
W, H, DEPTH, FIRST, FRAMES = 48, 32, 4, 0, 2
MODES = {"lambert": 1, "layered": 4}
IN_BOUNDS = ("unit", "tiny", "slivers", "aligned", "coplanar", "degenerate")  # every coordinate within kLitMaxCoord
LIT_ANSWERS = tuple(v for v in IN_BOUNDS if v != "tiny")
OCCLUDER_ANSWERS = tuple(v for v in IN_BOUNDS if v != "slivers")
_oracle_answers = {}
_reference_images = {}


def _all_rays(variant):
    return np.concatenate([trace_scenes.ray_set(variant, k) for k in trace_scenes.RAY_SETS])


def _oracle_trace(variant, rays):
    if variant not in _oracle_answers:
        from oracle.oracle import OracleScene

        o = OracleScene(trace_scenes.make(variant)[0])
        _oracle_answers[variant] = (o.trace(rays), o.trace(rays, any_hit=True)[0] >= 0)
        o.close()
    return _oracle_answers[variant]


@pytest.mark.parametrize("variant,builder", TRACE_CASES, ids=[f"{v}-{b}" for v, b in TRACE_CASES])
def test_traced_rays_meet_float64_contract_and_equal_oracle(variant, builder):
    from optixpathtracer_amd.renderer import setup_renderer

    sc = trace_scenes.make(variant)[0]
    rays = _all_rays(variant)
    r = setup_renderer(sc, 32, 32, 2, bvh_builder=BUILDERS[builder])
    tris = trace_scenes.record_triangles(r.bvh_arrays()[1])
    closest = r.trace_rays(rays)
    any_hit = r.trace_rays(rays, any_hit=True)[0] >= 0
    r.close()
    assert len(tris) == sc.n_triangles <= 2000

    broke = []
    at = 0
    for kind in trace_scenes.RAY_SETS:  # A: float64 geometry, no oracle; clauses and cap per ray set
        sl = slice(at, at + len(trace_scenes.ray_set(variant, kind)))
        at = sl.stop
        try:
            trace_ref.assert_contract(tris, rays[sl], tuple(x[sl] for x in closest), any_hit[sl],
                                      f"gpu {variant}/{kind}/{builder}")
        except AssertionError as e:
            broke.append(f"A (GPU against float64 geometry): {e}")
    assert at == len(rays)
    try:  # B: the oracle, bit for bit
        (op, ot, ou, ov, ob), oa = _oracle_trace(variant, rays)
        gp, gt, gu, gv, gb = closest
        np.testing.assert_array_equal(gp, op)
        hit = op >= 0
        for g, o_ in ((gt, ot), (gu, ou), (gv, ov), (gb, ob)):
            np.testing.assert_array_equal(g[hit], o_[hit])
        np.testing.assert_array_equal(any_hit, oa)
    except AssertionError as e:
        broke.append(f"B (GPU == oracle bit for bit): {e}")
    assert not broke, "\n".join(broke)


def _render(sc, mode, kernel, streams=None, tables=None):
    from optixpathtracer_amd.renderer import setup_renderer

    r = setup_renderer(sc, W, H, DEPTH, kernel=kernel)
    r.set_material_mode(mode)
    if streams is not None:
        r.set_wavefront_streams(streams)
    if tables is not None:
        r.set_lit_table(tables)
        r.set_occluder_table(tables)
        r.set_skip_table(tables)
    r.accum_clear()
    r.render_frames(FIRST, FRAMES)
    img = r.accum().copy()
    st = r.stats()
    used = dict(lit=st["lit_table_answers"], occluder=st["occluder_table_answers"],
                occluder_table=r.occluder_table() is not None, skip_table=r.skip_table() is not None)
    r.close()
    return img, used


def _references(variant, mode):
    """(oracle image, megakernel image), once per (variant, mode)."""
    if (variant, mode) not in _reference_images:
        from helpers import oracle_render

        sc = trace_scenes.make(variant)[0]
        ref, _ = oracle_render(sc, W, H, DEPTH, FIRST, FRAMES, mode=MODES[mode])
        _reference_images[(variant, mode)] = (ref, _render(sc, MODES[mode], kernel=0)[0])
    return _reference_images[(variant, mode)]


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("variant", trace_scenes.VARIANTS)
def test_product_kernels_bit_identical(variant, mode, streams):
    sc = trace_scenes.make(variant)[0]
    ref, mega = _references(variant, mode)
    shipped, used = _render(sc, MODES[mode], kernel=1, streams=streams)
    plain, unused = _render(sc, MODES[mode], kernel=1, streams=streams, tables=False)
    lit_pixels = (ref > 0).any(axis=2).mean()
    print(f"tables {variant}/{mode}/{streams}: shipped {used} off {unused} lit pixels {lit_pixels:.3f}")
    assert np.isfinite(ref).all() and lit_pixels > 0.3, "the scene renders (nearly) black: the test would be empty"
    # which tables the shipped run really used (module docstring); with them off, none
    assert unused == dict(lit=0, occluder=0, occluder_table=False, skip_table=False)
    assert used["occluder_table"] == (variant in IN_BOUNDS)
    assert used["skip_table"] == (variant in IN_BOUNDS and mode == "lambert")
    assert (used["lit"] > 0) == (variant in LIT_ANSWERS)
    assert (used["occluder"] > 0) == (variant in OCCLUDER_ANSWERS)
    np.testing.assert_array_equal(shipped, plain, err_msg="wavefront: tables as shipped vs all three tables off")
    np.testing.assert_array_equal(plain, mega, err_msg="wavefront (tables off) vs megakernel")
    np.testing.assert_array_equal(mega, ref, err_msg="megakernel vs oracle")
