"""Geometrical simulations on the GPU (csrc/geometrical.hip): every case of tests/_geometrical_cases.py through
`KikuchiPatternSimulator.on_detector` against the reference's own classes (tests/golden/geometrical.npz), or the NumPy
restatement where a case has no fixture entry.  `in_pattern`, the kept reflectors and zone axes and the places of NaN
must be equal; coordinates agree within 1e-10 R_g (gnomonic) and that divided by the point's pixel scale (pixel): the
derivation is at `tolerances` of tests/_geometrical_cases.py.  Pairs next to a threshold are left out and counted (at
most 0.5 % of a case, none at one point: tests/test_host_geometrical.py); the hand-made z = 0 and z = -5e-6 reflectors
are exact and stay in.  Then the chunk switch (bit for bit), and the refusals of the C ABI."""

import ctypes as C

import numpy as np
import pytest

import _geometrical_cases as cases
import kikuchipy_amd as kpa
from conftest import load_golden
from kikuchipy_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = load_golden("geometrical.npz")
CASES = cases.cases()
BY_NAME = {c["name"]: c for c in CASES}
ARRAYS = ("keep", "uvw", "line_in", "zone_in", "line_gn", "line_px", "zone_gn", "zone_px")
_WANT = {}


def expected(case):
    """(the restatement, what to compare with: the fixture's arrays or the restatement's), computed once."""
    name = case["name"]
    if name not in _WANT:
        sim = cases.simulate(case)
        want = {k: GOLDEN[cases.key(case, k)] if case["golden"] else sim[k] for k in ARRAYS}
        for a in want.values():
            a.setflags(write=False)
        _WANT[name] = (sim, want)
    return _WANT[name]


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def run(ctx, case, monkeypatch, chunk=None):
    if chunk is None:
        monkeypatch.delenv("KPDI_GEOMETRICAL_CHUNK", raising=False)
    else:
        monkeypatch.setenv("KPDI_GEOMETRICAL_CHUNK", str(chunk))
    simulator = kpa.KikuchiPatternSimulator(kpa.Reflectors(case["hkl"], None, reciprocal_basis=case["basis"]))
    return simulator.on_detector(cases.detector(case), case["rotations"], context=ctx)


def flat(got):
    """The arrays of a simulation, navigation axes flattened, under the names of the restatement."""
    n = int(np.prod(got.navigation_shape))
    return {"uvw": got.zone_axes, "line_in": got.lines.in_pattern.reshape(n, -1),
            "zone_in": got.zone_axes_features.in_pattern.reshape(n, -1),
            "line_gn": got.lines.plane_trace_coordinates.reshape(n, -1, 4),
            "line_px": got._lines_detector_coordinates.reshape(n, -1, 4),
            "zone_gn": got._zone_axes._xy_within_r_gnomonic.reshape(n, -1, 2),
            "zone_px": got._zone_axes_detector_coordinates.reshape(n, -1, 2)}


def assert_equals_the_reference(got, case):
    sim, want = expected(case)
    nav = case["rotations"].shape[:-1]
    assert got.navigation_shape == nav and got.ndim == len(nav)
    assert np.array_equal(got.reflectors.hkl, case["hkl"][want["keep"]])
    arrays = flat(got)
    assert np.array_equal(arrays["uvw"], want["uvw"])
    lines_out, zones_out = cases.left_out(case, sim)
    left = int(lines_out.sum() + zones_out.sum())
    assert left <= cases.LEFT_OUT_CAP * (lines_out.size + zones_out.size) and (left == 0 or lines_out.shape[0] > 1)
    assert arrays["line_in"].dtype == np.bool_ and np.array_equal(arrays["line_in"][~lines_out], want["line_in"][~lines_out])
    assert np.array_equal(arrays["zone_in"][~zones_out], want["zone_in"][~zones_out])
    atol, tol_x, tol_y = cases.tolerances(sim)
    line_tol = np.stack([tol_x, tol_y, tol_x, tol_y], axis=-1)
    zone_tol = np.stack([tol_x, tol_y], axis=-1)
    for k, out, tol in (("line_gn", lines_out, atol), ("line_px", lines_out, line_tol), ("zone_gn", zones_out, atol),
                        ("zone_px", zones_out, zone_tol)):
        assert arrays[k].dtype == np.float64 and arrays[k].shape == want[k].shape, k
        ok, worst = cases.compare(arrays[k], want[k], out, tol)
        print(case["name"], k, want[k].shape, "left out:", int(out.sum()), "largest error / tolerance:", worst)
        assert ok, k


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_on_detector_equals_the_reference(ctx, monkeypatch, name):
    case = BY_NAME[name]
    assert_equals_the_reference(run(ctx, case, monkeypatch), case)


def test_handmade_reflectors_are_decided_exactly(ctx, monkeypatch):
    """z = 0 exactly and z = -5e-6 at the first point: not in the pattern, yet within the gnomonic radius, so drawn."""
    got = run(ctx, BY_NAME["handmade_z0"], monkeypatch)
    assert np.array_equal(got.reflectors.hkl[:2], [[0, 1, 0], [-1, 1, 0]])
    assert got.lines.in_pattern[0, :2].tolist() == [False, False]
    assert np.isfinite(got.lines_coordinates(0, exclude_nan=False)[:2]).all()
    assert got.lines.within_r_gnomonic[0, :2].all()


@pytest.mark.parametrize("chunk", [1, cases.FORCED_CHUNK, 64])
def test_same_result_for_every_chunk_length(ctx, monkeypatch, chunk):
    case = BY_NAME["points65_reflectors257"]
    own, forced = flat(run(ctx, case, monkeypatch)), flat(run(ctx, case, monkeypatch, chunk=chunk))
    for k in own:
        assert np.array_equal(own[k], forced[k], equal_nan=True), k  # every pair, the ones left out included


def test_on_a_context_of_its_own_and_with_a_rotation_object(ctx, monkeypatch):
    case = BY_NAME["map3x3_nine_pcs"]
    shared = flat(run(ctx, case, monkeypatch))

    class Rotations:
        data = case["rotations"]

    simulator = kpa.KikuchiPatternSimulator(kpa.Reflectors(case["hkl"], None))
    own = simulator.on_detector(cases.detector(case), Rotations(), device=0)
    for k, a in flat(own).items():
        assert np.array_equal(a, shared[k], equal_nan=True), k
    index = (2, 1)
    lines, zones = own.lines_coordinates(index), own.zone_axes_coordinates(index)
    assert lines.shape[1] == 4 and zones.shape[1] == 2 and not np.isnan(lines).any() and not np.isnan(zones).any()
    assert own.lines_coordinates(index, exclude_nan=False).shape == own.lines_coordinates((0, 0), exclude_nan=False).shape


def test_counters_report_both_passes(ctx, monkeypatch):
    ctx.set_profiling(1)
    try:
        run(ctx, BY_NAME["map3x3_one_pc"], monkeypatch)
        counters = ctx.counters()
    finally:
        ctx.set_profiling(0)
    assert counters["geometrical_visibility_ms"] > 0 and counters["geometrical_coordinates_ms"] > 0


def test_refused_calls_at_the_c_abi(ctx):
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hkl = np.array([[1.0, 1, 1], [2, 0, 0]])
    rot = cases.random_rotations(1, (3,))
    eye = np.eye(3)
    pcs = np.tile([-1.0, 1, -1, 1, 0.5, 0.5, 0.03, 0.03], (3, 1))
    flags = np.full(2, 7, dtype=np.uint8)
    vis = lib.kpdi_geometrical_visibility
    nulls = "vectors, rotations, u_s, basis, pcs or flags is NULL"
    refused = [
        ((None, p(hkl), 2, 0, p(rot), 3, p(eye), p(eye), p(pcs), 3, p(flags)), "ctx is NULL"),
        ((ctx._h, None, 2, 0, p(rot), 3, p(eye), p(eye), p(pcs), 3, p(flags)), nulls),
        ((ctx._h, p(hkl), 2, 0, None, 3, p(eye), p(eye), p(pcs), 3, p(flags)), nulls),
        ((ctx._h, p(hkl), 2, 0, p(rot), 3, None, p(eye), p(pcs), 3, p(flags)), nulls),
        ((ctx._h, p(hkl), 2, 0, p(rot), 3, p(eye), None, p(pcs), 3, p(flags)), nulls),
        ((ctx._h, p(hkl), 2, 0, p(rot), 3, p(eye), p(eye), None, 3, p(flags)), nulls),
        ((ctx._h, p(hkl), 2, 0, p(rot), 3, p(eye), p(eye), p(pcs), 3, None), nulls),
        ((ctx._h, p(hkl), 0, 0, p(rot), 3, p(eye), p(eye), p(pcs), 3, p(flags)), "0 features: at least one is needed"),
        ((ctx._h, p(hkl), 2, 0, p(rot), 0, p(eye), p(eye), p(pcs), 1, p(flags)), "0 map points: at least one is needed"),
        ((ctx._h, p(hkl), 2, 0, p(rot), 3, p(eye), p(eye), p(pcs), 2, p(flags)),
         "2 projection centres for 3 map points: one, or one per point"),
        ((ctx._h, p(hkl), 2, 2, p(rot), 3, p(eye), p(eye), p(pcs), 3, p(flags)), "kind 2: 0 (lines) or 1 (zone axes)"),
    ]
    for args, text in refused:
        assert vis(*args) == -1 and _lib.last_error() == text, (text, _lib.last_error())
    assert (flags == 7).all()  # nothing was written
    out = {"li": np.full((3, 2), 7, dtype=np.uint8), "lg": np.full((3, 2, 4), -1.0), "lp": np.full((3, 2, 4), -1.0),
           "zi": np.full((3, 1), 7, dtype=np.uint8), "zg": np.full((3, 1, 2), -1.0), "zp": np.full((3, 1, 2), -1.0)}
    uvw = np.array([[0.0, 1, -1]])
    outs = [p(out[k]) for k in ("li", "lg", "lp", "zi", "zg", "zp")]
    head = [ctx._h, p(hkl), 2, p(uvw), 1, p(rot), 3, p(eye), p(eye), p(eye), p(pcs), 3, 2.0]
    coord = lib.kpdi_geometrical_coordinates

    def call(**change):
        args = head + outs
        for i, v in change.items():
            args[int(i[1:])] = v
        return coord(*args)

    line_nulls = "hkl, rotations, u_s, a_star, a_direct, pcs or a line output is NULL"
    for change, text in (({"_0": None}, "ctx is NULL"), ({"_1": None}, line_nulls), ({"_5": None}, line_nulls),
                         ({"_7": None}, line_nulls), ({"_8": None}, line_nulls), ({"_9": None}, line_nulls),
                         ({"_10": None}, line_nulls), ({"_13": None}, line_nulls), ({"_14": None}, line_nulls),
                         ({"_15": None}, line_nulls), ({"_3": None}, "uvw or a zone axis output is NULL"),
                         ({"_17": None}, "uvw or a zone axis output is NULL"),
                         ({"_2": 0}, "0 lines: at least one is needed"), ({"_4": -1}, "-1 zone axes: none or more"),
                         ({"_6": 0}, "0 map points: at least one is needed"),
                         ({"_11": 2}, "2 projection centres for 3 map points: one, or one per point")):
        assert call(**change) == -1 and _lib.last_error() == text, (change, text, _lib.last_error())
    assert all((a == 7).all() if a.dtype == np.uint8 else (a == -1.0).all() for a in out.values())  # nothing was written
    with pytest.raises(_lib.KpdiError, match=r"\(n, 4\) and \(1 or n, 8\) expected"):
        ctx.geometrical_visibility(hkl, 0, rot[:, :3], eye, eye, pcs)
    # and the context still works: no zone axes at all is a valid call
    assert call(_3=None, _4=0, _16=None, _17=None, _18=None) == 0 and (out["li"] <= 1).all() and (out["zi"] == 7).all()
    assert vis(ctx._h, p(hkl), 2, 0, p(rot), 3, p(eye), p(eye), p(pcs), 3, p(flags)) == 0 and (flags <= 3).all()
