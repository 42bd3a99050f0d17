"""Disorientation angles, zone reduction and KAM maps on the GPU (csrc/orientations.hip) against the `np.longdouble`
restatement of tests/_orientation_cases.py, within the bound derived there: every rotation group and three mixed pairs;
sizes of 1, 2 and one below, at and above the outer kernel's tile sides and the workgroup size (read from
csrc/orientations_plan.h); forced row passes; float32 output; broadcasting; identical rows, exact equivalents, half turns,
NaN, infinite and zero rows (the pools' diagonal); the refusals of the C ABI."""

import ctypes as C

import numpy as np
import pytest

import _orientation_cases as cases
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib, sampling
from kikuchipy_amd.filters import Window

pytestmark = pytest.mark.gpu

U = cases.U
HC = cases.header_constants()
TI, TJ, WG = HC["ORI_TILE_I"], HC["ORI_TILE_J"], HC["ORI_THREADS"]
assert cases.POOL > max(TI, TJ)


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def inside(got, theta, slack, degrees=False):
    err, bound = cases.lost(got, theta, slack, degrees)
    print("largest share of the bound", (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0)
    return bool((err <= bound).all())


# ---- the outer kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g1,g2", cases.GROUP_PAIRS)
def test_outer_every_group(ctx, g1, g2):
    """34 x 34: two tile rows and two tile columns, the second of each with two rows / columns in use."""
    a, b = cases.pools(g1, g2)
    theta, slack = cases.outer_reference(g1, g2)
    got = kpa.disorientation_angle_outer(a, b, g1, g2, context=ctx)
    assert got.dtype == np.float64 and got.shape == theta.shape and inside(got, theta, slack)
    assert np.isnan(got[list(cases.INVALID_ROWS_A)]).all() and np.isnan(got[:, list(cases.INVALID_ROWS_B)]).all()
    assert np.isnan(got).sum() == cases.POOL * 3 - 2
    assert (np.diag(got)[:5] <= cases.angle_bound(np.diag(slack)[:5])).all()  # identical rows, -q, exact equivalents
    if g1 == "1" and g2 == "1":
        assert abs(got[11, 11] - np.pi) <= cases.angle_bound(0.0) and abs(got[12, 12] - np.pi) <= cases.angle_bound(0.0)  # half turns
    deg = kpa.disorientation_angle_outer(a, b, g1, g2, True, context=ctx)
    assert inside(deg, theta, slack, True)


SHAPES = sorted({(n, m) for n in (1, 2, TI - 1, TI, TI + 1) for m in (1, 2, TJ - 1, TJ, TJ + 1)}
                | {(WG - 1, 1), (WG, 2), (WG + 1, TJ + 1), (2, WG + 1)})


@pytest.mark.parametrize("n,m", SHAPES)
def test_outer_shapes(ctx, n, m):
    for g1, g2 in (("432", "432"), ("432", "622")):
        a, b = cases.pools(g1, g2)
        theta, slack = cases.outer_reference(g1, g2)
        i, j = np.arange(n) % cases.POOL, np.arange(m) % cases.POOL
        got = kpa.disorientation_angle_outer(a[i], b[j], g1, g2, context=ctx)
        assert got.shape == (n, m) and inside(got, theta[np.ix_(i, j)], slack[np.ix_(i, j)])


@pytest.mark.parametrize("rows", [1, 3])
def test_forced_passes_give_the_bits_of_one_pass(ctx, rows, monkeypatch):
    for (g1, g2), dtype in ((("432", "622"), "float64"), (("432", "432"), "float32")):
        a, b = cases.pools(g1, g2)
        i = np.arange(TI + 3) % cases.POOL
        monkeypatch.delenv("KPDI_ORIENT_PASS_ROWS", raising=False)
        one = kpa.disorientation_angle_outer(a[i], b, g1, g2, dtype_out=dtype, context=ctx)
        monkeypatch.setenv("KPDI_ORIENT_PASS_ROWS", str(rows))
        many = kpa.disorientation_angle_outer(a[i], b, g1, g2, dtype_out=dtype, context=ctx)
        assert one.dtype == np.dtype(dtype) and np.array_equal(one, many, equal_nan=True)
    monkeypatch.setenv("KPDI_ORIENT_PASS_ROWS", "0")
    with pytest.raises(_lib.KpdiError, match="KPDI_ORIENT_PASS_ROWS=0"):
        kpa.disorientation_angle_outer(a, b, "432", context=ctx)


def test_float32_output_is_the_rounded_float64_output(ctx):
    for g1, g2 in (("432", "432"), ("32", "1")):
        a, b = cases.pools(g1, g2)
        for degrees in (False, True):
            f64 = kpa.disorientation_angle_outer(a, b, g1, g2, degrees, context=ctx)
            f32 = kpa.disorientation_angle_outer(a, b, g1, g2, degrees, "float32", context=ctx)
            assert f32.dtype == np.float32 and np.array_equal(f32, f64.astype(np.float32), equal_nan=True)
    own = kpa.disorientation_angle_outer(a, None, "32", context=ctx)
    assert np.array_equal(own, kpa.disorientation_angle_outer(a, a, "32", context=ctx), equal_nan=True)


# ---- the pairs kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g1,g2", cases.GROUP_PAIRS)
def test_pairs_every_group(ctx, g1, g2):
    a, b = cases.pools(g1, g2)
    theta, slack = cases.outer_reference(g1, g2)
    for degrees in (False, True):
        got = kpa.disorientation_angle(a, b, g1, g2, degrees, context=ctx)
        assert got.shape == (cases.POOL,) and inside(got, np.diag(theta), np.diag(slack), degrees)
    assert np.isnan(got[[15, 16, 17]]).all() and np.isnan(got).sum() == 3


def test_pairs_broadcasting_and_sizes(ctx):
    a, b = cases.pools("432", "432")
    theta, slack = cases.outer_reference("432", "432")
    pick = lambda v: v[:15, :5].reshape(5, 3, 5)[np.arange(5), :, np.arange(5)]  # noqa: E731
    got = kpa.disorientation_angle(a[:15].reshape(5, 3, 4), b[:5].reshape(5, 1, 4), "m-3m", context=ctx)
    assert got.shape == (5, 3) and inside(got, pick(theta), pick(slack))
    # every row of A against every row of B as a broadcast pair call: (34, 1, 4) x (34, 4)
    got = kpa.disorientation_angle(a[:, None, :], b, "432", context=ctx)
    assert got.shape == theta.shape and inside(got, theta, slack)
    # one below, at and above the workgroup size, one row against many and a scalar pair
    i, j = np.divmod(np.arange(cases.POOL**2), cases.POOL)
    for count in (1, 2, WG - 1, WG, WG + 1):
        got = kpa.disorientation_angle(a[i[:count]], b[j[:count]], "432", context=ctx)
        assert got.shape == (count,) and inside(got, theta[i[:count], j[:count]], slack[i[:count], j[:count]])
    got = kpa.disorientation_angle(a[3], b[:20], "432", context=ctx)
    assert got.shape == (20,) and inside(got, theta[3, :20], slack[3, :20])
    got = kpa.disorientation_angle(a[3], b[4], "432", context=ctx)
    assert got.shape == () and inside(got, theta[3, 4], slack[3, 4])
    # a call with a device number opens and closes its own context
    assert np.array_equal(kpa.disorientation_angle(a[3], b[:20], "432", device=0), kpa.disorientation_angle(a[3], b[:20], "432", context=ctx),
                          equal_nan=True)


# ---- zone reduction ----------------------------------------------------------------------------------------------------------
def check_reduction(got, index, q, group):
    want, want_index, gap = cases.restate_reduce(q, group)
    bad = want_index < 0
    assert np.isnan(got[bad]).all() and (index[bad] == -1).all() and not np.isnan(got[~bad]).any()
    g, w, wi, gp = got[~bad], want[~bad], want_index[~bad], gap[~bad]
    assert sampling.in_fundamental_zone(g, sampling.fundamental_zone_faces(group)).all() and (g[:, 0] >= 0).all()
    zero, _ = cases.restate_pairs(g, q[~bad], group, group)  # equivalent to the input
    assert (zero.astype(np.float64) <= cases.angle_bound(0.0)).all()
    clear = gp > 2 * cases.EQUIV * U
    assert np.array_equal(index[~bad][clear], wi[clear])
    sign = np.where((np.abs(w[:, :1]) < 1e-15) & ((g * w).sum(axis=1, keepdims=True) < 0), -1, 1)
    assert (np.abs(g - (w * sign).astype(np.float64))[clear] <= cases.EQUIV * U + 1e-17).all()
    return int(clear.sum())


@pytest.mark.parametrize("group", cases.GROUPS)
def test_reduction_every_group(ctx, group):
    a, b = cases.pools(group, group)
    q = np.concatenate([a, b])
    got, index = kpa.reduce_to_fundamental_zone(q, group, True, context=ctx)
    assert got.shape == q.shape and got.dtype == np.float64 and index.dtype == np.int32 and index.shape == (2 * cases.POOL,)
    assert check_reduction(got, index, q, group) >= cases.POOL
    assert np.array_equal(kpa.reduce_to_fundamental_zone(q.reshape(2, -1, 4), group, context=ctx), got.reshape(2, -1, 4), equal_nan=True)


def test_reduction_sizes_and_zone_samples(ctx):
    a, b = cases.pools("622", "622")
    for n in (1, 2, WG - 1, WG, WG + 1):
        q = np.concatenate([a, b])[np.arange(n) % (2 * cases.POOL)]
        got, index = kpa.reduce_to_fundamental_zone(q, "6/mmm", True, context=ctx)
        check_reduction(got, index, q, "622")
    for group in ("432", "622", "32", "1"):
        q = kpa.get_sample_fundamental(point_group=group, semi_edge_steps=7)
        inner = q[:, 0] > sampling.FACE_SLACK
        for a0, a1, a2, t in sampling.fundamental_zone_faces(group):
            inner &= np.abs(q[:, 1] * a0 + q[:, 2] * a1 + q[:, 3] * a2) < t * q[:, 0] - sampling.FACE_SLACK
        got, index = kpa.reduce_to_fundamental_zone(q[inner], group, True, context=ctx)
        assert inner.sum() > 10 and (index == 0).all() and np.abs(got - q[inner]).max() <= 4 * U


# ---- KAM -----------------------------------------------------------------------------------------------------------------------
def test_kam_two_grains(ctx):
    """A 5 x 6 map, columns 0-2 one grain and 3-5 another 5 degrees away, every point a different symmetry equivalent of
    its grain, in another length and sign: interior points 0, the two columns at the boundary 5 / 4 degrees (5 / 3 in the
    first and last row), nothing with max_angle below 5 degrees, NaN at masked points."""
    rng = np.random.default_rng(5)
    ops = cases.ld_operations("432")[0].astype(np.float64)
    grain_a = cases.about([1, 2, 3], 0.7)
    grain_b = cases.f64_product(cases.about([-2, 1, 0.5], np.deg2rad(5.0)), grain_a)
    ny, nx = 5, 6
    q = np.array([cases.f64_product(ops[rng.integers(24)], grain_a if x < 3 else grain_b) * rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2)
                  for y in range(ny) for x in range(nx)])
    off = cases.window_offsets((np.asarray(Window("circular", (3, 3))) != 0))
    want, bound, _ = cases.restate_kam(q, ny, nx, "432", off)
    got = kpa.kernel_average_misorientation_map(q.reshape(ny, nx, 4), "m-3m", degrees=True, context=ctx)
    assert got.shape == (ny, nx)
    assert (np.abs(got.astype(cases.L) - want * (180 / cases.PI)).astype(np.float64) <= bound * (180 / np.pi) + 180 * U).all()
    tol = np.rad2deg(cases.angle_bound(0.0)) + 8 * U
    assert (got[:, [0, 1, 4, 5]] <= tol).all()
    assert (np.abs(got[1:-1, 2:4] - 5.0 / 4) <= tol + 5 * U * 4).all() and (np.abs(got[[0, -1], 2:4] - 5.0 / 3) <= tol + 5 * U * 4).all()
    limited = kpa.kernel_average_misorientation_map(q, "m-3m", (ny, nx), max_angle=2.0, degrees=True, context=ctx)
    assert (limited <= tol).all()
    assert np.array_equal(kpa.kernel_average_misorientation_map(q, "m-3m", (ny, nx), max_angle=6.0, degrees=True, context=ctx), got)
    mask = np.ones((ny, nx), dtype=bool)
    mask[2, 2] = mask[0, 5] = False
    masked = kpa.kernel_average_misorientation_map(q, "m-3m", (ny, nx), is_in_data=mask, context=ctx)
    want, bound, _ = cases.restate_kam(q, ny, nx, "432", off, mask)
    assert np.array_equal(np.isnan(masked), ~mask) and np.array_equal(np.isnan(want.astype(np.float64)), ~mask)
    assert (np.abs(masked[mask].astype(cases.L) - want[mask]).astype(np.float64) <= bound[mask]).all()
    assert masked[2, 3] <= cases.angle_bound(0.0)  # its only neighbour across the boundary is masked
    # no neighbour left: a lone point of the data
    alone = np.zeros((ny, nx), dtype=bool)
    alone[1, 1] = alone[3, 3] = True
    assert np.isnan(kpa.kernel_average_misorientation_map(q, "m-3m", (ny, nx), is_in_data=alone, context=ctx)).all()


KAM_WINDOWS = {"default": None, "circular5": Window("circular", (5, 5)), "rectangular3": Window("rectangular", (3, 3)),
               "rectangular35": Window("rectangular", (3, 5)), "gaussian": Window("gaussian", (3, 3), std=1),
               "even": Window("rectangular", (2, 4)), "custom": np.array([[1, 0, 1], [0, 1, 0], [0, 1, 1]], dtype=bool)}
KAM_MAPS = ((1, 1), (1, 5), (3, 3), (4, 7))


@pytest.mark.parametrize("name", sorted(KAM_WINDOWS))
@pytest.mark.parametrize("nav", KAM_MAPS)
def test_kam_windows(ctx, name, nav):
    a, b = cases.pools("622", "622")
    q = np.concatenate([a[:14], b[:14]])[:nav[0] * nav[1]]
    w = np.asarray(Window("circular", (3, 3)) if KAM_WINDOWS[name] is None else KAM_WINDOWS[name]) != 0
    want, bound, _ = cases.restate_kam(q, nav[0], nav[1], "622", cases.window_offsets(w))
    got = kpa.kernel_average_misorientation_map(q, "6/mmm", nav, KAM_WINDOWS[name], context=ctx)
    assert got.shape == nav and np.array_equal(np.isnan(got), np.isnan(want.astype(np.float64)))
    ok = ~np.isnan(got)
    assert (np.abs(got[ok].astype(cases.L) - want[ok]).astype(np.float64) <= bound[ok]).all()
    assert nav != (1, 1) or np.isnan(got).all()  # a lone point has no neighbours


def test_kam_one_axis_and_many_points(ctx):
    a, b = cases.pools("432", "432")
    q = np.concatenate([a[:14], b[:14]])[np.arange(WG + 1) % 28]
    want, bound, _ = cases.restate_kam(q, WG + 1, 1, "432", [(-1, 0), (1, 0)])
    got = kpa.kernel_average_misorientation_map(q, "432", context=ctx)
    assert got.shape == (WG + 1,) and (np.abs(got.astype(cases.L) - want[:, 0]).astype(np.float64) <= bound[:, 0]).all()
    limit = 0.6
    want, bound, ambiguous = cases.restate_kam(q, WG + 1, 1, "432", [(-1, 0), (1, 0)], None, limit)
    got = kpa.kernel_average_misorientation_map(q, "432", max_angle=limit, context=ctx)
    assert not ambiguous and np.array_equal(np.isnan(got), np.isnan(want[:, 0].astype(np.float64))) and np.isnan(got).any()
    ok = ~np.isnan(got)
    assert (np.abs(got[ok].astype(cases.L) - want[ok, 0]).astype(np.float64) <= bound[ok, 0]).all()


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_context_usable(ctx):
    lib = _lib.load()
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    a, b = (np.ascontiguousarray(v) for v in cases.pools("432", "432"))
    ops = np.ascontiguousarray(sampling.rotation_group_operations("432"))
    one = np.ascontiguousarray(sampling.rotation_group_operations("1"))
    out = np.full((cases.POOL, cases.POOL), -1.0)
    index = np.full(cases.POOL, -7, dtype=np.int32)
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    shape, st1, st0 = i64(cases.POOL), i64(1), i64(0)
    off = np.array([[0, 1]], dtype=np.int32)
    n = cases.POOL
    pairs, outer, reduce_, kam = lib.kpdi_orientation_pairs, lib.kpdi_orientation_outer, lib.kpdi_orientation_reduce, lib.kpdi_orientation_kam
    refused = [
        (pairs, (None, p(a), n, p(b), n, 1, p(shape), p(st1), p(st1), p(one), 1, p(ops), 24, 0, p(out)), "ctx is NULL"),
        (pairs, (ctx._h, None, n, p(b), n, 1, p(shape), p(st1), p(st1), p(one), 1, p(ops), 24, 0, p(out)), "q1, q2 or out is NULL"),
        (pairs, (ctx._h, p(a), 0, p(b), n, 1, p(shape), p(st1), p(st1), p(one), 1, p(ops), 24, 0, p(out)), "at least one each"),
        (pairs, (ctx._h, p(a), n, p(b), n, 9, p(shape), p(st1), p(st1), p(one), 1, p(ops), 24, 0, p(out)), "9 leading axes: between 0 and 8"),
        (pairs, (ctx._h, p(a), n, p(b), n, 1, None, p(st1), p(st1), p(one), 1, p(ops), 24, 0, p(out)), "shape, stride1 or stride2 is NULL"),
        (pairs, (ctx._h, p(a), n, p(b), n - 1, 1, p(shape), p(st1), p(st1), p(one), 1, p(ops), 24, 0, p(out)), "leaves an input"),
        (pairs, (ctx._h, p(a), n, p(b), n, 1, p(i64(0)), p(st1), p(st1), p(one), 1, p(ops), 24, 0, p(out)), "axis 0: length 0"),
        (pairs, (ctx._h, p(a), n, p(b), n, 1, p(shape), p(i64(-1)), p(st1), p(one), 1, p(ops), 24, 0, p(out)), "axis 0: length"),
        (pairs, (ctx._h, p(a), n, p(b), n, 1, p(shape), p(st1), p(st0), p(one), 0, p(ops), 24, 0, p(out)), "0 operations in ops1: between 1 and 24"),
        (pairs, (ctx._h, p(a), n, p(b), n, 1, p(shape), p(st1), p(st0), p(one), 1, p(ops), 25, 0, p(out)), "25 operations in ops2"),
        (pairs, (ctx._h, p(a), n, p(b), n, 1, p(shape), p(st1), p(st0), p(one), 1, None, 24, 0, p(out)), "ops2 is NULL"),
        (outer, (ctx._h, p(a), n, p(b), 0, p(one), 1, p(ops), 24, 0, 3, p(out)), "at least one each"),
        (outer, (ctx._h, p(a), n, p(b), n, p(one), 1, p(ops), 24, 0, 0, p(out)), "dtype_out 0: the angles are float64 or float32"),
        (outer, (ctx._h, p(a), n, p(b), n, p(one), 1, p(ops), 24, 0, 8, p(out)), "dtype_out 8"),
        (outer, (ctx._h, p(a), n, p(b), n, p(one), 1, p(ops), 24, 0, 3, None), "q1, q2 or out is NULL"),
        (outer, (ctx._h, p(a), n, p(b), n, p(one), 30, p(ops), 24, 0, 3, p(out)), "30 operations in ops1"),
        (reduce_, (ctx._h, p(a), 0, p(ops), 24, p(out), p(index)), "0 orientations"),
        (reduce_, (ctx._h, p(a), n, p(ops), 24, p(out), None), "q, out or index is NULL"),
        (reduce_, (ctx._h, p(a), n, p(ops), 0, p(out), p(index)), "0 operations in ops"),
        (kam, (ctx._h, p(a), 0, n, p(ops), 24, p(off), 1, None, -1.0, 0, p(out)), "a map of 0 x 34 points"),
        (kam, (ctx._h, p(a), 1, n, p(ops), 24, p(off), 1025, None, -1.0, 0, p(out)), "1025 window offsets"),
        (kam, (ctx._h, p(a), 1, n, p(ops), 24, None, 1, None, -1.0, 0, p(out)), "1 window offsets"),
        (kam, (ctx._h, p(a), 1, n, p(ops), 24, p(off), 1, None, float("nan"), 0, p(out)), "max_angle is NaN"),
        (kam, (ctx._h, None, 1, n, p(ops), 24, p(off), 1, None, -1.0, 0, p(out)), "q or out is NULL"),
    ]
    for fn, args, message in refused:
        assert fn(*args) == -1 and message in _lib.last_error(), (message, _lib.last_error())
    assert (out == -1.0).all() and (index == -7).all()  # nothing was written
    with pytest.raises(ValueError, match="at most 8"):
        kpa.disorientation_angle(a.reshape((1,) * 8 + (n, 4)), b.reshape((1,) * 8 + (n, 4)), context=ctx)
    with pytest.raises(_lib.KpdiError, match="rotations for a map"):
        ctx.orientation_kam(a, 5, 5, ops, off)
    # the context still computes
    theta, slack = cases.outer_reference("432", "432")
    assert inside(kpa.disorientation_angle_outer(a, b, "432", context=ctx), theta, slack)
    # an empty window (the origin alone) has no neighbours: NaN everywhere; profiling fills the counter
    assert np.isnan(ctx.orientation_kam(a[:6], 2, 3, ops, np.zeros((0, 2), dtype=np.int32))).all()
    ctx.set_profiling(True)
    try:
        kpa.disorientation_angle_outer(a, b, "432", context=ctx)
        assert ctx.counters()["orientation_ms"] > 0
    finally:
        ctx.set_profiling(False)
