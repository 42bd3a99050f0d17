"""Neighbour pattern averaging and neighbour dot products on the GPU (csrc/neighbours.hip through
kpdi_average_neighbour_patterns / kpdi_neighbour_dot_products): against the reference's fixture
(tests/golden/neighbours.npz) through `EBSD`, the stack functions and the raw ABI; every pattern dtype and large
patterns against the restatement; members of a group sharing the GPU; a resident chain into dictionary indexing.

Bounds: integer-valued windows equal the fixture exactly.  For the Gaussian window no pixel may differ by more than
one grey level and the share of differing pixels is capped by what the restatement itself shows against the fixture
(`gauss__restate_share`, 0.0 when the fixture was made) plus 1e-3 of the pixels.  Dot products:
|ours - g64| <= 1e-5 s with identical NaN positions (tests/_neighbour_cases.py, `dot_scale`)."""

import json
import os

import numpy as np
import pytest

import _neighbour_cases as cases
import _neighbour_restate as R
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib
from kikuchipy_amd.filters import Window
from kikuchipy_amd.pattern import (average_neighbour_dot_product_map, average_neighbour_patterns_stack,
                                   neighbour_dot_product_matrices)
from kikuchipy_amd.pattern import _neighbours as N
from test_host_neighbours import FIX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("inp, win", [c for c in cases.AVERAGE_CASES if c[1] in cases.INTEGER_WINDOWS])
def test_averaging_equals_the_reference(inp, win):
    data = cases.inputs(inp)
    keep = data.copy()
    want = FIX[cases.avg_key(inp, win)]
    s = kpa.EBSD(data)
    s2 = s.average_neighbour_patterns(inplace=False, **cases.WINDOWS[win])
    assert s.data is data and np.array_equal(data, keep)  # untouched
    assert s2.data.dtype == want.dtype
    np.testing.assert_array_equal(s2.data, want)
    np.testing.assert_array_equal(average_neighbour_patterns_stack(data, FIX[f"win__{win}"]), want)
    assert s.average_neighbour_patterns(**cases.WINDOWS[win]) is None
    np.testing.assert_array_equal(s.data, want)
    s.close()


def test_gaussian_window_within_one_grey_level():
    report = {}
    for inp, win in [c for c in cases.AVERAGE_CASES if c[1] not in cases.INTEGER_WINDOWS]:
        data = cases.inputs(inp)
        want = FIX[cases.avg_key(inp, win)]
        got = average_neighbour_patterns_stack(data, **cases.WINDOWS[win])
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        share = float((d != 0).mean())
        report[cases.avg_key(inp, win)] = {"max_abs_diff": int(d.max()), "share_differing": share,
                                           "restatement_share": float(FIX["gauss__restate_share"])}
        print(cases.avg_key(inp, win), report[cases.avg_key(inp, win)])
        assert d.max() <= 1
        assert share <= float(FIX["gauss__restate_share"]) + 1e-3
    try:
        with open(os.path.join(ROOT, "profiles", "neighbours_parity.json"), "w") as f:
            json.dump(report, f, indent=1)
    except OSError:  # a read-only checkout: the figures are printed above
        pass


def _window(fpn):
    spec = cases.FOOTPRINTS[fpn]
    return None if spec is None else spec if isinstance(spec, np.ndarray) else Window(**spec)


def _check_dot(key, nm, mat, adp, dtype):
    m64, a64 = FIX[key + "__mat64"], FIX[key + "__adp64"]
    s_mat, s_map = cases.dot_scale(m64, nm)
    if mat is not None:
        assert mat.dtype == dtype and mat.shape == m64.shape
        np.testing.assert_array_equal(np.isnan(mat), np.isnan(m64), err_msg=key)
        ok = ~np.isnan(m64)
        err = np.abs(mat.astype(np.float64) - m64)[ok]
        print(key, "matrices: worst |d| / s", float(np.max(err / np.maximum(s_mat[ok], 1e-300))))
        assert np.all(err <= (cases.DOT_RTOL * s_mat)[ok]), key
    if adp is not None:
        assert adp.dtype == dtype and adp.shape == a64.shape
        np.testing.assert_array_equal(np.isnan(adp), np.isnan(a64), err_msg=key)
        ok = ~np.isnan(a64)
        err = np.abs(adp.astype(np.float64) - a64)[ok]
        print(key, "map: worst |d| / s", float(np.max(err / np.maximum(s_map[ok], 1e-300))))
        assert np.all(err <= (cases.DOT_RTOL * s_map)[ok]), key


@pytest.mark.parametrize("inp, fpn", cases.DOT_CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dot_products_meet_the_bound(inp, fpn, dtype):
    data = cases.inputs(inp)
    s = kpa.EBSD(data)
    for zm, nm in cases.FLAGS:
        key = cases.dot_key(inp, fpn, zm, nm)
        mat = s.get_neighbour_dot_product_matrices(_window(fpn), zm, nm, dtype)
        adp = s.get_average_neighbour_dot_product_map(_window(fpn), zm, nm, dtype)
        _check_dot(key, nm, mat, adp, dtype)
        # stack functions give the same bits; the map from the matrices agrees with the map from the kernel
        np.testing.assert_array_equal(neighbour_dot_product_matrices(data, _window(fpn), zm, nm, dtype), mat)
        np.testing.assert_array_equal(average_neighbour_dot_product_map(data, _window(fpn), zm, nm, dtype), adp)
        via = s.get_average_neighbour_dot_product_map(_window(fpn), dp_matrices=mat)
        _check_dot(key, nm, None, via.astype(dtype), dtype)
    s.close()


def test_raw_abi_one_launch_writes_both():
    data = cases.inputs("synthc")
    fp = FIX["fp__synthc__default"]
    with _lib.Context(0) as ctx:
        ctx.set_problem(*data.shape[-2:], None, _lib.METRIC_NCC, 1)
        ctx.set_experimental(data.reshape((-1,) + data.shape[-2:]))
        mat, adp = ctx.neighbour_dot_products(6, 7, fp, True, True, np.float64)
        _check_dot(cases.dot_key("synthc", "default", True, True), True, mat, adp, np.float64)
        m2, a2 = ctx.neighbour_dot_products(6, 7, fp, True, True, np.float64, row0=2, row1=5)
        np.testing.assert_array_equal(m2, mat[2:5])
        np.testing.assert_array_equal(a2, adp[2:5])
        np.testing.assert_array_equal(ctx.get_experimental().reshape(data.shape), data)  # only read
        for bad in (lambda: ctx.neighbour_dot_products(6, 6, fp), lambda: ctx.neighbour_dot_products(6, 7, fp, row0=3, row1=3),
                    lambda: ctx.neighbour_dot_products(6, 7, fp, row1=7), lambda: ctx.neighbour_dot_products(6, 7, fp * 0),
                    lambda: ctx.average_neighbour_patterns(6, 7, np.ones((3, 3)), np.zeros((6, 7))),
                    lambda: ctx.average_neighbour_patterns(7, 6, np.full((3, 3), np.nan), np.ones((7, 6)))):
            with pytest.raises(_lib.KpdiError):
                bad()
        w = N.window_on_map(FIX["win__circ55"], (6, 7))
        ctx.average_neighbour_patterns(6, 7, w, N.neighbour_window_sums(w, 6, 7))
        np.testing.assert_array_equal(ctx.get_experimental().reshape(data.shape), R.average(data, FIX["win__circ55"]))


@pytest.mark.parametrize("dtype", ["uint8", "int8", "uint16", "int16", "float32", "float64"])
def test_every_dtype_and_odd_shapes(dtype):
    """All six dtypes, a pattern size that is no multiple of 4 (the scalar path), patterns too large for the registers,
    a window larger than the map and negative coefficients, against the restatement (exact arithmetic: dyadic data)."""
    data = cases.synth(dtype, seed=3, nav=(4, 5), sig=(7, 9))
    for win in (FIX["win__circ55"], np.array([[1, -2, 0], [4, 1, 2]]), np.ones((9, 3))):
        np.testing.assert_array_equal(average_neighbour_patterns_stack(data, win), R.average(data, win))
    big = cases.synth(dtype, seed=4, nav=(2, 3), sig=(96, 80))
    np.testing.assert_array_equal(average_neighbour_patterns_stack(big, FIX["win__default"]),
                                  R.average(big, FIX["win__default"]))
    for p in (data, big):
        mat = neighbour_dot_product_matrices(p, dtype_out=np.float64)
        want = R.dot_matrices(p, FIX["win__default"] != 0)
        np.testing.assert_array_equal(np.isnan(mat), np.isnan(want))
        assert np.allclose(mat, want, rtol=0, atol=1e-9, equal_nan=True)


def test_nan_and_constant_patterns():
    data = cases.synth("float32", seed=5, nav=(3, 4), sig=(8, 8)).copy()
    data[1, 1, 2, 3] = np.nan
    data[2, 3] = 0.25
    mat = neighbour_dot_product_matrices(data, dtype_out=np.float64)
    assert np.isnan(mat[1, 1]).all() and np.isnan(mat[0, 1, 2, 1]) and np.isnan(mat[2, 3]).all()
    assert np.isnan(mat[2, 2, 1, 2]) and not np.isnan(mat[2, 2, 1, 0])
    adp = average_neighbour_dot_product_map(data)
    assert np.isnan(adp[1, 1]) and np.isnan(adp[2, 3]) and not np.isnan(adp[2, 2]) and not np.isnan(adp[0, 0])
    one = average_neighbour_dot_product_map(data[:1, :1])  # a 1 x 1 map: no neighbour at all
    assert one.shape == (1, 1) and np.isnan(one).all()
    const = np.full((2, 2, 4, 4), 9, dtype=np.uint8)
    assert not average_neighbour_patterns_stack(const).any()  # 0 / 0: 0 for integer dtypes, as rescale_intensity
    assert np.isnan(average_neighbour_patterns_stack(const.astype(np.float32))).all()


@pytest.mark.parametrize("n_ctx", [2, 8])
def test_members_sharing_the_gpu_equal_one_context(n_ctx):
    data = cases.synth("uint16", seed=6, nav=(11, 5), sig=(12, 12))
    data[4, 2] = 3
    one_avg = average_neighbour_patterns_stack(data, FIX["win__circ55"])
    one_g = average_neighbour_patterns_stack(data, FIX["win__gauss"])
    one_mat = neighbour_dot_product_matrices(data, Window("rectangular", (5, 3)))
    one_adp = average_neighbour_dot_product_map(data, dtype_out=np.float64)
    np.testing.assert_array_equal(one_avg, R.average(data, FIX["win__circ55"]))
    ctxs = [_lib.Context(0) for _ in range(n_ctx)]
    try:
        np.testing.assert_array_equal(average_neighbour_patterns_stack(data, FIX["win__circ55"], contexts=ctxs), one_avg)
        np.testing.assert_array_equal(average_neighbour_patterns_stack(data, FIX["win__gauss"], contexts=ctxs), one_g)
        np.testing.assert_array_equal(neighbour_dot_product_matrices(data, Window("rectangular", (5, 3)), contexts=ctxs),
                                      one_mat)
        np.testing.assert_array_equal(average_neighbour_dot_product_map(data, dtype_out=np.float64, contexts=ctxs), one_adp)
        few = average_neighbour_patterns_stack(data[:3], FIX["win__circ55"], contexts=ctxs)  # fewer rows than members
        np.testing.assert_array_equal(few, R.average(data[:3], FIX["win__circ55"]))
        line = average_neighbour_patterns_stack(data[:, 0], window_shape=(3,), contexts=ctxs)  # a 1-D map
        np.testing.assert_array_equal(line, R.average(data[:, 0], np.ones(3)))
    finally:
        for c in ctxs:
            c.close()


def test_resident_chain_into_dictionary_indexing():
    """set_experimental -> static background -> averaging -> dictionary indexing on the resident stack equals the same
    chain with the averaged patterns (the fixture's arithmetic, restated on the host) uploaded afresh."""
    shape = (24, 20)
    p = cases.synth("uint8")
    rng = np.random.default_rng(2)
    bg = rng.integers(0, 40, shape).astype(np.uint8)
    dic = rng.random((300,) + shape).astype(np.float32)
    w = N.window_on_map(FIX["win__default"], (6, 7))

    def tail(ctx):
        ctx.reset_topk()
        ctx.push_dictionary_chunk(dic, 0)
        return ctx.finalize(5)

    with _lib.Context(0) as ctx:
        ctx.set_problem(*shape, None, _lib.METRIC_NCC, 5)
        ctx.set_experimental(p.reshape((-1,) + shape))
        ctx.remove_static_background(bg.astype(np.float32), _lib.OP_SUBTRACT, False)
        ctx.average_neighbour_patterns(6, 7, w, N.neighbour_window_sums(w, 6, 7))
        resident = ctx.get_experimental()
        a = tail(ctx)
        corrected = kpa.pattern.remove_static_background(p, bg)
        host = R.average(corrected, FIX["win__default"])
        np.testing.assert_array_equal(resident.reshape(host.shape), host)
        ctx.set_experimental(host.reshape((-1,) + shape))
        b = tail(ctx)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # the fixture itself, from raw patterns
    np.testing.assert_array_equal(average_neighbour_patterns_stack(p, FIX["win__circ55"]),
                                  FIX[cases.avg_key("synth_uint8", "circ55")])


def test_one_by_one_window_changes_nothing():
    data = cases.inputs("dummy").copy()
    keep = data.copy()
    s = kpa.EBSD(data)
    with pytest.warns(UserWarning, match="A window of shape .* was passed, no averaging is therefore performed"):
        assert s.average_neighbour_patterns(window="rectangular", window_shape=(1, 1)) is None
    assert s.data is data and np.array_equal(data, keep)
    s3 = s.average_neighbour_patterns(inplace=False, lazy_output=True)
    assert isinstance(s3, kpa.EBSD) and np.array_equal(s3.data, FIX[cases.avg_key("dummy", "default")])
    s.close()
