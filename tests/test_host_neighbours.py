"""Neighbour pattern averaging and neighbour dot products, host side (no GPU): the NumPy restatement
(tests/_neighbour_restate.py) against the reference's fixture (tests/golden/neighbours.npz, made by
tools/gen_neighbour_golden.py), the signatures of the three `EBSD` methods, every error and warning raised before any
context is created, the host-only `dp_matrices=` path, and the row / halo split over several contexts."""

import inspect
import os
import warnings

import numpy as np
import pytest

import _neighbour_cases as cases
import _neighbour_restate as R
import kikuchipy_amd as kpa
from kikuchipy_amd.filters import Window
from kikuchipy_amd.pattern import _neighbours as N

FIX = np.load(os.path.join(cases.GOLDEN, "neighbours.npz"))


def our_window(name):
    spec = dict(cases.WINDOWS[name])
    return N.averaging_window(spec.pop("window"), spec.pop("window_shape", (3, 3)), **spec)


@pytest.mark.parametrize("name", sorted(cases.WINDOWS))
def test_windows_are_the_references(name):
    np.testing.assert_array_equal(np.asarray(our_window(name), dtype=np.float64), FIX[f"win__{name}"])


@pytest.mark.parametrize("inp, win", cases.AVERAGE_CASES)
def test_restatement_equals_the_fixture(inp, win):
    data = cases.inputs(inp)
    want = FIX[cases.avg_key(inp, win)]
    got = R.average(data, FIX[f"win__{win}"])
    assert got.dtype == want.dtype == data.dtype
    if win in cases.INTEGER_WINDOWS:
        np.testing.assert_array_equal(got, want)
    else:
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        assert d.max() <= 1 and (d != 0).mean() <= float(FIX["gauss__restate_share"])
    # the window sums: the restatement, the package's and SciPy's (the fixture) agree
    p, w = R.as_map(data, FIX[f"win__{win}"])
    sums = FIX[cases.avg_key(inp, win) + "__window_sums"].reshape(p.shape[:2])
    np.testing.assert_array_equal(R.window_sums(w, *p.shape[:2]), sums)
    np.testing.assert_array_equal(N.neighbour_window_sums(N.window_on_map(FIX[f"win__{win}"], data.shape[:-2]),
                                                          *p.shape[:2]), sums)


def test_window_sums_truncate():
    w = N.window_on_map(FIX["win__gauss"], (3, 3))
    np.testing.assert_array_equal(N.neighbour_window_sums(w, 3, 3), [[3, 5, 3], [5, 7, 5], [3, 5, 3]])


def test_known_answers_of_the_reference():
    """The reference's hard-coded answers come from its fastmath build: within one grey level / 1e-5."""
    n = 0
    for key in FIX.files:
        if key.startswith("known__avg__"):
            d = np.abs(FIX[key].astype(int) - FIX[key[len("known__"):]].astype(int))
            assert d.max() <= 1, key
            n += 1
        elif key.startswith("known__dp__"):
            a32 = FIX[key[len("known__"):] + "__adp32"]
            tol = 1e-5 if key.endswith("nm1") else 1e-5 * np.abs(a32).max()
            assert np.allclose(a32, FIX[key], atol=tol), key
            n += 1
    assert n == 10


@pytest.mark.parametrize("inp, fpn", cases.DOT_CASES)
@pytest.mark.parametrize("zm, nm", cases.FLAGS)
def test_dot_restatement_meets_the_bound(inp, fpn, zm, nm):
    key = cases.dot_key(inp, fpn, zm, nm)
    m64, a64 = FIX[key + "__mat64"], FIX[key + "__adp64"]
    data = cases.inputs(inp)
    got = R.dot_matrices(data, FIX[f"fp__{inp}__{fpn}"], zm, nm)
    s_mat, s_map = cases.dot_scale(m64, nm)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(m64))
    assert np.all(np.abs(got - m64)[~np.isnan(m64)] <= (cases.DOT_RTOL * s_mat)[~np.isnan(m64)])
    adp = R.adp_from_matrices(got, data.ndim - 2)
    np.testing.assert_array_equal(np.isnan(adp), np.isnan(a64))
    assert np.all(np.abs(adp - a64)[~np.isnan(a64)] <= (cases.DOT_RTOL * s_map)[~np.isnan(a64)])


# ---- the public interface
SIGNATURES = {
    "average_neighbour_patterns": (
        ["window", "window_shape", "show_progressbar", "inplace", "lazy_output"], ["circular", (3, 3), None, True, None]),
    "get_neighbour_dot_product_matrices": (
        ["window", "zero_mean", "normalize", "dtype_out", "show_progressbar"], [None, True, True, "float32", None]),
    "get_average_neighbour_dot_product_map": (
        ["window", "zero_mean", "normalize", "dtype_out", "dp_matrices", "show_progressbar"],
        [None, True, True, "float32", None, None]),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures_bind_like_the_reference(name):
    positional, defaults = SIGNATURES[name]
    params = list(inspect.signature(getattr(kpa.EBSD, name)).parameters.values())[1:]
    pos = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in pos] == positional and [p.default for p in pos] == defaults
    extra = [p for p in params if p.kind == p.KEYWORD_ONLY]
    assert [p.name for p in extra] == ["devices"] and extra[0].default is None
    assert any(p.kind == p.VAR_KEYWORD for p in params) == (name == "average_neighbour_patterns")


def _signal(nav=(3, 3)):
    s = kpa.EBSD(np.arange(int(np.prod(nav)) * 12, dtype=np.uint8).reshape(nav + (3, 4)), device=0)
    return s


def test_errors_and_warnings_come_before_any_context():
    s = _signal()
    keep = s.data.copy()
    with pytest.raises(ValueError, match="'lazy_output=True' requires 'inplace=False'"):
        s.average_neighbour_patterns(lazy_output=True)
    for shape in [(1,), (1, 1)]:
        with pytest.warns(UserWarning, match=r"A window of shape .* was passed, no averaging is therefore performed"):
            assert s.average_neighbour_patterns("rectangular", shape) is None
    with pytest.warns(UserWarning, match="no averaging"):
        assert s.average_neighbour_patterns(Window("rectangular", (1, 1)), inplace=False) is None
    with pytest.raises(ValueError, match="more axes than the map"):
        s.average_neighbour_patterns(np.ones((2, 2, 2)))
    with pytest.raises(ValueError, match="more axes than the map"):
        _signal((4,)).average_neighbour_patterns(window_shape=(3, 3))
    with pytest.raises(ValueError, match="window sum"):
        s.average_neighbour_patterns(np.array([[1.0, -1.0, 0.0]]))
    for method in (s.get_neighbour_dot_product_matrices, s.get_average_neighbour_dot_product_map):
        with pytest.raises(ValueError, match="origin"):
            method(window=np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]]))
        with pytest.raises(ValueError, match="dtype_out"):
            method(dtype_out="int32")
        with pytest.raises(ValueError, match="axes of the map"):
            method(window=Window("rectangular", (3,)))
    s0 = kpa.EBSD(np.zeros((3, 4), dtype=np.uint8), device=0)
    for method in (s0.get_neighbour_dot_product_matrices, s0.get_average_neighbour_dot_product_map):
        with pytest.raises(ValueError, match="Signal must have at least one navigation dimension"):
            method()
    assert s._ctx is None and s0._ctx is None and np.array_equal(s.data, keep)


def test_window_on_map():
    assert N.window_on_map(Window("rectangular", (3,)), (4, 5)).shape == (3, 1)  # along the first navigation axis
    assert N.window_on_map(Window("rectangular", (3,)), (4,)).shape == (3, 1)
    assert N.window_on_map(Window("circular", (5, 5)), (2, 2)).shape == (5, 5)  # larger than the map is legal
    w = Window("gaussian", (3, 3), std=2)
    assert N.averaging_window(w) is not w and np.array_equal(N.averaging_window(w), w)
    assert N.dot_product_window(None, (4,)).shape == (3,) and N.dot_product_window(None, (4, 4)).shape == (3, 3)
    assert not N.dot_product_window(None, (4, 4))[0, 0]  # circular


@pytest.mark.parametrize("inp, fpn", cases.DOT_CASES)
def test_dp_matrices_path_is_host_only(inp, fpn):
    data = cases.inputs(inp)
    s = kpa.EBSD(data, device=0)
    spec = cases.FOOTPRINTS[fpn]
    window = None if spec is None else spec if isinstance(spec, np.ndarray) else Window(**spec)
    for zm, nm in cases.FLAGS:
        key = cases.dot_key(inp, fpn, zm, nm)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            adp = s.get_average_neighbour_dot_product_map(window=window, dp_matrices=FIX[key + "__mat64"])
        a64 = FIX[key + "__adp64"]
        _, s_map = cases.dot_scale(FIX[key + "__mat64"], nm)
        np.testing.assert_array_equal(np.isnan(adp), np.isnan(a64))
        assert np.all(np.abs(adp - a64)[~np.isnan(a64)] <= 1e-12 * np.maximum(s_map, 1)[~np.isnan(a64)])
    assert s._ctx is None


@pytest.mark.parametrize("ny, wy, n", [(7, 5, 3), (512, 3, 8), (3, 3, 8), (2, 4, 2), (10, 1, 4), (5, 9, 2), (1, 3, 4)])
def test_row_blocks_cover_the_map_once(ny, wy, n):
    blocks = N.neighbour_row_blocks(ny, wy, n)
    assert len(blocks) == min(n, ny)
    assert [b[0] for b in blocks] == [0] + [b[1] for b in blocks[:-1]] and blocks[-1][1] == ny  # once, in order
    for r0, r1, lo, hi in blocks:
        assert r0 < r1
        assert lo == max(r0 - wy // 2, 0) and hi == min(r1 + (wy - wy // 2 - 1), ny)  # the halo, clipped


def test_blocks_take_the_window_sums_of_the_whole_map():
    """What a member is handed: its rows of the WHOLE map's sums - not the sums of its block, which differ at the
    block's border."""
    w = N.window_on_map(Window("rectangular", (3, 3)), (6, 4))
    whole = N.neighbour_window_sums(w, 6, 4)
    for r0, r1, lo, hi in N.neighbour_row_blocks(6, 3, 3):
        own = whole[lo:hi]
        assert own.shape == (hi - lo, 4)
        if lo > 0:
            assert not np.array_equal(own, N.neighbour_window_sums(w, hi - lo, 4))
    assert whole[2, 1] == 9 and whole[0, 0] == 4
