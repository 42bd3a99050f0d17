"""Kinematical master patterns on the GPU (csrc/kinematical.hip): every case of tests/_kinematical_cases.py against the
reference's own `get_pattern` (tests/golden/kinematical.npz), or the NumPy restatement where a case has no fixture entry,
bit for bit in float64.  A pixel is left out only when some reflector's acos(D) lies within 1e-12 of a band edge or |D|
within 1e-12 of 1e-7 (the last bit of a device acos may differ); at most 1 % of a case's pixels may be, and with these
inputs none is (tests/test_host_kinematical.py).  Then `calculate_master_pattern` for every scaling and hemisphere, the
hemispheres of "both", every forced chunk length, the refusals of the C ABI, and the chain to `dictionary_indexing`."""

import ctypes as C

import numpy as np
import pytest

import _kinematical_cases as cases
import _kinematical_restate as restate
import kikuchipy_amd as kpa
from conftest import load_golden
from kikuchipy_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = load_golden("kinematical.npz")
CASES = cases.cases()
BY_NAME = {c["name"]: c for c in CASES + [cases.END_TO_END]}
_WANT = {}


def expected(case):
    """(pattern, pixels left out) of a case, computed once."""
    name = case["name"]
    if name not in _WANT:
        want = GOLDEN[cases.key(case)] if case["golden"] else restate.master_pattern(case)
        want.setflags(write=False)
        _WANT[name] = (want, restate.left_out(case))
    return _WANT[name]


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def run(ctx, case, monkeypatch, chunk="case"):
    chunk = case["chunk"] if chunk == "case" else chunk
    if chunk is None:
        monkeypatch.delenv("KPDI_KINEMATICAL_CHUNK", raising=False)
    else:
        monkeypatch.setenv("KPDI_KINEMATICAL_CHUNK", str(chunk))
    u, theta, f = cases.reflectors(case["reflectors"], case["m"])
    return ctx.kinematical_master_pattern(u, theta, cases.intensity(f, case["scaling"]), case["half_size"], case["hemisphere"])


def assert_equal_outside_thresholds(got, case):
    want, out = expected(case)
    assert got.dtype == np.float64 and got.shape == want.shape
    print(case["name"], "pixels left out:", int(out.sum()), "of", out.size, "differing:", int((got != want).sum()))
    assert out.mean() <= 0.01
    assert np.array_equal(got[~out], want[~out])


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_kernel_equals_the_reference_bit_for_bit(ctx, monkeypatch, name):
    case = BY_NAME[name]
    assert_equal_outside_thresholds(run(ctx, case, monkeypatch), case)


@pytest.mark.parametrize("chunk", cases.CHUNK_LENGTHS)
def test_same_result_for_every_chunk_length(ctx, monkeypatch, chunk):
    for name in ("ni_h8_both", "handmade_h20_both"):
        case = BY_NAME[name]
        got = run(ctx, case, monkeypatch, chunk=chunk)
        assert_equal_outside_thresholds(got, case)
        assert np.array_equal(got, run(ctx, case, monkeypatch, chunk=None))  # (every pixel, the ones left out included)


def test_both_is_upper_then_lower(ctx, monkeypatch):
    for hs in (8, 20):
        both = run(ctx, BY_NAME[f"ni_h{hs}_both"], monkeypatch)
        assert np.array_equal(both[0], run(ctx, BY_NAME[f"ni_h{hs}_upper"], monkeypatch))
        assert np.array_equal(both[1], run(ctx, BY_NAME[f"ni_h{hs}_lower"], monkeypatch))
        assert not np.array_equal(both[0], both[1])


def ni_simulator():
    hkl, theta, f = cases.ni_reflectors()
    return kpa.KikuchiPatternSimulator(kpa.Reflectors(hkl, theta, f, phase_name="ni"))


@pytest.mark.parametrize("scaling", ["linear", "square", None])
@pytest.mark.parametrize("hemisphere", ["upper", "lower", "both"])
def test_calculate_master_pattern(ctx, monkeypatch, scaling, hemisphere):
    monkeypatch.delenv("KPDI_KINEMATICAL_CHUNK", raising=False)
    case = dict(BY_NAME["ni_h8_both"], name=f"api_{hemisphere}_{scaling}", hemisphere=hemisphere, scaling=scaling, golden=False)
    stored = {("both", "linear"): "ni_h8_both", ("both", "square"): "ni_h8_both_square", ("both", None): "ni_h8_both_none",
              ("upper", "linear"): "ni_h8_upper", ("lower", "linear"): "ni_h8_lower"}.get((hemisphere, scaling))
    if stored:
        case = BY_NAME[stored]
    mp = ni_simulator().calculate_master_pattern(8, hemisphere, scaling, context=ctx)
    assert isinstance(mp, kpa.EBSDMasterPattern) and (mp.projection, mp.hemisphere, mp.phase_name) == ("stereographic", hemisphere, "ni")
    assert mp.has_inversion_symmetry is True
    assert_equal_outside_thresholds(mp.data, case)
    if hemisphere == "upper" and scaling == "linear":  # on a context of its own, by device number
        own = ni_simulator().calculate_master_pattern(8, device=0)
        assert np.array_equal(own.data, mp.data)


def test_refused_calls_at_the_c_abi(ctx):
    lib = _lib.load()
    u, theta, f = cases.reflectors("ni", 4)
    inten = abs(f)
    out = np.full((2, 3, 3), -1.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lib.kpdi_kinematical_master_pattern
    refused = [
        ((ctx._h, p(u), p(theta), p(inten), 0, 1, 0, p(out)), "0 reflectors: at least one is needed"),
        ((ctx._h, p(u), p(theta), p(inten), -3, 1, 0, p(out)), "-3 reflectors: at least one is needed"),
        ((ctx._h, p(u), p(theta), p(inten), 4, -1, 0, p(out)), "half_size -1: between 0 and 4096"),
        ((ctx._h, p(u), p(theta), p(inten), 4, 4097, 0, p(out)), "half_size 4097: between 0 and 4096"),
        ((ctx._h, p(u), p(theta), p(inten), 4, 1, 3, p(out)), "hemispheres 3: 0 (upper), 1 (lower) or 2 (both)"),
        ((ctx._h, p(u), p(theta), p(inten), 4, 1, -1, p(out)), "hemispheres -1: 0 (upper), 1 (lower) or 2 (both)"),
        ((ctx._h, None, p(theta), p(inten), 4, 1, 0, p(out)), "unit_vectors, theta, intensity or out is NULL"),
        ((ctx._h, p(u), None, p(inten), 4, 1, 0, p(out)), "unit_vectors, theta, intensity or out is NULL"),
        ((ctx._h, p(u), p(theta), None, 4, 1, 0, p(out)), "unit_vectors, theta, intensity or out is NULL"),
        ((ctx._h, p(u), p(theta), p(inten), 4, 1, 0, None), "unit_vectors, theta, intensity or out is NULL"),
        ((None, p(u), p(theta), p(inten), 4, 1, 0, p(out)), "ctx is NULL"),
    ]
    for args, text in refused:
        assert call(*args) == -1 and _lib.last_error() == text, (text, _lib.last_error())
    assert (out == -1.0).all()  # nothing was written
    with pytest.raises(_lib.KpdiError, match="half_size 5000: between 0 and 4096"):
        ctx.kinematical_master_pattern(u, theta, inten, 5000, "both")
    with pytest.raises(_lib.KpdiError, match=r"\(m, 3\), m and m expected"):
        ctx.kinematical_master_pattern(u, theta[:3], inten, 1, "both")
    # and the context still works
    assert call(ctx._h, p(u), p(theta), p(inten), 4, 1, 2, p(out)) == 0 and (out >= 0).all()


def test_end_to_end_master_pattern_to_dictionary_indexing(ctx, monkeypatch):
    """Ni, half_size 50, both hemispheres -> as_lambert() -> get_patterns for 64 rotations on a 24 x 24 detector; indexed
    against a dictionary of the same rotations every pattern finds itself."""
    monkeypatch.delenv("KPDI_KINEMATICAL_CHUNK", raising=False)
    mp = ni_simulator().calculate_master_pattern(50, "both", context=ctx)
    assert_equal_outside_thresholds(mp.data, cases.END_TO_END)
    det = kpa.EBSDDetector(shape=(24, 24), pc=(0.42, 0.6, 0.5))
    rng = np.random.default_rng(7)
    rot = rng.standard_normal((64, 4))
    rot /= np.linalg.norm(rot, axis=1)[:, None]
    with pytest.raises(NotImplementedError, match="Master pattern must be in the square Lambert projection"):
        mp.get_patterns(rot, det)
    lam = mp.as_lambert()
    want = GOLDEN["lambert__" + cases.END_TO_END["name"]]
    assert lam.data.dtype == np.float32 and np.all(np.abs(lam.data - want) <= np.spacing(np.abs(want)))
    patterns = lam.get_patterns(rot, det, compute=True)
    assert patterns.data.shape == (64, 24, 24) and patterns.data.dtype == np.float32 and np.isfinite(patterns.data).all()
    assert patterns.data.std(axis=(1, 2)).min() > 0
    dictionary = lam.get_patterns(rot, det)
    res = kpa.EBSD(np.array(patterns.data)).dictionary_indexing(dictionary, keep_n=1, verbose=False)
    print("scores", res.scores.min(), res.scores.max())
    assert np.array_equal(np.ravel(res.simulation_indices), np.arange(64))
    assert np.all(np.abs(np.ravel(res.scores) - 1) <= 1e-5)
