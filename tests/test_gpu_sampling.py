"""Orientation sampling on the GPU (csrc/sampling.hip): for every rotation group the kernel keeps the grid points the
host sampler keeps, in its order; every quaternion component against the `np.longdouble` restatement of
tests/_sampling_cases.py within 4 floor + 8 ulp; the refusals of the C ABI; a hexagonal phase end to end (kinematical
master pattern -> dictionary of the 6/mmm zone -> symmetry-equivalent orientations index as their dictionary entry); and
the cubic dictionary of the reference's benchmark sampled on the device."""

import ctypes as C

import numpy as np
import pytest

import _sampling_cases as cases
import kikuchipy_amd as kpa
from conftest import load_golden
from kikuchipy_amd import _lib, sampling

pytestmark = pytest.mark.gpu

KEPT_CASES = [(g, n) for n in cases.GPU_STEPS for g in cases.GROUPS] + [("432", 45)]


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def faces(group):
    return sampling.fundamental_zone_faces(group)


@pytest.mark.parametrize("group,n", KEPT_CASES)
def test_kernel_keeps_the_hosts_points_in_its_order(ctx, group, n):
    """27 points at n = 1 (the centre, the on-axis points and the w = pi surface in one wave), 3375 at n = 7 (several
    workgroups, a ragged last one).  Grid points lie 1e-3 and more apart as quaternions, so rows that agree to 1e-12 are
    the same points: the kept index set and its order are the host's."""
    q = cases.all_quaternions(n)
    want = q[sampling.in_fundamental_zone(q, faces(group))]
    got = ctx.sample_fundamental(n, faces(group))
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12
    if n == 22:
        assert got.shape[0] == cases.KEPT_AT_22[group]
    if n == 45:
        assert got.shape[0] == cases.KEPT_432_AT_45


@pytest.mark.parametrize("name", sorted(set(cases.LAUE) | set(cases.GROUPS)))
def test_every_name_runs_on_the_device(ctx, name):
    group = cases.LAUE.get(name, name)
    got = sampling.get_sample_fundamental(point_group=name, semi_edge_steps=3, context=ctx)
    q = cases.all_quaternions(3)
    assert np.abs(got - q[cases.definition_margin(q, cases.group_operations(group)) >= 0]).max() <= 1e-12


@pytest.mark.parametrize("n", cases.GPU_STEPS)
def test_quaternions_against_the_longdouble_restatement(ctx, n):
    got = ctx.sample_fundamental(n, np.zeros((0, 4)))  # the group 1: every grid point
    assert got.shape == ((2 * n + 1) ** 3, 4)
    err, floor, tol = cases.lost(got, n)
    print(n, "largest loss", err.max() / cases.EPS, "eps; largest share of the tolerance", (err / tol).max())
    assert (err <= tol).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 4 * cases.EPS and (got[:, 0] >= 0).all()
    assert np.array_equal(got[(2 * n + 1) ** 3 // 2], [1, 0, 0, 0])  # the cube's centre


def test_refused_calls_leave_the_context_usable(ctx, monkeypatch):
    lib = _lib.load()
    f = np.ascontiguousarray(faces("622"))
    out = np.full((40, 4), -1.0)
    count = C.c_int64(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fill, cnt = lib.kpdi_sample_fundamental_fill, lib.kpdi_sample_fundamental_count
    refused = [
        (cnt, (None, 3, p(f), 7, C.byref(count)), -1, "ctx is NULL"),
        (cnt, (ctx._h, 0, p(f), 7, C.byref(count)), -1, "semi_edge_steps 0: between 1 and 2048"),
        (cnt, (ctx._h, 2049, p(f), 7, C.byref(count)), -1, "semi_edge_steps 2049: between 1 and 2048"),
        (cnt, (ctx._h, 3, p(f), 24, C.byref(count)), -1, "24 faces: between 0 and 23"),
        (cnt, (ctx._h, 3, p(f), -1, C.byref(count)), -1, "-1 faces: between 0 and 23"),
        (cnt, (ctx._h, 3, None, 7, C.byref(count)), -1, "faces is NULL"),
        (cnt, (ctx._h, 3, p(f), 7, None), -1, "count is NULL"),
        (fill, (ctx._h, 3, p(f), 7, None, 40, C.byref(count)), -1, "out is NULL or capacity 40 is negative"),
        (fill, (ctx._h, 3, p(f), 7, p(out), -2, C.byref(count)), -1, "out is NULL or capacity -2 is negative"),
    ]
    for call, args, rc, text in refused:
        assert call(*args) == rc and _lib.last_error() == text, (text, _lib.last_error())
    assert count.value == -7 and (out == -1.0).all()  # nothing was written
    # too small an output: the count comes back, nothing is written
    want = ctx.sample_fundamental(3, f)
    assert 0 < want.shape[0] <= 40
    assert fill(ctx._h, 3, p(f), 7, p(out), want.shape[0] - 1, C.byref(count)) == -1
    assert _lib.last_error() == f"sampling with semi_edge_steps 3 keeps {want.shape[0]} orientations, out holds {want.shape[0] - 1}"
    assert count.value == want.shape[0] and (out == -1.0).all()
    # a size that does not fit the free device memory: the counts (a grid not seen before), then the kept quaternions
    # (on a context that holds no buffers yet; 887 counts of 4 bytes and 888 offsets of 8)
    monkeypatch.setenv("KPDI_SAMPLING_FREE_BYTES", "1000")
    with _lib.Context(0) as fresh:
        with pytest.raises(_lib.KpdiError, match="libkpdi error -5: sampling with semi_edge_steps 30: the counts of 887 workgroups "
                                                 "need 10652 bytes more, 1000 bytes of device memory are free"):
            fresh.sample_fundamental(30, f)
        with pytest.raises(_lib.KpdiError, match=r"libkpdi error -5: sampling with semi_edge_steps 2: 125 orientations need 4000 "
                                                 r"bytes, 1000 bytes of device memory are free"):
            fresh.sample_fundamental(2, np.zeros((0, 4)))
        monkeypatch.delenv("KPDI_SAMPLING_FREE_BYTES")
        assert fresh.sample_fundamental(2, np.zeros((0, 4))).shape == (125, 4)
    # and the context still works, with and without a count call before the fill
    assert np.array_equal(ctx.sample_fundamental(3, f), want)
    assert fill(ctx._h, 2, p(f), 7, p(out), 40, C.byref(count)) == 0 and count.value == 9
    assert np.array_equal(out[:count.value], ctx.sample_fundamental(2, f)) and (out[count.value:] == -1.0).all()
    with pytest.raises(_lib.KpdiError, match="semi_edge_steps 0: between 1 and 2048"):
        ctx.sample_fundamental(0, f)


def test_kernel_time_is_counted(ctx):
    ctx.set_profiling(1)
    try:
        ctx.sample_fundamental(7, faces("32"))
        assert ctx.counters()["sampling_ms"] > 0
    finally:
        ctx.set_profiling(0)


# ---- a hexagonal phase, end to end ---------------------------------------------------------------------------------------
A_HEX, C_HEX, MIN_D_HEX, WAVELENGTH = 2.95, 4.68, 0.8, 0.08586  # titanium-like, angstrom; electrons at 20 kV


def hexagonal_reflectors():
    """Every hkl with d >= MIN_D_HEX of a hexagonal lattice with a || x and c || z; |F| = 1 / (1 + |g|^2), real: a
    function of |g| alone, so the set has the full 6/mmm symmetry."""
    direct = np.array([[A_HEX, 0, 0], [-A_HEX / 2, A_HEX * np.sqrt(3) / 2, 0], [0, 0, C_HEX]])
    reciprocal = np.linalg.inv(direct).T  # rows a*, b*, c*
    r = range(-8, 9)
    hkl = np.array([(h, k, l) for h in r for k in r for l in r if (h, k, l) != (0, 0, 0)], dtype=np.float64)
    g = np.linalg.norm(hkl @ reciprocal, axis=1)
    hkl, g = hkl[g <= 1 / MIN_D_HEX], g[g <= 1 / MIN_D_HEX]
    assert np.abs(hkl).max() < 8  # the index range holds the whole sphere
    return kpa.Reflectors(hkl, np.arcsin(WAVELENGTH * g / 2), (1 / (1 + g * g)).astype(np.complex128), reciprocal, "hexagonal")


def ncc(a, b):
    a, b = a.reshape(a.shape[0], -1).astype(np.float64), b.reshape(b.shape[0], -1).astype(np.float64)
    a, b = a - a.mean(axis=1, keepdims=True), b - b.mean(axis=1, keepdims=True)
    return np.sum(a * b, axis=1) / np.sqrt(np.sum(a * a, axis=1) * np.sum(b * b, axis=1))


def test_hexagonal_phase_from_master_pattern_to_indexed_orientations(ctx):
    lam = kpa.KikuchiPatternSimulator(hexagonal_reflectors()).calculate_master_pattern(100, "both", context=ctx).as_lambert()
    rot = sampling.get_sample_fundamental(point_group="6/mmm", semi_edge_steps=10, device=0)
    q_all = cases.all_quaternions(10)
    assert np.abs(rot - q_all[cases.definition_margin(q_all, cases.group_operations("622")) >= 0]).max() <= 1e-12
    det = kpa.EBSDDetector(shape=(24, 24), pc=(0.42, 0.6, 0.5))
    dictionary = np.array(lam.get_patterns(rot, det, compute=True).data)
    assert dictionary.shape == (rot.shape[0], 24, 24) and dictionary.std(axis=(1, 2)).min() > 0
    # six entries at least 1e-3 inside every face: no duplicate of them sits on the opposite face
    f = faces("622")
    inside = np.min(f[:, 3][None] * rot[:, :1] - np.abs(rot[:, 1:] @ f[:, :3].T), axis=1) >= 1e-3
    pick = np.flatnonzero(inside)[np.linspace(0, inside.sum() - 1, 6).astype(int)]
    assert len(set(pick)) == 6
    ops = cases.group_operations("622")[[1, 2, 4, 6, 8, 11]]  # six non-identity operations, about z and in the plane
    assert np.abs(ops[:, 0]).max() < 1 - 1e-6
    # the side on which the projection is invariant
    sides = {"left": sampling.quaternion_product(ops, rot[pick]), "right": sampling.quaternion_product(rot[pick], ops)}
    agree = {side: ncc(np.array(lam.get_patterns(q, det, compute=True).data), dictionary[pick]) for side, q in sides.items()}
    side = max(agree, key=lambda s: agree[s].mean())
    other = "left" if side == "right" else "right"
    # ... against how well an entry agrees with its best other entry
    rest = np.array([np.delete(ncc(dictionary, np.broadcast_to(dictionary[i], dictionary.shape)), i).max() for i in pick])
    print("invariant on the", side, agree[side], "other side", agree[other], "best other dictionary entry", rest)
    assert (agree[side] > rest).all() and (agree[side] > agree[other]).all()
    patterns = np.array(lam.get_patterns(sides[side], det, compute=True).data)
    res = kpa.EBSD(patterns).dictionary_indexing(lam.get_patterns(rot, det), keep_n=1, verbose=False)
    assert np.array_equal(np.ravel(res.simulation_indices), pick)


def test_cubic_dictionary_of_the_reference_benchmark_sampled_on_the_device():
    """The reference benchmark's calls (tests/test_reference_benchmark.py) with the orientations from the kernel."""
    pre, proj = load_golden("preproc.npz"), load_golden("projection.npz")
    s = kpa.EBSD(pre["ni"].copy(), static_background=pre["ni_bg"])
    s.remove_static_background()
    s.remove_dynamic_background()
    mp = kpa.EBSDMasterPattern(np.stack([proj["mp_upper"], proj["mp_lower"]]))
    rot = sampling.get_sample_fundamental(resolution=6, point_group="m-3m", device=0)
    host = sampling.get_sample_fundamental(resolution=6, point_group="m-3m")
    assert rot.shape == (3557, 4) and np.abs(rot - host).max() <= 1e-12
    detector = kpa.EBSDDetector(shape=(60, 60), pc=(0.42, 0.22, 0.50), sample_tilt=70)
    signal_mask = ~kpa.filters.Window("circular", (60, 60)).astype(bool)
    res = s.dictionary_indexing(dictionary=mp.get_patterns(rot, detector), signal_mask=signal_mask, keep_n=1, verbose=False)
    assert np.isclose(res.scores.mean(), 0.1887, atol=1e-4), res.scores.mean()  # the reference benchmark's known answer
    want = s.dictionary_indexing(dictionary=mp.get_patterns(host, detector), signal_mask=signal_mask, keep_n=1, verbose=False)
    assert np.array_equal(res.simulation_indices, want.simulation_indices)
