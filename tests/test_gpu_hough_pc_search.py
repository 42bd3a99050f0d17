"""The projection-centre search kernel on the GPU: `EBSD.hough_indexing_optimize_pc(batch=True)` and
`Context.hough_optimize_pc` against the host path - SciPy's Nelder-Mead with one launch of the indexing kernel per step -
bit for bit, whatever the evaluations per launch and the lanes per workgroup; keywords the kernel does not know go to the
host; and the calibration workflow from a grid of patterns to per-point PCs.  60 x 60 patterns simulated from
tests/golden/projection.npz; every compared search runs with maxfev = 25."""

import numpy as np
import pytest

import _hough_cases as cases
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib
from kikuchipy_amd.indexing import _hough_indexing as hi

pytestmark = pytest.mark.gpu

SHAPE = (60, 60)
OPTIONS = dict(maxfev=25)
PC0 = np.array([0.43, 0.23, 0.51])


@pytest.fixture(scope="module")
def master():
    mpu, mpl = cases.master_pattern()
    return kpa.EBSDMasterPattern(np.stack([mpu, mpl]), hemisphere="both")


@pytest.fixture(scope="module")
def world(master):
    """The 12 simulated patterns, a constant one appended; their bands; what the search calls take; and the reference,
    computed once: the host path of the public call on the first four patterns (a 2 x 2 map) with SciPy's result of each
    of its searches kept, and further host searches on demand, kept too.  A host search costs a kernel launch and four
    downloads per evaluation, which is why every test shares these."""
    import warnings

    q, pcs = cases.simulated_inputs(SHAPE)
    data = master.get_patterns(q, kpa.EBSDDetector(SHAPE, pc=pcs), compute=True).data
    data = np.concatenate([np.asarray(data, dtype=np.float32), np.full((1,) + SHAPE, 0.5, dtype=np.float32)])
    s = kpa.EBSD(data)
    ix = kpa.EBSDDetector(SHAPE, pc=PC0).get_indexer(cases.POINT_GROUP)
    bands = ix.detect_bands(data, s.context)
    phase = ix.phaselist[0]
    args = (SHAPE, ix.sample_to_detector, phase.normals, phase.family, phase.angles, ix.tolerance(PC0))
    host, real = {}, hi._host_search

    class CountingContext:
        """The context as the host search sees it, its launches of the indexing kernel counted: an evaluation that
        launches none is one the objective answered with 180 because PCz > 0 was false."""

        def __init__(self):
            self.launches = 0

        def hough_index(self, *a):
            self.launches += 1
            return s.context.hough_index(*a)

    def host_result(i, pc0=PC0):
        key = (i, tuple(pc0))
        if key not in host:
            counting = CountingContext()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # SciPy: the budget ran out
                host[key] = real(counting, bands[i:i + 1], np.asarray(pc0), args, options=dict(OPTIONS))
            host[key].launches = counting.launches
        return host[key]

    four, seen = kpa.EBSD(data[:4].reshape((2, 2) + SHAPE)), []
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mp.setenv("KPDI_HOUGH_PC_SEARCH", "host")
        mp.setattr(hi, "_host_search", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
        host_api = four.hough_indexing_optimize_pc(PC0, ix, batch=True, options=dict(OPTIONS))
    assert len(seen) == 4  # one host search per pattern, in order
    host.update({(i, tuple(PC0)): res for i, res in enumerate(seen)})
    yield dict(signal=s, four=four, host_api=host_api, data=data, indexer=ix, bands=bands, args=args, host=host_result, ctx=s.context)
    four.close()
    s.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_bands_are_what_the_tests_need(world):
    valid = (world["bands"]["valid"] != 0).sum(axis=1)
    assert (valid[:12] >= 6).all() and valid[12] == 0  # the constant pattern has no band


def test_default_path_is_the_host_path(world, monkeypatch):
    """Four patterns through the public call: the device path, whatever the evaluations per launch, returns the bits of
    the call under KPDI_HOUGH_PC_SEARCH=host (made once, in `world`)."""
    s, host = world["four"], world["host_api"]
    monkeypatch.delenv("KPDI_HOUGH_PC_SEARCH", raising=False)
    monkeypatch.delenv("KPDI_HOUGH_SEARCH_EVALS", raising=False)
    monkeypatch.setattr(hi, "_host_search", None)  # the device path calls no host search
    device = s.hough_indexing_optimize_pc(PC0, world["indexer"], batch=True, options=dict(OPTIONS))
    per_launch = {}
    for evals in ("1", "7"):
        monkeypatch.setenv("KPDI_HOUGH_SEARCH_EVALS", evals)
        per_launch[evals] = s.hough_indexing_optimize_pc(PC0, world["indexer"], batch=True, options=dict(OPTIONS)).pc
    assert device.navigation_shape == host.navigation_shape == (2, 2) and device.shape == SHAPE
    assert np.array_equal(bits(device.pc), bits(host.pc)), (device.pc, host.pc)
    for evals, pc in per_launch.items():
        assert np.array_equal(bits(pc), bits(device.pc)), evals
    assert np.array_equal(bits(host.pc), bits(np.stack([world["host"](i).x for i in range(4)]).reshape(2, 2, 3)))
    assert np.abs(device.pc - PC0).max() > 0  # the searches moved


# m, and the lanes a workgroup is forced to hold in a second call (evaluations per launch changed with them): one lane group
# partly filled (1 of 64, 3 of 4), then the lane-group and workgroup edges crossed (65 = 64 + 1; 130 = 32 x 4 + 2).  An
# evaluation costs tens of milliseconds however few lanes work, so every case makes two device calls and no more.
@pytest.mark.parametrize("m, lanes, evals", [(1, 64, 0), (3, 4, 5), (65, 64, 0), (130, 4, 7)])
def test_context_call_tiled_over_lanes_and_workgroups(world, m, lanes, evals):
    originals = world["bands"][:5]
    tiled = originals[np.arange(m) % 5]
    planned = world["ctx"].hough_optimize_pc(tiled, PC0, *world["args"], **OPTIONS)  # the plan's lanes, the default evaluations
    forced = world["ctx"].hough_optimize_pc(tiled, PC0, *world["args"], **OPTIONS, lanes=lanes, evals_per_launch=evals)
    pc, fun, nfev, nit, status = planned
    assert pc.shape == (m, 3) and fun.shape == nfev.shape == nit.shape == status.shape == (m,)
    for a, b in zip(planned, forced):
        assert a.tobytes() == b.tobytes(), lanes
    for i in range(m):  # every copy equals its original
        o = i % 5
        assert pc[i].tobytes() == pc[o].tobytes() and fun[i] == fun[o] and (nfev[i], nit[i], status[i]) == (nfev[o], nit[o], status[o])
    for o, index in enumerate(range(5)[:m]):  # the originals equal the host path
        res = world["host"](index)
        assert np.array_equal(bits(pc[o]), bits(res.x)) and bits(fun[o]) == bits(res.fun), (o, pc[o], res.x)
        assert (nfev[o], nit[o], status[o]) == (res.nfev, res.nit, res.status), (o, nfev[o], nit[o], status[o], res)
        assert res.nfev == 25 and res.status == 1  # the budget is what ended it


def test_no_valid_band_and_starts_at_the_screen(world):
    """A pattern without a band, and starts before, on and behind the screen.  From PCz = 0 three vertices of the first
    simplex, from -0.01 every point asked for, have PCz <= 0: the host search answers those with 180 without a launch
    (counted), and the kernel's search must take the same branch to return the same bits."""
    ctx, args = world["ctx"], world["args"]
    behind = {}
    for rows, pc0 in (([12, 0], PC0), ([0], (0.42, 0.22, 0.01)), ([0], (0.42, 0.22, 0.0)), ([0], (0.42, 0.22, -0.01))):
        pc, fun, nfev, nit, status = ctx.hough_optimize_pc(world["bands"][rows], pc0, *args, **OPTIONS)
        for k, row in enumerate(rows):
            want = world["host"](row, pc0)
            assert np.array_equal(bits(pc[k]), bits(want.x)) and bits(fun[k]) == bits(want.fun), (row, pc0, pc[k], want.x)
            assert (nfev[k], nit[k], status[k]) == (want.nfev, want.nit, want.status)
        if len(rows) == 2:
            assert fun[0] == np.degrees(args[-1])  # no band: the tolerance everywhere
        else:
            behind[pc0[2]] = want.nfev - want.launches  # evaluations with PCz <= 0
    print("evaluations with PCz <= 0 by the start's PCz:", behind)
    assert behind[0.0] >= 3 and behind[-0.01] >= 4
    # a budget without a sane end is refused before anything is launched
    with pytest.raises(_lib.KpdiError, match="at most 10000 on the device"):
        ctx.hough_optimize_pc(world["bands"][:1], PC0, *args, maxfev=_lib.HOUGH_SEARCH_MAX_EVALS + 1)
    with pytest.raises(_lib.KpdiError, match="at most 10000 on the device"):
        ctx.hough_optimize_pc(world["bands"][:1], PC0, *args, maxiter=2**31 - 1)
    # the context is usable afterwards
    quat, fit, cm, nmatch = ctx.hough_index(world["bands"][:2], cases.simulated_inputs(SHAPE)[1][:2], *args)
    assert (nmatch >= 3).all() and np.isfinite(quat).all()


def test_other_keywords_go_to_the_host(world, monkeypatch):
    """`adaptive` and `bounds` are SciPy's business: the call hands them to the host search untouched and returns what it
    returns.  One pattern: a host search costs a launch per evaluation."""
    import warnings

    monkeypatch.delenv("KPDI_HOUGH_PC_SEARCH", raising=False)
    s = kpa.EBSD(world["data"][:1])
    calls, real = [], hi._host_search
    monkeypatch.setattr(hi, "_host_search", lambda *a, **k: calls.append((k, real(*a, **k))) or calls[-1][1])
    bounds = [(0.3, 0.6), (0.1, 0.4), (0.4, 0.6)]
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plain = s.hough_indexing_optimize_pc(PC0, world["indexer"], batch=True, options=dict(OPTIONS))
            assert not calls  # plain keywords: the kernel
            adaptive = s.hough_indexing_optimize_pc(PC0, world["indexer"], batch=True, options=dict(OPTIONS, adaptive=True))
            assert len(calls) == 1 and calls[0][0]["options"] == dict(OPTIONS, adaptive=True)
            bounded = s.hough_indexing_optimize_pc(PC0, world["indexer"], batch=True, options=dict(OPTIONS), bounds=bounds)
            assert len(calls) == 2 and calls[1][0]["bounds"] == bounds
    finally:
        s.close()
    assert np.array_equal(bits(adaptive.pc[0]), bits(calls[0][1].x)) and np.array_equal(bits(bounded.pc[0]), bits(calls[1][1].x))
    assert np.array_equal(bits(plain.pc[0]), bits(world["host"](0).x))
    assert plain.navigation_shape == adaptive.navigation_shape == bounded.navigation_shape == (1,)
    lo, hi_ = np.array(bounds).T
    assert (bounded.pc[0] >= lo).all() and (bounded.pc[0] <= hi_).all()


def test_workflow_from_a_grid_to_per_point_pcs(master):
    """extract a grid -> optimise every PC on the device -> fit a plane -> index with one PC per point."""
    q, _ = cases.simulated_inputs(SHAPE)
    i, j = np.indices((3, 4))
    truth = np.stack([0.42 - 0.004 * j, 0.22 + 0.003 * i, 0.50 - 0.0013 * i], axis=-1)
    det = kpa.EBSDDetector(SHAPE, pc=truth.reshape(-1, 3))
    data = np.asarray(master.get_patterns(q, det, compute=True).data, dtype=np.float32).reshape((3, 4) + SHAPE)
    s = kpa.EBSD(data)
    try:
        s.to_device()
        ix = kpa.EBSDDetector(SHAPE, pc=truth.reshape(-1, 3).mean(axis=0)).get_indexer(cases.POINT_GROUP)
        found = s.hough_indexing_optimize_pc(ix.PC, ix, batch=True)
        assert s.is_resident and found.navigation_shape == (3, 4)
        indices = np.stack([i, j])
        fitted = found.fit_pc(indices, indices, transformation="affine", plot=False)
        rms_found = float(np.sqrt(np.mean((found.pc - truth) ** 2)))
        rms_fitted = float(np.sqrt(np.mean((fitted.pc - truth) ** 2)))
        print("RMS deviation from the true PCs: found", rms_found, "fitted", rms_fitted, "sample tilt", fitted.sample_tilt)
        # the least-squares projection onto a model that contains the truth cannot increase the 2-norm of the error
        assert rms_fitted <= rms_found
        xmap = s.hough_indexing(cases.POINT_GROUP, fitted.get_indexer(cases.POINT_GROUP), verbose=0)
    finally:
        s.close()
    assert xmap.shape == (3, 4) and (xmap.phase_id == 0).all() and (xmap.nmatch >= 3).all()
