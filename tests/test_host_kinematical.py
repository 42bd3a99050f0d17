"""Kinematical master patterns without a GPU: the NumPy restatement against the reference's own `get_pattern`
(tests/golden/kinematical.npz, tools/gen_kinematical_golden.py), that every case reaches the branches it claims and that
three wrong restatements would be noticed, csrc/kinematical_plan.h compiled with the host compiler (geometry, chunking,
LDS budget, the pixel directions bit for bit, the acos screen), `EBSDMasterPattern.as_lambert` / `deepcopy` against the
reference's steps, the mirrored signatures and every refused call with its text."""

import inspect
import json
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import _kinematical_cases as cases
import _kinematical_restate as restate
import kikuchipy_amd as kpa
from conftest import ROOT, load_golden
from kikuchipy_amd import simulations

GOLDEN = load_golden("kinematical.npz")
BY_NAME = {c["name"]: c for c in cases.cases() + [cases.END_TO_END]}
GOLDEN_CASES = [c["name"] for c in cases.cases() + [cases.END_TO_END] if c["golden"]]


# ---- the fixture and the restatement ---------------------------------------------------------------------------------
def test_inputs_regenerate_bit_for_bit():
    for which in ("ni", "handmade"):
        u, theta, f = cases.reflectors(which)
        assert np.array_equal(u, GOLDEN[f"in__{which}__unit_vectors"])
        assert np.array_equal(theta, GOLDEN[f"in__{which}__theta"])
        assert np.array_equal(f, GOLDEN[f"in__{which}__structure_factor"])
    hkl = cases.ni_reflectors()[0]
    assert hkl.shape == (338, 3) and np.array_equal(hkl, GOLDEN["in__ni__hkl"])
    d = cases.A_NI / np.sqrt(np.sum(hkl**2, axis=1))
    assert d.min() >= cases.MIN_D and np.abs(hkl).max() == 6
    assert cases.CHUNK == 256 and cases.FORCED_CHUNK < cases.CHUNK


def test_every_golden_case_is_stored_and_no_other():
    stored = sorted(k[4:] for k in GOLDEN.files if k.startswith("mp__"))
    assert stored == sorted(GOLDEN_CASES)
    assert [c["name"] for c in cases.cases() if not c["golden"]]  # (some cases rest on the restatement alone)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    case = BY_NAME[name]
    got = restate.master_pattern(case)
    want = GOLDEN[cases.key(case)]
    size = 2 * case["half_size"] + 1
    assert got.dtype == np.float64 and got.shape == ((2, size, size) if case["hemisphere"] == "both" else (size, size))
    assert np.array_equal(got, want)
    # the cap of the GPU comparison is a condition on the inputs: at most 1 % of a case's pixels lie near a threshold
    assert restate.left_out(case).mean() <= 0.01


def test_ni_cases_leave_no_pixel_out():
    """With the Ni list no pixel lies within 1e-12 of a threshold (half_size 8, 20 and 50)."""
    for name in ("ni_h8_both", "ni_h20_both", "ni_h50_both"):
        assert not restate.left_out(BY_NAME[name]).any(), name


# ---- the branches --------------------------------------------------------------------------------------------------
# what a case claims to reach: pairs on the half-intensity branch, in a band, with D < 0 inside the mirrored band (a
# symmetric band test would count them), with D >= 1
CLAIMS = {
    "ni_h8_both": ("half", "band", "negative_in_mirror_band"),
    "ni_h20_both": ("half", "band", "negative_in_mirror_band"),
    "ni_h1_both": ("half", "band"),
    "handmade_h8_both": ("half", "band", "negative_in_mirror_band", "d_ge_1"),
    "handmade_h20_both": ("half", "band", "negative_in_mirror_band", "d_ge_1"),
    "ni_m1_c16": ("band",),
}


@pytest.mark.parametrize("name", sorted(CLAIMS))
def test_cases_reach_the_branches_they_claim(name):
    counts = {}
    restate.master_pattern(BY_NAME[name], counts=counts, screen=1e-6)
    print(name, counts)
    for branch in CLAIMS[name]:
        assert counts[branch] > 0, (name, branch, counts)
    assert counts["acos"] <= counts["pairs"]


def test_handmade_reflectors_are_what_they_say():
    u, theta, _ = cases.handmade_reflectors()
    v = cases.directions(8, -1)
    centre = 8 * 17 + 8
    assert cases.dot_plain(u[0], v[centre]) == 1.0           # +z: D = 1 at the centre pixel
    assert cases.dot_plain(u[1], v[centre]) == 0.0           # equatorial: D exactly 0
    assert all(cases.dot_plain(u[1], v[r * 17 + 8]) == 0.0 for r in range(17))
    assert theta[2] == 0.0 and all(cases.dot_plain(u[2], v[r * 17 + (16 - r)]) == 0.0 for r in range(17))
    hit = [i for i in range(v.shape[0]) if np.array_equal(v[i], u[3])]
    assert len(hit) == 1 and cases.dot_plain(u[3], v[hit[0]]) > 1.0 >= cases.dot_fma(u[3], v[hit[0]])
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.arccos(cases.dot_plain(u[3], v[hit[0]])))  # D > 1 by rounding: NaN, nothing is added


@pytest.mark.parametrize("wrong", ["symmetric", "no_half", "fma"])
def test_a_wrong_restatement_differs_from_the_fixture(wrong):
    names = ("handmade_h8_both", "ni_h1_both") if wrong == "fma" else ("handmade_h8_both", "ni_h8_both", "ni_h20_both")
    differs = [n for n in names if not np.array_equal(restate.master_pattern(BY_NAME[n], wrong=wrong),
                                                      GOLDEN[cases.key(BY_NAME[n])])]
    print(wrong, "differs on", differs)
    assert differs
    if wrong == "fma":  # the pixel of the parallel reflector, where the contracted dot product is not above 1
        assert "handmade_h8_both" in differs


# ---- csrc/kinematical_plan.h on the host ---------------------------------------------------------------------------
PLAN_PROBE = r"""
#include "kinematical_plan.h"
#include <cstdio>
#include <initializer_list>
using namespace kpdi;
int main() {
  const long long ms[] = {1, 15, 16, 17, 255, 256, 257, 338, 1000};
  const int hs[] = {0, 1, 8, 20, 500, 4096};
  const int forces[] = {0, 1, 16, 300};
  for (long long m : ms) for (int h : hs) for (int code = 0; code < 3; ++code) for (int f : forces) {
    KinPlan p = kin_plan(m, h, code, f);
    std::printf("plan %lld %d %d %d %d %d %lld %d %d %d %d %d %d %d %d %zu\n", m, h, code, f, p.ok, p.size, (long long)p.pixels,
                p.hemispheres, p.grid_x, p.grid_y, p.threads, p.last_threads, p.chunk, p.n_chunks, p.tail, p.lds_bytes);
  }
  const KinPlan bad[] = {kin_plan(0, 8, 0), kin_plan(5, -1, 0), kin_plan(5, 8, 3), kin_plan(5, 8, -1), kin_plan(5, 4097, 2)};
  for (auto &p : bad) std::printf("bad %d\n", p.ok);
  std::printf("const %d %d %d %zu %d %a %a\n", KIN_THREADS, KIN_CHUNK, KIN_ENTRY_DOUBLES, KIN_LDS_BYTES, KIN_MAX_HALF_SIZE,
              KIN_HALF_WIDTH, KIN_SCREEN);
  for (int code = 0; code < 3; ++code) std::printf("zsign %d %g %g\n", code, kin_zsign(code, 0), kin_zsign(code, 1));
  for (int h : {0, 1, 8, 20, 50}) {
    const int size = 2 * h + 1;
    for (int r = 0; r < size; ++r) for (int c = 0; c < size; ++c) {
      double v[3];
      kin_direction(kin_axis(c, size), kin_axis(r, size), v);
      std::printf("dir %d %a %a %a\n", h, v[0], v[1], v[2]);
    }
  }
  const double thetas[] = {0.0, 0.02, 0.0845, 1.0, 1.5707963267948966, -0.1, 1.7, 4.0, -2.0};
  for (double t : thetas) {
    double lo, hi;
    kin_screen(1.5707963267948966 - t, &lo, &hi);
    std::printf("screen %a %a %a\n", t, lo, hi);
  }
  double lo, hi;
  kin_screen(std::nan(""), &lo, &hi);
  std::printf("screen nan %a %a\n", lo, hi);
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("kinplan")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")


def test_plan_geometry_chunking_and_lds_budget(plan_lines):
    assert [ln for ln in plan_lines if ln.startswith("bad")] == ["bad 0"] * 5
    const = [ln for ln in plan_lines if ln.startswith("const")][0].split()
    threads, chunk, entry, lds, max_half = int(const[1]), int(const[2]), int(const[3]), int(const[4]), int(const[5])
    assert (threads, chunk, entry, max_half) == (256, cases.CHUNK, 8, kpa._lib.KINEMATICAL_MAX_HALF_SIZE)
    assert float.fromhex(const[6]) == 1e-7 and float.fromhex(const[7]) == 1e-6
    # the table of one chunk, and 8 workgroups of it (the 2048 lanes of a CU) within the CU's 160 KiB of LDS
    assert lds == chunk * entry * 8 == 16384 and 8 * lds <= 160 * 1024
    assert [ln.split()[1:] for ln in plan_lines if ln.startswith("zsign")] == [["0", "1", "1"], ["1", "-1", "-1"], ["2", "1", "-1"]]
    seen = 0
    for ln in plan_lines:
        if not ln.startswith("plan"):
            continue
        m, h, code, force, ok, size, pixels, hemis, gx, gy, thr, last, ch, nch, tail, lds_b = map(int, ln.split()[1:])
        seen += 1
        assert ok == 1 and size == 2 * h + 1 and pixels == size * size and hemis == (2 if code == 2 else 1)
        assert thr == threads and gy == hemis and gx == -(-pixels // threads) and lds_b == lds
        assert (gx - 1) * threads + last == pixels and 1 <= last <= threads   # every pixel has one lane
        assert ch == (chunk if force == 0 else min(force, chunk))
        assert (nch - 1) * ch + tail == m and 1 <= tail <= ch                # every reflector is in one stage
    assert seen == 9 * 6 * 3 * 4


def test_pixel_directions_equal_numpy_bit_for_bit(plan_lines):
    got = {}
    for ln in plan_lines:
        if ln.startswith("dir"):
            _, h, a, b, c = ln.split()
            got.setdefault(int(h), []).append([float.fromhex(a), float.fromhex(b), float.fromhex(c)])
    for h in (0, 1, 8, 20, 50):
        want = cases.directions(h, -1)
        assert np.array_equal(np.array(got[h]), want), h
        # the lower hemisphere is the upper one with z negated, exactly
        lower = cases.directions(h, 1)
        assert np.array_equal(lower[:, :2], want[:, :2]) and np.array_equal(lower[:, 2], -want[:, 2])
    assert np.array_equal(cases.directions(0, -1), [[-2 / 3, -2 / 3, -1 / 3]])  # np.linspace(-1, 1, 1) is [-1]


def test_acos_screen_decides_like_acos(plan_lines):
    """Pairs that the screen decides without acos fall where the reference's acos test puts them: for every reflector and
    pixel of the larger cases, D <= lo is in the band and D >= hi is not; out-of-range angles have no screen."""
    screens = {}
    for ln in plan_lines:
        if ln.startswith("screen nan"):
            assert [float.fromhex(x) for x in ln.split()[2:]] == [-np.inf, np.inf]
        elif ln.startswith("screen"):
            t, lo, hi = (float.fromhex(x) for x in ln.split()[1:])
            screens[t] = (lo, hi)
    for t in (1.7, 4.0, -2.0):  # pi/2 - theta outside [0, pi]: every pair with D > 1e-7 evaluates acos
        assert screens[t] == (-np.inf, np.inf)
    for t in (0.0, 0.02, 0.0845, 1.0, 1.5707963267948966, -0.1):
        c = np.cos(np.pi / 2 - t)
        assert screens[t] == (c - 1e-6, c + 1e-6)
    skipped = total = 0
    for name in ("ni_h20_both", "handmade_h20_both", "ni_h50_both"):
        case = BY_NAME[name]
        u, theta, _ = cases.reflectors(case["reflectors"], case["m"])
        theta1 = np.pi / 2 - theta
        for pole in (-1, 1):
            v = cases.directions(case["half_size"], pole)
            d = (u[:, None, 0] * v[None, :, 0] + u[:, None, 1] * v[None, :, 1]) + u[:, None, 2] * v[None, :, 2]
            with np.errstate(invalid="ignore"):
                angle = np.arccos(d)
            band = (angle <= np.pi / 2) & (angle >= theta1[:, None])
            positive = d > 1e-7
            lo, hi = np.cos(theta1)[:, None] - 1e-6, np.cos(theta1)[:, None] + 1e-6
            assert band[positive & (d <= lo)].all() and not band[positive & (d >= hi)].any()
            assert not band[d < -1e-7].any()
            skipped += int((positive & ((d <= lo) | (d >= hi))).sum()) + int((d <= 1e-7).sum())
            total += d.size
    assert skipped / total > 0.999  # (the screen is worth having: fewer than 1 in 1000 pairs evaluate acos)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_screened_decisions_give_the_reference_bit_for_bit(name):
    """The kernel's branch structure, restated in NumPy, on every stored case."""
    case = BY_NAME[name]
    u, theta, f = cases.reflectors(case["reflectors"], case["m"])
    inten = cases.intensity(f, case["scaling"])
    got = [restate.get_pattern_screened(inten, cases.directions(case["half_size"], pole), u, theta)
           for pole in cases.poles(case["hemisphere"])]
    assert np.array_equal(np.array(got).reshape(GOLDEN[cases.key(case)].shape), GOLDEN[cases.key(case)])


# ---- as_lambert, deepcopy ------------------------------------------------------------------------------------------
def lambert_close(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and bool(np.all(np.abs(a - b) <= np.spacing(np.abs(b))))


@pytest.fixture(scope="module")
def stereographic():
    data = GOLDEN[cases.key(cases.END_TO_END)]
    return kpa.EBSDMasterPattern(data, projection="stereographic", hemisphere="both", phase_name="ni")


def test_as_lambert_equals_the_reference_steps(stereographic):
    want = GOLDEN["lambert__" + cases.END_TO_END["name"]]
    lam = stereographic.as_lambert()
    assert lam is not stereographic and lam.projection == "lambert" and lam.hemisphere == "both"
    assert lam.phase_name == "ni" and lam.has_inversion_symmetry is True and lam.energies is None
    assert lambert_close(lam.data, want)
    assert stereographic.projection == "stereographic" and stereographic.data.dtype == np.float64  # (untouched)
    assert lam._is_suitable_for_projection()
    # progress bar flag of the reference's signature: accepted, no effect
    assert np.array_equal(stereographic.as_lambert(show_progressbar=False).data, lam.data)


def test_as_lambert_of_every_navigation_shape(stereographic):
    want = GOLDEN["lambert__" + cases.END_TO_END["name"]]
    data = stereographic.data
    one = kpa.EBSDMasterPattern(data[1], projection="stereographic", hemisphere="lower").as_lambert()
    assert one.hemisphere == "lower" and lambert_close(one.data, want[1])
    energies = kpa.EBSDMasterPattern(data[::-1], projection="stereographic", hemisphere="upper", energies=[10, 20]).as_lambert()
    assert np.array_equal(energies.energies, [10, 20]) and lambert_close(energies.data, want[::-1])
    both = kpa.EBSDMasterPattern(np.stack([data, data[::-1]]), projection="stereographic", hemisphere="both",
                                 energies=[15.0, 20.0])
    lam = both.as_lambert()
    assert lam.data.shape == (2, 2, 101, 101) and lambert_close(lam.data, np.stack([want, want[::-1]]))
    up, lo = lam._get_master_pattern_arrays_from_energy(15)
    assert np.array_equal(up, lam.data[0, 0]) and np.array_equal(lo, lam.data[1, 0])


def test_as_lambert_of_a_lambert_pattern_warns_and_copies():
    mp = kpa.EBSDMasterPattern(np.arange(50, dtype=np.float32).reshape(2, 5, 5), hemisphere="both", phase_name="x")
    with pytest.warns(UserWarning) as w:
        out = mp.as_lambert()
    assert str(w[0].message) == "Already in the Lambert projection, returning a deepcopy"
    assert out is not mp and out.data is not mp.data and np.array_equal(out.data, mp.data) and out.projection == "lambert"


def test_deepcopy_shares_nothing():
    mp = kpa.EBSDMasterPattern(np.zeros((2, 2, 5, 5), dtype=np.float32), hemisphere="both", energies=[10, 20], phase_name="x",
                               has_inversion_symmetry=False)
    cp = mp.deepcopy()
    assert type(cp) is type(mp) and cp is not mp
    cp.data[:] = 1
    cp.energies[0] = 5
    assert not mp.data.any() and mp.energies[0] == 10
    assert (cp.hemisphere, cp.projection, cp.phase_name, cp.has_inversion_symmetry) == ("both", "lambert", "x", False)


def test_stereographic_pattern_is_still_refused_by_get_patterns(stereographic):
    det = kpa.EBSDDetector(shape=(24, 24), pc=(0.5, 0.5, 0.5))
    with pytest.raises(NotImplementedError, match="Master pattern must be in the square Lambert projection"):
        stereographic.get_patterns(np.array([[1.0, 0, 0, 0]]), det)


# ---- the Python surface --------------------------------------------------------------------------------------------
def test_signatures_equal_the_reference():
    table = json.loads(str(GOLDEN["signatures"]))
    ours = {"KikuchiPatternSimulator.__init__": kpa.KikuchiPatternSimulator.__init__,
            "KikuchiPatternSimulator.calculate_master_pattern": kpa.KikuchiPatternSimulator.calculate_master_pattern,
            "KikuchiMasterPattern.as_lambert": kpa.EBSDMasterPattern.as_lambert}
    assert sorted(table) == sorted(ours)
    assert table["KikuchiPatternSimulator.calculate_master_pattern"] == [["half_size", 500], ["hemisphere", "upper"],
                                                                       ["scaling", "linear"]]
    for name, fn in ours.items():
        params = list(inspect.signature(fn).parameters.values())[1:]
        positional = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert [[p.name, "<required>" if p.default is p.empty else p.default] for p in positional] == table[name], name
        for p in params:  # what this package adds can only be given by keyword, and never has to be
            if p not in positional:
                assert p.kind == p.KEYWORD_ONLY and p.default is not p.empty, (name, p.name)
    extra = inspect.signature(kpa.KikuchiPatternSimulator.calculate_master_pattern).parameters
    assert extra["device"].default == 0 and extra["context"].default is None
    assert list(inspect.signature(kpa.Reflectors.__init__).parameters)[1:] == [
        "hkl", "theta", "structure_factor", "reciprocal_basis", "phase_name", "has_inversion_symmetry"]
    assert kpa.Reflectors is simulations.Reflectors and "KikuchiPatternSimulator" in kpa.__all__ and "Reflectors" in kpa.__all__


def ni(**kwargs):
    hkl, theta, f = cases.ni_reflectors()
    return kpa.Reflectors(hkl, theta, f, phase_name="ni", **kwargs)


def test_reflectors_holder():
    ref = ni()
    assert ref.size == 338 and np.array_equal(ref.unit_vectors, cases.unit_vectors(ref.hkl))
    # a non-cubic basis: rows a*, b*, c*
    basis = np.array([[0.5, 0, 0], [0, 0.25, 0], [0.1, 0, 0.2]])
    ref = kpa.Reflectors([[1, 0, 0], [0, 2, 0], [1, 1, 1]], [0.1, 0.2, 0.3], reciprocal_basis=basis)
    want = np.array([[0.5, 0, 0], [0, 0.5, 0], [0.6, 0.25, 0.2]])
    assert np.allclose(ref.unit_vectors, want / np.linalg.norm(want, axis=1)[:, None], rtol=0, atol=1e-15)
    assert np.isnan(ref.structure_factor).all() and ref.structure_factor.dtype == np.complex128
    for bad in ([1, 2], np.zeros((2, 2, 3))):
        with pytest.raises(ValueError, match=r"\(m, 3\) expected"):
            kpa.Reflectors(bad, [0.1])
    with pytest.raises(ValueError, match="3 reflectors but 2 Bragg angles"):
        kpa.Reflectors(np.eye(3), [0.1, 0.2])
    with pytest.raises(ValueError, match=r"reciprocal_basis of shape \(2, 2\)"):
        kpa.Reflectors(np.eye(3), [0.1, 0.2, 0.3], reciprocal_basis=np.eye(2))


def test_simulator_keeps_a_copy_and_prints_like_the_reference():
    ref = ni()
    sim = kpa.KikuchiPatternSimulator(ref)
    assert sim.reflectors is not ref and np.array_equal(sim.reflectors.hkl, ref.hkl)
    ref.theta[0] = np.nan
    assert not np.isnan(sim.reflectors.theta[0])
    assert repr(sim) == "KikuchiPatternSimulator:\n" + repr(sim.reflectors)


class StandInContext:
    """Answers `kinematical_master_pattern` from the restatement's loop: what reaches the library, and what comes back."""

    def __init__(self):
        self.calls = []

    def kinematical_master_pattern(self, unit_vectors, theta, intensity, half_size, hemisphere):
        self.calls.append((unit_vectors, theta, intensity, half_size, hemisphere))
        size = 2 * half_size + 1
        out = [restate.get_pattern(intensity, cases.directions(half_size, pole), unit_vectors, theta)
               for pole in cases.poles(hemisphere)]
        out = np.array(out).reshape(-1, size, size)
        return out if hemisphere == "both" else out[0]


@pytest.mark.parametrize("name", ["ni_h8_both", "ni_h8_upper", "ni_h8_lower", "ni_h8_both_square", "ni_h8_both_none"])
def test_calculate_master_pattern_hands_the_reference_intensities_to_the_library(name):
    case = BY_NAME[name]
    ctx = StandInContext()
    mp = kpa.KikuchiPatternSimulator(ni()).calculate_master_pattern(case["half_size"], case["hemisphere"].upper(),
                                                                  case["scaling"], context=ctx)
    (u, theta, intensity, half_size, hemisphere), = ctx.calls
    ru, rtheta, rf = cases.reflectors("ni")
    assert np.array_equal(u, ru) and np.array_equal(theta, rtheta) and np.array_equal(intensity, cases.intensity(rf, case["scaling"]))
    assert (half_size, hemisphere) == (case["half_size"], case["hemisphere"])
    assert isinstance(mp, kpa.EBSDMasterPattern) and mp.projection == "stereographic" and mp.hemisphere == case["hemisphere"]
    assert mp.phase_name == "ni" and mp.has_inversion_symmetry is True and mp.data.dtype == np.float64
    assert np.array_equal(mp.data, GOLDEN[cases.key(case)])
    assert not mp._is_suitable_for_projection()


def test_an_object_shaped_like_a_reciprocal_lattice_vector_is_accepted():
    class Unit:
        data = cases.reflectors("ni", 5)[0]

    class PointGroup:
        contains_inversion = False

    class Phase:
        name = "fake"
        point_group = PointGroup()

    class Rlv:
        hkl, theta, structure_factor, unit, phase, size = cases.ni_reflectors()[0][:5], cases.reflectors("ni", 5)[1], \
            cases.reflectors("ni", 5)[2], Unit(), Phase(), 5

        def deepcopy(self):
            return self

        def flatten(self):
            return self

    ctx = StandInContext()
    mp = kpa.KikuchiPatternSimulator(Rlv()).calculate_master_pattern(1, "both", context=ctx)
    assert np.array_equal(ctx.calls[0][0], Unit.data) and mp.phase_name == "fake" and mp.has_inversion_symmetry is False
    assert mp.data.shape == (2, 3, 3)


def test_refused_calls_and_their_texts():
    hkl, theta, f = cases.ni_reflectors()
    ctx = StandInContext()
    sim = kpa.KikuchiPatternSimulator(ni())
    with pytest.raises(ValueError) as e:
        sim.calculate_master_pattern(8, "upper", "cubic", context=ctx)
    assert str(e.value) == "Unknown scaling 'cubic', options are 'linear', 'square', or None"
    with pytest.raises(ValueError) as e:
        sim.calculate_master_pattern(8, "north", context=ctx)
    assert str(e.value) == "Unknown hemisphere 'north', options are 'upper', 'lower', or 'both'"
    with pytest.raises(ValueError) as e:
        kpa.KikuchiPatternSimulator(kpa.Reflectors(hkl, None, f)).calculate_master_pattern(8, context=ctx)
    assert str(e.value) == ("Reflectors have no Bragg angles. Calculate with "
                            "`diffsims.crystallography.ReciprocalLatticeVector.calculate_theta()`.")
    with pytest.raises(ValueError) as e:
        kpa.KikuchiPatternSimulator(kpa.Reflectors(hkl, theta)).calculate_master_pattern(8, context=ctx)
    assert str(e.value) == ("Reflectors have no structure factors. Calculate with "
                            "`diffsims.crystallography.ReciprocalLatticeVector.calculate_structure_factor()`.")
    # the order of the reference: Bragg angles, structure factors, hemisphere, scaling
    with pytest.raises(ValueError, match="no Bragg angles"):
        kpa.KikuchiPatternSimulator(kpa.Reflectors(hkl, None)).calculate_master_pattern(8, "north", "cubic", context=ctx)
    with pytest.raises(ValueError, match="Unknown hemisphere"):
        sim.calculate_master_pattern(8, "north", "cubic", context=ctx)
    assert not ctx.calls  # nothing reached the library
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="Unknown projection 'gnomonic'"):
            kpa.EBSDMasterPattern(np.zeros((3, 3)), projection="gnomonic")
