"""Orientation sampling without a GPU: the generic face rule of kikuchipy_amd/sampling.py for every rotation group
against the DEFINITION of a fundamental zone (the smallest-angle member of a class, from groups enumerated independently
in tests/_sampling_cases.py), the kept counts at 22 steps, the generic rule against the cubic special case, the accepted
and refused names, three wrong restatements that these checks notice, what float64 loses against the `np.longdouble`
restatement, and csrc/sampling_plan.h compiled with the host compiler (launch arithmetic, grid decode, kept flags and
quaternions: the C++ the kernel runs)."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import _sampling_cases as cases
from conftest import ROOT
from kikuchipy_amd import _lib, sampling


def faces(group):
    return sampling.fundamental_zone_faces(group)


# ---- the groups ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", cases.GROUPS)
def test_operations_are_the_group(group):
    mine, want = sampling.rotation_group_operations(group), cases.group_operations(group)
    assert mine.shape == want.shape == (cases.ORDERS[group], 4)
    assert np.array_equal(mine[0], [1, 0, 0, 0]) and np.allclose(np.linalg.norm(mine, axis=1), 1, atol=1e-15)
    same = np.isclose(np.abs(mine @ want.T), 1, atol=1e-12)  # q and -q are one rotation
    assert (same.sum(axis=0) == 1).all() and (same.sum(axis=1) == 1).all()
    # one face pair per rotation axis, from the smallest angle about it
    f = faces(group)
    n_axes = {"1": 0, "2": 1, "222": 3, "4": 1, "422": 5, "3": 1, "32": 4, "6": 1, "622": 7, "23": 7, "432": 13}[group]
    assert f.shape == (n_axes, 4) and n_axes <= _lib.SAMPLING_MAX_FACES
    assert np.allclose(np.linalg.norm(f[:, :3], axis=1), 1, atol=1e-15)
    n_fold = {"1": 1, "2": 2, "222": 2, "4": 4, "422": 4, "3": 3, "32": 3, "6": 6, "622": 6, "23": 2, "432": 4}[group]
    if n_axes:
        along_z = f[np.abs(f[:, 2]) > 1 - 1e-12]
        assert along_z.shape[0] == 1 and np.isclose(along_z[0, 3], np.tan(np.pi / (2 * n_fold)), atol=1e-15)
    if group in ("222", "422", "32", "622"):  # the first two-fold axis is along x
        along_x = f[np.abs(f[:, 0]) > 1 - 1e-12]
        assert along_x.shape[0] == 1 and np.isclose(along_x[0, 3], 1.0, atol=1e-15)


# ---- the definition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", cases.GROUPS)
def test_kept_iff_smallest_angle_of_its_class(group):
    ops = cases.group_operations(group)
    for n in cases.STEPS:
        q = cases.all_quaternions(n)
        margin = cases.definition_margin(q, ops)
        print(group, n, "closest decision", np.abs(margin).min(), "kept", int((margin >= 0).sum()))
        assert np.abs(margin).min() >= 1e-10  # the premise: no decision hangs on the last bits
        want = margin >= 0
        assert np.array_equal(sampling.in_fundamental_zone(q, faces(group)), want)
        got = sampling.get_sample_fundamental(point_group=group, semi_edge_steps=n)
        assert got.dtype == np.float64 and np.array_equal(got, q[want])  # the kept rows, in grid order


def test_kept_counts_at_22_steps():
    q = cases.all_quaternions(22)
    got = {g: int(sampling.in_fundamental_zone(q, faces(g)).sum()) for g in cases.GROUPS}
    assert got == cases.KEPT_AT_22
    for laue, group in cases.LAUE.items():
        if laue not in sampling._FUNDAMENTAL_ZONES:  # (those keep their own path: the test below)
            assert sampling.get_sample_fundamental(point_group=laue, semi_edge_steps=22).shape == (got[group], 4), laue


@pytest.mark.parametrize("n", [1, 2, 3, 7, 22, 45])
def test_generic_rule_keeps_what_the_cubic_special_case_keeps(n):
    q = cases.all_quaternions(n)
    special = sampling.get_sample_fundamental(point_group="m-3m", semi_edge_steps=n)
    if n < 45:  # (the two names share one path)
        assert np.array_equal(sampling.get_sample_fundamental(point_group="432", semi_edge_steps=n), special)
    assert np.array_equal(q[sampling.in_fundamental_zone(q, faces("432"))], special)
    if n in (22, 45):
        assert special.shape[0] == {22: cases.KEPT_AT_22["432"], 45: cases.KEPT_432_AT_45}[n]


# ---- names and arguments ---------------------------------------------------------------------------------------------------
def test_names():
    assert sampling.ROTATION_GROUPS == cases.GROUPS
    for name in cases.GROUPS:
        assert sampling.rotation_group_name(name) == name
    for laue, group in cases.LAUE.items():
        assert sampling.rotation_group_name(laue) == group
    assert len(set(cases.GROUPS) | set(cases.LAUE)) == 22
    for name in cases.REFUSED:
        with pytest.raises(ValueError, match="pass the rotation group you want"):
            sampling.get_sample_fundamental(point_group=name, semi_edge_steps=1)
    with pytest.raises(NotImplementedError, match="point group '5'"):
        sampling.get_sample_fundamental(point_group="5", semi_edge_steps=1)

    class Symmetry:
        name = "6/mmm"

    assert np.array_equal(sampling.get_sample_fundamental(point_group=Symmetry(), semi_edge_steps=3),
                          sampling.get_sample_fundamental(point_group="622", semi_edge_steps=3))
    with pytest.raises(NotImplementedError, match="only the cubochoric sampling"):
        sampling.get_sample_fundamental(point_group="622", method="haar_euler", semi_edge_steps=1)


def test_arguments_are_validated_before_a_context_is_opened(monkeypatch):
    def no_context(*args, **kwargs):
        raise AssertionError("a context was opened")

    monkeypatch.setattr(_lib, "Context", no_context)
    with pytest.raises(ValueError, match="pass the rotation group you want"):
        sampling.get_sample_fundamental(point_group="-6m2", semi_edge_steps=1, device=0)
    with pytest.raises(NotImplementedError, match="only the cubochoric sampling"):
        sampling.get_sample_fundamental(point_group="m-3m", method="haar_euler", device=0)
    with pytest.raises(ValueError, match="resolution must be positive"):
        sampling.get_sample_fundamental(resolution=0, device=0)
    with pytest.raises(ValueError, match="semi_edge_steps 0"):
        sampling.get_sample_fundamental(semi_edge_steps=0, device=0)
    with pytest.raises(AssertionError, match="a context was opened"):
        sampling.get_sample_fundamental(point_group="m-3m", semi_edge_steps=1, device=0)


# ---- wrong restatements ---------------------------------------------------------------------------------------------------
def wrong_kept(group, n, wrong):
    q, f = cases.all_quaternions(n), faces(group).copy()
    if wrong == "open":  # neither face of a pair is kept
        keep = np.ones(q.shape[0], dtype=bool)
        for a0, a1, a2, t in f:
            keep &= np.abs(q[:, 1] * a0 + q[:, 2] * a1 + q[:, 3] * a2) < t * q[:, 0] - cases.SLACK
        return keep
    if wrong == "half_angle":  # tan(w / 2) from tan(w / 4); a half turn's face leaves to infinity
        t = f[:, 3]
        f[:, 3] = np.where(t < 1 - 1e-12, 2 * t / np.where(t < 1 - 1e-12, 1 - t * t, 1), np.inf)
    if wrong == "rotated":  # every axis turned by 15 degrees about z
        c, s = np.cos(np.radians(15)), np.sin(np.radians(15))
        f[:, :3] = f[:, :3] @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T
    with np.errstate(invalid="ignore"):
        return sampling.in_fundamental_zone(q, f)


def test_wrong_variants_are_noticed():
    """A face at tan(w/2) fails the table of counts for every group but 1; an open boundary fails it for the cyclic groups
    (their face through the w = pi surface holds 176 grid points at 22 steps; the on-face points of the other groups
    are cut off by another face); the two-fold axis of 32 at 15 degrees from x keeps 14167 points at 22 steps as the right
    setting does - the table cannot see it - and fails the definition at 7 and 22 steps."""
    for group in cases.GROUPS[1:]:
        assert int(wrong_kept(group, 22, "half_angle").sum()) != cases.KEPT_AT_22[group], group
    for group in ("2", "4", "3", "6"):
        assert int(wrong_kept(group, 22, "open").sum()) == cases.KEPT_AT_22[group] - 176, group
    ops = cases.group_operations("32")
    differing = {n: int((wrong_kept("32", n, "rotated") != (cases.definition_margin(cases.all_quaternions(n), ops) >= 0)).sum())
                 for n in cases.STEPS}
    print("32 with its two-fold axis at 15 degrees: points that leave the definition", differing)
    assert differing[7] > 0 and differing[22] > 0
    assert np.array_equal(wrong_kept("32", 22, "none"), cases.definition_margin(cases.all_quaternions(22), ops) >= 0)


# ---- what float64 loses --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.GPU_STEPS)
def test_host_path_stays_inside_the_floor(n):
    q = cases.all_quaternions(n)
    err, floor, tol = cases.lost(q, n)
    print(n, "largest loss", err.max() / cases.EPS, "eps; largest share of the floor", (err[floor > 0] / floor[floor > 0]).max())
    assert (err <= floor).all()
    assert (floor <= tol).all()
    assert np.array_equal(q[(2 * n + 1) ** 3 // 2], [1, 0, 0, 0])


def test_floor_is_led_by_the_cancellation_at_small_angles():
    zero = np.zeros((1, 1))
    at = [float(cases.floor(np.array([w]), zero)[0, 0]) / cases.EPS for w in (1e-3, 1e-2, 1e-1)]
    assert np.allclose(at, [1 / 1e-3, 1 / 1e-2, 1 / 1e-1], rtol=0.15)  # eps / w: the term eps w / (1 - cos w) / 2


# ---- csrc/sampling_plan.h with the host compiler ----------------------------------------------------------------------------
PLAN_PROBE = r"""
#include "sampling_plan.h"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
using namespace kpdi;
// stdin: lines "n n_faces f..."; per line: the kept flags of every point as 0/1, then (n <= 3) every quaternion
int main() {
  for (int n : {0, 1, 7, 22, 645, 2048, 2049}) {
    const SmpPlan p = smp_plan(n);
    printf("plan %d %d %d %lld %lld %d %d %lld %zu %zu\n", n, p.ok, p.side, (long long)p.points, (long long)p.blocks, p.threads,
           p.last_threads, (long long)p.scan_rounds, p.count_bytes, p.offset_bytes);
  }
  for (long long p : {0LL, 1LL, 44LL, 45LL, 2024LL, 2025LL, 91124LL}) {
    int ix, iy, iz;
    smp_decode(p, 45, &ix, &iy, &iz);
    printf("decode %lld %d %d %d %.17g\n", p, ix, iy, iz, smp_coordinate(iz, 22));
  }
  {
    int ix, iy, iz;
    const long long big = 1291LL * 1291 * 1291 - 2;  // n = 645: past 2^31
    smp_decode(big, 1291, &ix, &iy, &iz);
    printf("decode %lld %d %d %d %.17g\n", big, ix, iy, iz, smp_coordinate(iz, 645));
  }
  int n, nf;
  while (scanf("%d %d", &n, &nf) == 2) {
    SmpFaces f{};
    f.n = nf;
    for (int j = 0; j < nf; ++j)
      for (int k = 0; k < SMP_FACE_DOUBLES; ++k)
        if (scanf("%lf", &f.f[j][k]) != 1) return 1;
    const SmpPlan p = smp_plan(n);
    printf("flags ");
    for (long long i = 0; i < p.points; ++i) {
      double q[4];
      smp_point_quaternion(i, n, q);
      putchar(smp_in_zone(q, f) ? '1' : '0');
    }
    putchar('\n');
    if (nf == 0 && n <= 7) {
      printf("quaternions");
      for (long long i = 0; i < p.points; ++i) {
        double q[4];
        smp_point_quaternion(i, n, q);
        printf(" %.17g %.17g %.17g %.17g", q[0], q[1], q[2], q[3]);
      }
      putchar('\n');
    }
  }
  return 0;
}
"""

PROBE_CASES = [(g, n) for n in cases.STEPS for g in cases.GROUPS]


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("smpplan")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    text = "".join(f"{n} {faces(g).shape[0]} " + " ".join(repr(float(v)) for v in faces(g).ravel()) + "\n" for g, n in PROBE_CASES)
    return subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.strip().split("\n")


def test_plan_arithmetic(plan_lines):
    plans = {int(l.split()[1]): [int(v) for v in l.split()[2:]] for l in plan_lines if l.startswith("plan")}
    assert plans[0][0] == 0 and plans[2049][0] == 0  # refused
    # ok, side, points, workgroups, threads, lanes of the last workgroup, scan rounds, count bytes, offset bytes
    assert plans[1] == [1, 3, 27, 1, 256, 27, 1, 4, 16]
    assert plans[7] == [1, 15, 3375, 14, 256, 3375 - 13 * 256, 1, 56, 120]  # several workgroups, a ragged last one
    assert plans[22] == [1, 45, 91125, 356, 256, 91125 - 355 * 256, 1, 356 * 4, 357 * 8]
    assert plans[645][2] == 1291**3 > 2**31 and plans[645][3] == -(-(1291**3) // 256)  # a 64-bit point index
    assert plans[645][6] == -(-plans[645][3] // 1024)
    assert plans[2048][0] == 1 and plans[2048][3] < 2**31  # the largest grid: its workgroups fit a launch
    assert _lib.SAMPLING_MAX_STEPS == 2048


def test_grid_decode_is_the_host_paths(plan_lines):
    g = np.arange(-22, 23) * (np.pi ** (2 / 3) / 2 / 22)  # the host path's coordinates
    idx = cases.grid_indices(22)
    rows = [l.split()[1:] for l in plan_lines if l.startswith("decode")]
    for p, ix, iy, iz, coordinate in rows[:-1]:
        assert tuple(idx[int(p)]) == (int(ix), int(iy), int(iz))
        assert float(coordinate) == g[int(iz)]
    p, ix, iy, iz, coordinate = rows[-1]
    assert (int(ix), int(iy), int(iz)) == (1290, 1290, 1289) and int(p) > 2**31
    assert float(coordinate) == (np.arange(-645, 646) * (np.pi ** (2 / 3) / 2 / 645))[1289]


def test_header_keeps_what_the_numpy_path_keeps(plan_lines):
    flags = [l.split()[1] for l in plan_lines if l.startswith("flags")]
    assert len(flags) == len(PROBE_CASES)
    for (group, n), line in zip(PROBE_CASES, flags):
        got = np.frombuffer(line.encode(), dtype=np.uint8) == ord("1")
        want = sampling.in_fundamental_zone(cases.all_quaternions(n), faces(group))
        assert got.shape == want.shape and np.array_equal(got, want), (group, n)


def test_header_quaternions_stay_inside_the_tolerance(plan_lines):
    rows = [l.split()[1:] for l in plan_lines if l.startswith("quaternions")]
    steps = [n for g, n in PROBE_CASES if g == "1" and n <= 7]
    assert len(rows) == len(steps)
    for n, row in zip(steps, rows):
        q = np.array([float(v) for v in row]).reshape(-1, 4)
        err, _, tol = cases.lost(q, n)
        print(n, "largest loss", err.max() / cases.EPS, "eps")
        assert (err <= tol).all()
        assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 4 * cases.EPS and (q[:, 0] >= 0).all()
