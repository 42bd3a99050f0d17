"""Disorientation angles, zone reduction and KAM maps without a GPU: the NumPy host path of kikuchipy_amd/orientations.py
against the `np.longdouble` restatement of tests/_orientation_cases.py within the bound derived there, for every rotation
group and three mixed pairs; csrc/orientations_plan.h compiled with the host compiler (tiles, passes, the 64-bit output
index, and the pair / reduce functions the kernels run); the refusals; +q and -q giving the same bits; and three wrong
variants that the tables notice."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import _orientation_cases as cases
import kikuchipy_amd as kpa
from conftest import ROOT
from kikuchipy_amd import _lib, orientations, sampling
from kikuchipy_amd.filters import Window

U = cases.U


def test_operation_tables_are_within_the_bounds_premise():
    for group in cases.GROUPS:
        ordered, off = cases.ld_operations(group)
        print(group, "largest table error", off / U, "U")
        assert off <= cases.TABLE * U
        assert np.abs((ordered * ordered).sum(axis=1) - 1).max() < 1e-18


def test_bound_is_what_the_docstring_derives():
    assert (cases.EQUIV, cases.DOT) == (24, 100) and 176 < cases.VEC < 177 and 566 < cases.ANGLE < 567
    assert cases.angle_bound(0.0) < 6.4e-14


# ---- the host path against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("g1,g2", cases.GROUP_PAIRS)
def test_host_outer_and_pairs_stay_inside_the_bound(g1, g2):
    a, b = cases.pools(g1, g2)
    theta, slack = cases.outer_reference(g1, g2)
    got = kpa.disorientation_angle_outer(a, b, g1, g2)
    assert got.dtype == np.float64 and got.shape == theta.shape
    err, bound = cases.lost(got, theta, slack)
    print(g1, g2, "largest share of the bound", (err[bound > 0] / bound[bound > 0]).max(), "largest slack", slack.max())
    assert (err <= bound).all()
    assert np.isnan(got[list(cases.INVALID_ROWS_A)]).all() and np.isnan(got[:, list(cases.INVALID_ROWS_B)]).all()
    assert np.isnan(got).sum() == cases.POOL * 3 - 2  # those and no other
    for degrees in (False, True):
        diag = kpa.disorientation_angle(a, b, g1, g2, degrees)
        err, bound = cases.lost(diag, np.diag(theta), np.diag(slack), degrees)
        assert (err <= bound).all()
    # the special rows of the diagonal: identical, another length, -q, exact equivalents: an angle within the bound of 0
    assert (np.diag(got)[:5] <= cases.angle_bound(np.diag(slack)[:5])).all()


def test_group_1_is_the_plain_rotation_angle():
    a, b = cases.pools("1", "1")
    theta, _ = cases.outer_reference("1", "1")
    d = np.diag(theta).astype(np.float64)
    assert np.allclose(d[5:11], [1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-3], rtol=1e-6) and abs(d[11] - np.pi) < 1e-15 and d[12] == np.pi


def test_broadcasting_and_inputs():
    a, b = cases.pools("432", "432")
    theta, slack = cases.outer_reference("432", "432")
    got = kpa.disorientation_angle(a[:15].reshape(5, 3, 4), b[:5].reshape(5, 1, 4), "m-3m")
    want = theta[:15, :5].reshape(5, 3, 5)[np.arange(5), :, np.arange(5)]
    err, bound = cases.lost(got, want, slack[:15, :5].reshape(5, 3, 5)[np.arange(5), :, np.arange(5)])
    assert got.shape == (5, 3) and (err <= bound).all()

    class Holder:
        rotations = a[:4]

    class Orix:
        data = b[:4]

        class symmetry:
            name = "m-3m"

    assert np.array_equal(kpa.disorientation_angle(Holder(), Orix(), Orix.symmetry), kpa.disorientation_angle(a[:4], b[:4], "432"))
    assert np.array_equal(kpa.disorientation_angle(a[:4].astype(np.float32), b[:4], "432"),
                          kpa.disorientation_angle(a[:4].astype(np.float32).astype(np.float64), b[:4], "432"))
    f32 = kpa.disorientation_angle_outer(a[:7], b[:5], "432", dtype_out="float32")
    assert f32.dtype == np.float32
    assert np.array_equal(f32, kpa.disorientation_angle_outer(a[:7], b[:5], "432").astype(np.float32), equal_nan=True)
    assert np.array_equal(kpa.disorientation_angle_outer(a[:7], None, "432"), kpa.disorientation_angle_outer(a[:7], a[:7], "432"),
                          equal_nan=True)
    assert kpa.disorientation_angle(np.zeros((0, 4)), a[:1]).shape == (0,)


def test_plus_and_minus_q_give_the_same_bits():
    for g1, g2 in (("432", "432"), ("432", "622"), ("1", "1")):
        a, b = cases.pools(g1, g2)
        ref = kpa.disorientation_angle_outer(a, b, g1, g2)
        assert np.array_equal(kpa.disorientation_angle_outer(-a, b, g1, g2), ref, equal_nan=True)
        assert np.array_equal(kpa.disorientation_angle_outer(a, -b, g1, g2), ref, equal_nan=True)
    a, _ = cases.pools("622", "622")
    r, i = kpa.reduce_to_fundamental_zone(a, "622", True)
    r2, i2 = kpa.reduce_to_fundamental_zone(-a, "622", True)
    assert np.array_equal(r, r2, equal_nan=True) and np.array_equal(i, i2)


def test_refusals(monkeypatch):
    def no_context(*args, **kwargs):
        raise AssertionError("a context was opened")

    monkeypatch.setattr(_lib, "Context", no_context)
    q = np.tile([1.0, 0, 0, 0], (6, 1))
    for name in cases.REFUSED:
        for call in (lambda: kpa.disorientation_angle(q, q, name, device=0), lambda: kpa.disorientation_angle(q, q, "432", name),
                     lambda: kpa.disorientation_angle_outer(q, None, name, device=0),
                     lambda: kpa.reduce_to_fundamental_zone(q, name, device=0),
                     lambda: kpa.kernel_average_misorientation_map(q, name, (2, 3), device=0)):
            with pytest.raises(ValueError, match="pass the rotation group you want"):
                call()
    with pytest.raises(ValueError, match="last axis"):
        kpa.disorientation_angle(np.zeros((4, 3)), q, device=0)
    with pytest.raises(ValueError, match="last axis"):
        kpa.reduce_to_fundamental_zone(np.zeros(3), "1", device=0)
    with pytest.raises(ValueError, match="do not broadcast"):
        kpa.disorientation_angle(np.zeros((5, 3, 4)), np.zeros((5, 2, 4)), device=0)
    for dtype in ("float16", "int32", "complex128"):
        with pytest.raises(ValueError, match="float64 or float32"):
            kpa.disorientation_angle_outer(q, None, "1", dtype_out=dtype, device=0)
    with pytest.raises(ValueError, match="real dtype"):
        kpa.disorientation_angle(q.astype(complex), q)
    with pytest.raises(ValueError, match="6 rotations for a map"):
        kpa.kernel_average_misorientation_map(q, "1", (2, 2), device=0)
    with pytest.raises(ValueError, match="axes of the map"):
        kpa.kernel_average_misorientation_map(q, "1", (2, 3), window=Window("rectangular", (3,)), device=0)
    with pytest.raises(AssertionError, match="a context was opened"):
        kpa.disorientation_angle(q, q, "432", device=0)
    assert "disorientation_angle" in kpa.__all__ and kpa.orientations is orientations


# ---- wrong variants ---------------------------------------------------------------------------------------------------------
def variant(q1, q2, g1, g2, kind):
    """The float64 brute-force double loop with one thing wrong."""
    s1 = cases.ld_operations(g1)[0].astype(np.float64)
    s2 = cases.ld_operations(g2)[0].astype(np.float64)
    if kind == "one_sided":
        s1 = s1[:1]
    n1 = q1 / np.linalg.norm(q1, axis=1)[:, None]
    n2 = q2 / np.linalg.norm(q2, axis=1)[:, None]
    e1 = cases.ld_product(s1[:, None, :], n1[None])
    e2 = cases.ld_product(s2[:, None, :], n2[None])
    r = cases.ld_product(e2[None], (e1 * [1, -1, -1, -1])[:, None]).reshape(-1, n1.shape[0], 4)
    w = r[..., 0] if kind == "no_abs" else np.abs(r[..., 0])
    pick = w.argmax(axis=0)
    win = r[pick, np.arange(n1.shape[0])]
    if kind == "acos":
        return 2 * np.arccos(np.minimum(w.max(axis=0), 1.0))
    return 2 * np.arctan2(np.linalg.norm(win[:, 1:], axis=1), win[:, 0] if kind == "no_abs" else np.abs(win[:, 0]))


def test_wrong_variants_fall_outside_the_bound():
    valid = np.array([i for i in range(cases.POOL) if i not in (15, 16, 17)])
    # the right formula passes this very check ...
    for g1, g2 in (("1", "1"), ("432", "432"), ("432", "622"), ("222", "4")):
        a, b = cases.pools(g1, g2)
        theta, slack = (np.diag(v)[valid] for v in cases.outer_reference(g1, g2))
        err, bound = cases.lost(variant(a[valid], b[valid], g1, g2, "right"), theta, slack)
        assert (err <= bound).all(), (g1, g2)
    # ... 2 acos of the maximum fails at every angle <= 1e-6 (rows 5 ... 8 of the diagonal; 432: also row 13)
    for g in ("1", "432"):
        a, b = cases.pools(g, g)
        theta, slack = (np.diag(v) for v in cases.outer_reference(g, g))
        rows = np.array([5, 6, 7, 8] + ([13] if g != "1" else []))
        assert (theta[rows] <= 1.0001e-6).all()
        err, bound = cases.lost(variant(a[rows], b[rows], g, g, "acos"), theta[rows], slack[rows])
        print(g, "acos form: relative error", err / theta[rows].astype(np.float64))
        assert (err > bound).all()
    # ... one side's equivalents with two different groups fail
    for g1, g2 in cases.MIXED[:1] + cases.MIXED[2:]:
        a, b = cases.pools(g1, g2)
        theta, slack = (np.diag(v)[valid] for v in cases.outer_reference(g1, g2))
        err, bound = cases.lost(variant(a[valid], b[valid], g1, g2, "one_sided"), theta, slack)
        print(g1, g2, "one-sided: pairs outside the bound", int((err > bound).sum()), "of", len(valid))
        assert (err > bound).sum() >= len(valid) // 3
    # ... and so does the scalar part without its |.|
    for g in ("1", "3"):
        a, b = cases.pools(g, g)
        theta, slack = (np.diag(v)[valid] for v in cases.outer_reference(g, g))
        err, bound = cases.lost(variant(a[valid], b[valid], g, g, "no_abs"), theta, slack)
        print(g, "no |.|: pairs outside the bound", int((err > bound).sum()), "of", len(valid))
        assert (err > bound).sum() >= 1


# ---- zone reduction ----------------------------------------------------------------------------------------------------------
def check_reduction(got, index, q, group):
    """The two properties (in the closed zone, equivalent to the input) and, where the margin allows, the index."""
    want, want_index, gap = cases.restate_reduce(q, group)
    bad = want_index < 0
    assert np.isnan(got[bad]).all() and (index[bad] == -1).all() and not np.isnan(got[~bad]).any()
    g, w, wi, gp = got[~bad], want[~bad], want_index[~bad], gap[~bad]
    assert sampling.in_fundamental_zone(g, sampling.fundamental_zone_faces(group)).all() and (g[:, 0] >= 0).all()
    zero, _ = cases.restate_pairs(g, q[~bad], group, group)  # equivalent to the input: disorientation 0
    assert (zero.astype(np.float64) <= cases.angle_bound(0.0)).all()
    clear = gp > 2 * cases.EQUIV * U
    assert np.array_equal(index[~bad][clear], wi[clear])
    sign = np.where((np.abs(w[:, :1]) < 1e-15) & ((g * w).sum(axis=1, keepdims=True) < 0), -1, 1)  # a half turn's sign
    assert (np.abs(g - (w * sign).astype(np.float64))[clear] <= cases.EQUIV * U + 1e-17).all()
    return int(clear.sum())


@pytest.mark.parametrize("group", cases.GROUPS)
def test_host_reduction(group):
    a, b = cases.pools(group, group)
    q = np.concatenate([a, b])
    got, index = kpa.reduce_to_fundamental_zone(q, group, True)
    assert got.shape == q.shape and index.dtype == np.int32
    assert check_reduction(got, index, q, group) >= cases.POOL
    assert np.array_equal(kpa.reduce_to_fundamental_zone(q.reshape(2, -1, 4), group), got.reshape(2, -1, 4), equal_nan=True)


def test_zone_samples_reduce_to_themselves():
    for group in ("432", "622", "32", "1"):
        q = kpa.get_sample_fundamental(point_group=group, semi_edge_steps=7)
        f = sampling.fundamental_zone_faces(group)
        inner = np.ones(len(q), dtype=bool)
        for a0, a1, a2, t in f:
            inner &= np.abs(q[:, 1] * a0 + q[:, 2] * a1 + q[:, 3] * a2) < t * q[:, 0] - sampling.FACE_SLACK
        inner &= q[:, 0] > sampling.FACE_SLACK
        got, index = kpa.reduce_to_fundamental_zone(q[inner], group, True)
        assert inner.sum() > 10 and (index == 0).all() and np.abs(got - q[inner]).max() <= 4 * U


# ---- KAM -----------------------------------------------------------------------------------------------------------------------
KAM_WINDOWS = {"default": None, "circular5": Window("circular", (5, 5)), "rectangular3": Window("rectangular", (3, 3)),
               "rectangular35": Window("rectangular", (3, 5)), "gaussian": Window("gaussian", (3, 3), std=1),
               "even": Window("rectangular", (2, 4)),
               "custom": np.array([[1, 0, 1], [0, 1, 0], [0, 1, 1]], dtype=bool)}
KAM_MAPS = ((1, 1), (1, 5), (3, 3), (4, 7))


def kam_case(nav, group="432"):
    a, b = cases.pools(group, group)
    q = np.concatenate([a[:14], b[:14]])[:nav[0] * nav[1]].copy()  # valid rows only; neighbours repeat orientations
    return q


def window_2d(window, nav):
    w = np.asarray(Window("circular", (3, 3)) if window is None else window)
    return (w != 0).reshape(w.shape + (1,) * (2 - w.ndim))


@pytest.mark.parametrize("name", sorted(KAM_WINDOWS))
@pytest.mark.parametrize("nav", KAM_MAPS)
def test_host_kam_windows(name, nav):
    q = kam_case(nav)
    off = cases.window_offsets(window_2d(KAM_WINDOWS[name], nav))
    want, bound, _ = cases.restate_kam(q, nav[0], nav[1], "432", off)
    got = kpa.kernel_average_misorientation_map(q, "m-3m", nav, KAM_WINDOWS[name])
    assert got.shape == nav and np.array_equal(np.isnan(got), np.isnan(want.astype(np.float64)))
    ok = ~np.isnan(got)
    assert (np.abs(got[ok].astype(cases.L) - want[ok]).astype(np.float64) <= bound[ok]).all()
    if nav == (1, 1):
        assert np.isnan(got).all()


def test_host_kam_one_axis_mask_and_limit():
    q = kam_case((1, 6))
    want, bound, _ = cases.restate_kam(q, 6, 1, "432", [(-1, 0), (1, 0)])
    got = kpa.kernel_average_misorientation_map(q, "432", (6,))
    assert got.shape == (6,) and (np.abs(got.astype(cases.L) - want[:, 0]).astype(np.float64) <= bound[:, 0]).all()
    mask = np.array([1, 1, 0, 1, 0, 1], dtype=bool)
    limit = 0.6
    want, bound, ambiguous = cases.restate_kam(q, 6, 1, "432", [(-1, 0), (1, 0)], mask, limit)
    assert not ambiguous
    got = kpa.kernel_average_misorientation_map(q.reshape(6, 4), "432", None, None, limit, mask)
    assert np.array_equal(np.isnan(got), np.isnan(want[:, 0].astype(np.float64))) and np.isnan(got[[2, 3, 4]]).all()
    ok = ~np.isnan(got)
    assert (np.abs(got[ok].astype(cases.L) - want[ok, 0]).astype(np.float64) <= bound[ok, 0]).all()
    deg = kpa.kernel_average_misorientation_map(q.reshape(6, 4), "432", None, None, np.rad2deg(limit), mask, True)
    assert np.allclose(deg[ok], np.rad2deg(got[ok]), rtol=1e-15, atol=0)


# ---- csrc/orientations_plan.h with the host compiler ----------------------------------------------------------------------------
PLAN_PROBE = r"""
#include "orientations_plan.h"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
using namespace kpdi;
static bool read_ops(OriOps *o) {
  *o = OriOps{};
  if (scanf("%d", &o->n) != 1) return false;
  for (int s = 0; s < o->n; ++s)
    for (int k = 0; k < 4; ++k)
      if (scanf("%lf", &o->q[s][k]) != 1) return false;
  return true;
}
int main() {
  printf("const %d %d %d %d %d %d\n", ORI_MAX_OPS, ORI_THREADS, ORI_TILE_I, ORI_TILE_J, ORI_MFMA, ORI_MAX_DIMS);
  const long long plans[][5] = {{1, 1, 8, 1 << 20, 0}, {33, 31, 8, 1 << 20, 0}, {33, 31, 4, 1 << 20, 3}, {1000, 1000, 8, 1000 * 8 * 100, 0},
                                {1000, 1000, 8, 1000 * 8 * 20, 0}, {70000, 70000, 8, 1LL << 62, 0}, {5, 7, 8, 10, 0}, {0, 7, 8, 100, 0},
                                {5, 7, 2, 1000, 0}, {1LL << 40, 33, 4, 1LL << 62, 0}};
  for (const auto &a : plans) {
    const OriOuterPlan p = ori_outer_plan(a[0], a[1], (int)a[2], (size_t)a[3], a[4]);
    printf("plan %d %lld %lld %lld %lld %lld %zu\n", p.ok, (long long)p.pass_rows, (long long)p.n_passes, (long long)p.tail_rows,
           (long long)p.tiles_j, (long long)p.pass_tiles, p.pass_bytes);
  }
  for (long long t : {0LL, 1LL, 2187LL, 2188LL, 4785155LL}) {
    int64_t r, c;
    ori_tile_origin(t, 2188, &r, &c);  // 70000 columns
    printf("tile %lld %lld %lld %lld\n", t, (long long)r, (long long)c, (long long)ori_out_index(r, c, 70000));
  }
  printf("index %lld %lld\n", (long long)ori_out_index(69999, 69999, 70000), (long long)ori_blocks(257));
  OriShape s{};
  s.nd = 3;
  const int64_t dim[3] = {5, 3, 2}, st1[3] = {6, 2, 1}, st2[3] = {1, 0, 0};
  for (int d = 0; d < 3; ++d) s.dim[d] = dim[d], s.stride1[d] = st1[d], s.stride2[d] = st2[d];
  for (long long p : {0LL, 1LL, 5LL, 29LL}) {
    int64_t r1, r2;
    ori_pair_rows(p, s, &r1, &r2);
    printf("rows %lld %lld %lld\n", p, (long long)r1, (long long)r2);
  }
  OriOps o1, o2;
  int n;
  while (read_ops(&o1) && read_ops(&o2) && scanf("%d", &n) == 1) {
    for (int i = 0; i < n; ++i) {
      double a[4], b[4], g1[4], g2[4], r[4];
      for (int k = 0; k < 4; ++k) if (scanf("%lf", &a[k]) != 1) return 1;
      for (int k = 0; k < 4; ++k) if (scanf("%lf", &b[k]) != 1) return 1;
      ori_normalise(a, g1);
      ori_normalise(b, g2);
      int win = -1;
      const double w = ori_pair_angle(g1, g2, o1, o2, &win);
      const int at = ori_reduce(b, o2, r);
      printf("pair %.17g %d %d %.17g %.17g %.17g %.17g\n", w, win, at, r[0], r[1], r[2], r[3]);
    }
  }
  return 0;
}
"""

PROBE_PAIRS = (("432", "432"), ("432", "622"), ("32", "1"), ("6", "6"))


def fmt(values):
    return " ".join("nan" if np.isnan(v) else "inf" if np.isinf(v) else repr(float(v)) for v in np.ravel(values))


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("oriplan")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    text = ""
    for g1, g2 in PROBE_PAIRS:
        ops1, ops2 = orientations._operations(g1, g2)
        a, b = cases.pools(g1, g2)
        text += f"{len(ops1)} {fmt(ops1)} {len(ops2)} {fmt(ops2)} {len(a)}\n"
        text += "".join(f"{fmt(x)} {fmt(y)}\n" for x, y in zip(a, b))
    return subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.strip().split("\n")


def test_plan_arithmetic(plan_lines):
    consts = [int(v) for v in plan_lines[0].split()[1:]]
    hc = cases.header_constants()
    assert consts == [hc[k] for k in ("ORI_MAX_OPS", "ORI_THREADS", "ORI_TILE_I", "ORI_TILE_J", "ORI_MFMA", "ORI_MAX_DIMS")]
    assert hc["ORI_MAX_OPS"] == _lib.ORIENTATION_MAX_OPS == 24 and hc["ORI_MAX_DIMS"] == _lib.ORIENTATION_MAX_DIMS
    assert hc["ORI_TILE_I"] % hc["ORI_MFMA"] == 0 and hc["ORI_TILE_J"] % hc["ORI_MFMA"] == 0
    assert (hc["ORI_TILE_I"] // hc["ORI_MFMA"]) * (hc["ORI_TILE_J"] // hc["ORI_MFMA"]) * 64 == hc["ORI_THREADS"]  # a wave per block
    assert hc["ORI_TILE_I"] * hc["ORI_TILE_J"] == 4 * hc["ORI_THREADS"] and cases.POOL == hc["ORI_TILE_I"] + 2
    ti, tj = hc["ORI_TILE_I"], hc["ORI_TILE_J"]
    plans = [[int(v) for v in l.split()[1:]] for l in plan_lines if l.startswith("plan")]
    # ok, rows of a pass, passes, rows of the last, tiles along the columns, workgroups of a pass, bytes of a pass
    assert plans[0] == [1, 1, 1, 1, 1, 1, 8]
    assert plans[1] == [1, 33, 1, 33, 1, 2, 33 * 31 * 8]                      # everything fits: one pass, a ragged tile row
    assert plans[2] == [1, 3, 11, 3, 1, 1, 3 * 31 * 4]                        # forced passes
    assert plans[3] == [1, 96, 11, 1000 - 10 * 96, -(-1000 // tj), 3 * -(-1000 // tj), 96 * 8000]  # whole tile rows
    assert plans[4] == [1, 20, 50, 20, -(-1000 // tj), -(-1000 // tj), 20 * 8000]  # fewer rows than a tile: as many as fit
    assert plans[5][:3] == [1, 70000, 1] and plans[5][5] == 2188 * 2188 and plans[5][6] == 70000 * 70000 * 8 > 2**32
    assert plans[6][0] == 0 and plans[7][0] == 0 and plans[8][0] == 0          # not one row fits; no rows; no such dtype
    assert plans[9][0] == 1 and plans[9][5] <= 2**31 - 1 and plans[9][1] % ti == 0 and plans[9][2] > 1  # a launch's grid limits a pass
    tiles = [[int(v) for v in l.split()[1:]] for l in plan_lines if l.startswith("tile")]
    assert tiles[0] == [0, 0, 0, 0] and tiles[1] == [1, 0, tj, tj] and tiles[2] == [2187, 0, 2187 * tj, 2187 * tj]
    assert tiles[3] == [2188, ti, 0, ti * 70000]
    assert tiles[4] == [4785155, 2186 * ti, 2187 * tj, 2186 * ti * 70000 + 2187 * tj] and tiles[4][3] > 2**32  # a 64-bit index
    index = [int(v) for v in [l for l in plan_lines if l.startswith("index")][0].split()[1:]]
    assert index == [70000 * 70000 - 1, 2]
    rows = [[int(v) for v in l.split()[1:]] for l in plan_lines if l.startswith("rows")]
    assert rows == [[0, 0, 0], [1, 1, 0], [5, 5 // 2 % 3 * 2 + 1, 0], [29, 4 * 6 + 2 * 2 + 1, 4]]


def test_header_pairs_and_reduction_stay_inside_the_bound(plan_lines):
    lines = [l.split()[1:] for l in plan_lines if l.startswith("pair")]
    assert len(lines) == len(PROBE_PAIRS) * cases.POOL
    for k, (g1, g2) in enumerate(PROBE_PAIRS):
        part = lines[k * cases.POOL:(k + 1) * cases.POOL]
        a, b = cases.pools(g1, g2)
        theta, slack = (np.diag(v) for v in cases.outer_reference(g1, g2))
        err, bound = cases.lost(np.array([float(p[0]) for p in part]), theta, slack)
        assert (err <= bound).all(), (g1, g2)
        got = np.array([[float(v) for v in p[3:]] for p in part])
        check_reduction(got, np.array([int(p[2]) for p in part]), np.array(b), g2)
