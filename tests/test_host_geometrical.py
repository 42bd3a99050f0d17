"""Geometrical simulations, the part that needs no GPU: the NumPy restatement of tests/_geometrical_cases.py against the
reference's own classes (tests/golden/geometrical.npz, tools/gen_geometrical_golden.py), three wrong restatements that
must be noticed, the share of pairs left out of a comparison, csrc/geometrical_plan.h compiled with the host compiler
(geometry of both passes, the per-point table), the integer zone-axis reduction, signatures and refusals."""

import inspect
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _geometrical_cases as cases
import kikuchipy_amd as kpa
from conftest import load_golden
from kikuchipy_amd import simulations

ROOT = cases.ROOT
GOLDEN = load_golden("geometrical.npz")
CASES = cases.cases()
GOLDEN_CASES = [c for c in CASES if c["golden"]]
_SIM = {}


def simulated(case):
    if case["name"] not in _SIM:
        _SIM[case["name"]] = cases.simulate(case)
    return _SIM[case["name"]]


def test_inputs_regenerate_bit_for_bit():
    for case in CASES:
        for name in ("hkl", "basis", "rotations", "pc"):
            assert np.array_equal(GOLDEN[cases.key(case, "in_" + name)], case[name]), (case["name"], name)
        assert json.loads(str(GOLDEN[cases.key(case, "in_det")])) == json.loads(json.dumps(case["det"]))
    assert "KikuchiPatternLine" in str(GOLDEN["made_by"])


@pytest.mark.parametrize("name", [c["name"] for c in GOLDEN_CASES])
def test_restatement_equals_the_reference(name):
    case = [c for c in CASES if c["name"] == name][0]
    sim = simulated(case)
    want = {k: GOLDEN[cases.key(case, k)] for k in ("keep", "uvw", "line_in", "line_within", "zone_in", "zone_within",
                                                    "hesse_distance", "hesse_alpha", "r_gnomonic", "line_gn", "line_px",
                                                    "zone_gn", "zone_px")}
    for k in ("keep", "uvw", "line_in", "line_within", "zone_in", "zone_within"):
        assert np.array_equal(sim[k], want[k]), k
    lines_out, zones_out = cases.left_out(case, sim)
    atol, tol_x, tol_y = cases.tolerances(sim)
    line_tol = np.stack([tol_x, tol_y, tol_x, tol_y], axis=-1)
    zone_tol = np.stack([tol_x, tol_y], axis=-1)
    for k, out, tol in (("line_gn", lines_out, atol), ("line_px", lines_out, line_tol), ("zone_gn", zones_out, atol),
                        ("zone_px", zones_out, zone_tol)):
        ok, worst = cases.compare(sim[k], want[k], out, tol)
        print(name, k, "largest error / tolerance:", worst)
        assert ok, k
    for k, out in (("hesse_distance", lines_out), ("hesse_alpha", lines_out), ("r_gnomonic", zones_out)):
        ok, _ = cases.compare(sim[k][..., np.newaxis], want[k][..., np.newaxis], out, atol)
        assert ok, k


@pytest.mark.parametrize("wrong", ["z_ge", "not_widened", "y_not_negated"])
def test_a_wrong_restatement_differs_from_the_fixture(wrong):
    failed = []
    for case in GOLDEN_CASES:
        sim = cases.simulate(case, wrong)
        for k in ("keep", "uvw", "line_in", "zone_in", "line_px", "zone_px"):
            want = GOLDEN[cases.key(case, k)]
            if sim[k].shape != want.shape or not np.allclose(sim[k], want, rtol=0, atol=1e-9, equal_nan=True):
                failed.append((case["name"], k))
    print(wrong, failed)
    assert failed


def test_few_pairs_are_left_out_and_none_at_one_point():
    for case in CASES:
        sim = simulated(case)
        lines_out, zones_out = cases.left_out(case, sim)
        pairs = lines_out.size + zones_out.size
        share = (lines_out.sum() + zones_out.sum()) / pairs
        print(case["name"], "left out:", int(lines_out.sum()), "lines,", int(zones_out.sum()), "zone axes of", pairs)
        assert share <= cases.LEFT_OUT_CAP
        if lines_out.shape[0] == 1:
            assert share == 0


def test_cases_reach_what_they_claim():
    by = {c["name"]: c for c in CASES}
    assert simulated(by["one_point_one_reflector"])["keep"].tolist() == [True]
    assert simulated(by["one_point_one_reflector"])["uvw"].shape == (0, 3)
    keep = simulated(by["one_point_111_family"])["keep"]
    assert keep.size == 8 and 0 < keep.sum() < 8  # some members have z <= 0 at the one orientation
    big = simulated(by["points65_reflectors257"])
    assert by["points65_reflectors257"]["hkl"].shape == (257, 3) and big["line_in"].shape[0] == 65
    hand = simulated(by["handmade_z0"])
    assert hand["keep"][:2].all() and np.array_equal(hand["hkl_d"][0, :2, 2], [0.0, -5e-6])  # exactly
    assert hand["line_in"][0, :2].tolist() == [False, False] and hand["line_within"][0, :2].all()
    assert np.isfinite(hand["line_px"][0, :2]).all()
    tri = by["triclinic_2x2"]["basis"]
    lengths = np.sqrt(np.sum(tri**2, axis=1))
    assert len(set(np.round(lengths, 6))) == 3 and np.all(np.abs(tri @ tri.T - np.diag(lengths**2)) [~np.eye(3, dtype=bool)] > 1e-4)
    for case in CASES:  # every feature kind is exercised: present, NaN, and (in maps) varying between points
        sim = simulated(case)
        if sim["line_in"].shape[0] > 1:
            assert np.isnan(sim["line_gn"]).any() and np.isfinite(sim["line_gn"]).any()
            assert np.isnan(sim["zone_px"]).any() and np.isfinite(sim["zone_px"]).any()


# ---- csrc/geometrical_plan.h on the host --------------------------------------------------------------------------------
PLAN_PROGRAM = r"""
#include "geometrical_plan.h"
#include <cstdio>
#include <initializer_list>
using namespace kpdi;
int main() {
  const long ms[] = {1, 255, 256, 257}, ns[] = {1, 63, 64, 65};
  for (long m : ms) for (long n : ns) for (int force : {0, 16}) {
    GeoVisPlan p = geo_visibility_plan(m, n, force);
    printf("vis %ld %ld %d %d %d %d %d %ld %d %d %zu\n", m, n, force, p.ok, p.tiles, p.last_features, p.chunk, (long)p.n_chunks, p.tail,
           p.grid_y, p.lds_bytes);
    GeoCoordPlan c = geo_coord_plan(m, 3 * m, n, (size_t)1 << 30, force);
    printf("coord %ld %ld %d %d %d %d %d %zu %ld %ld %ld\n", m, n, force, c.ok, c.line_tiles, c.zone_tiles, c.tiles, c.bytes_per_point,
           (long)c.points, (long)c.n_passes, (long)c.tail);
  }
  GeoVisPlan many = geo_visibility_plan(10, 100000, 0);
  printf("many %ld %d\n", (long)many.n_chunks, many.grid_y);
  GeoCoordPlan small = geo_coord_plan(338, 5000, 40000, (size_t)64 << 20, 0), none = geo_coord_plan(1, 0, 1, 0, 0);
  printf("small %ld %ld %ld %zu\n", (long)small.points, (long)small.n_passes, (long)small.tail, small.bytes_per_point);
  printf("none %d %d %d %ld\n", none.ok, none.zone_tiles, none.tiles, (long)none.points);
  printf("refused %d %d %d %d\n", geo_visibility_plan(0, 1).ok, geo_visibility_plan(1, 0).ok, geo_coord_plan(0, 0, 1, 1).ok,
         geo_coord_plan(1, -1, 1, 1).ok);
  const double q[4] = {0.5, -0.5, 0.1, 0.7}, us[9] = {0, 0, 1, 1, 0, 0, 0, 1, 0}, as[9] = {2, 0.5, 0, 0, 3, 0.25, 0, 0, 4},
               ad[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pc[8] = {-1, 1, -2, 2, 0.5, 0.25, 0.01, 0.02};
  double e[GEO_ENTRY_DOUBLES];
  geo_point_entry(q, us, as, ad, pc, e);
  printf("entry");
  for (int i = 0; i < GEO_ENTRY_DOUBLES; ++i) printf(" %.17g", e[i]);
  printf("\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("geometrical_plan")
    src, exe = tmp / "plan.cpp", tmp / "plan"
    src.write_text(PLAN_PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")


def test_plan_geometry_of_both_passes(plan_lines):
    rows = [line.split() for line in plan_lines]
    vis = {(int(r[1]), int(r[2]), int(r[3])): [int(v) for v in r[4:]] for r in rows if r[0] == "vis"}
    coord = {(int(r[1]), int(r[2]), int(r[3])): [int(v) for v in r[4:]] for r in rows if r[0] == "coord"}
    assert len(vis) == 32 and len(coord) == 32
    for (m, n, force), (ok, tiles, last, chunk, n_chunks, tail, grid_y, lds) in vis.items():
        want_chunk = force or 64
        assert ok == 1 and tiles == -(-m // 256) and last == (m % 256 or 256) and chunk == want_chunk
        assert n_chunks == -(-n // want_chunk) and tail == (n % want_chunk or want_chunk) and grid_y == min(n_chunks, 256)
        assert (tiles - 1) * 256 + last == m and (n_chunks - 1) * chunk + tail == n  # every feature and point, once
        assert lds == 64 * 16 * 8 <= 160 * 1024
    for (m, n, force), (ok, lt, zt, tiles, per_point, points, passes, tail) in coord.items():
        z = 3 * m
        assert ok == 1 and lt == -(-m // 256) and zt == -(-z // 256) and tiles == lt + zt
        assert per_point == m * 65 + z * 33
        assert points == (min(force, n) if force else n) and (passes - 1) * points + tail == n and 1 <= tail <= points
    assert plan_lines[-5].split() == ["many", "1563", "256"]
    small = [int(v) for v in plan_lines[-4].split()[1:]]
    assert small[3] == 338 * 65 + 5000 * 33 and small[0] == (64 << 20) // small[3] and (small[1] - 1) * small[0] + small[2] == 40000
    assert plan_lines[-3].split() == ["none", "1", "0", "1", "1"]
    assert plan_lines[-2].split() == ["refused", "0", "0", "0", "0"]


def test_point_entry_equals_numpy(plan_lines):
    e = np.array([float(v) for v in plan_lines[-1].split()[1:]])
    q = np.array([[0.5, -0.5, 0.1, 0.7]])
    us = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=float)
    a_star = np.array([[2, 0.5, 0], [0, 3, 0.25], [0, 0, 4]])
    u_os = cases.to_matrix(q)[0] @ us
    assert np.allclose(e[:9].reshape(3, 3), a_star @ u_os, rtol=0, atol=1e-14)
    assert np.allclose(e[9:18].reshape(3, 3), u_os, rtol=0, atol=1e-14)
    assert np.allclose(simulations.rotation_matrices(q)[0], cases.to_matrix(q)[0], rtol=0, atol=1e-15)
    assert e[18:26].tolist() == [-1, 1, -2, 2, 0.5, 0.25, 0.01, 0.02] and not e[26:].any()


# ---- the Python surface --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_point_one_reflector", "one_point_111_family", "map3x3_one_pc", "points65_reflectors257"])
def test_zone_axes_equal_a_brute_force_unique(name):
    case = [c for c in CASES if c["name"] == name][0]
    hkl = case["hkl"].astype(np.int64)
    got = simulations.zone_axes_from_reflectors(hkl)
    assert got.dtype == np.float64 and np.array_equal(got, cases.zone_axes_brute_force(hkl))
    if got.shape[0]:
        pairs = np.cross(hkl[:, None], hkl[None]).reshape(-1, 3)
        pairs = pairs[np.any(pairs != 0, axis=1)]
        reduced = np.array([row // np.gcd.reduce(np.abs(row)) for row in pairs])
        assert np.array_equal(got, np.unique(reduced, axis=0))
        assert np.array_equal(got, -got[::-1])  # [uvw] and [-u -v -w] are both there


def test_pc_table_equals_the_restatement():
    for case in CASES:
        det = cases.detector(case)
        table = simulations._geometrical_pc_table(det)
        x_range, y_range, x_scale, y_scale = cases.widened_ranges(det)
        assert np.array_equal(table[:, :2], x_range) and np.array_equal(table[:, 2:4], y_range)
        assert np.array_equal(table[:, 6], x_scale) and np.array_equal(table[:, 7], y_scale)
        pc = det.pc_flattened
        assert np.array_equal(table[:, 4], pc[:, 0] / pc[:, 2] * det.aspect_ratio) and np.array_equal(table[:, 5], pc[:, 1] / pc[:, 2])


def test_signatures_equal_the_reference():
    table = json.loads(str(GOLDEN["signatures"]))
    sim = kpa.GeometricalKikuchiPatternSimulation
    ours = {"KikuchiPatternSimulator.on_detector": kpa.KikuchiPatternSimulator.on_detector,
            "GeometricalKikuchiPatternSimulation.lines_coordinates": sim.lines_coordinates,
            "GeometricalKikuchiPatternSimulation.zone_axes_coordinates": sim.zone_axes_coordinates,
            "GeometricalKikuchiPatternSimulation.as_collections": sim.as_collections,
            "GeometricalKikuchiPatternSimulation.as_markers": sim.as_markers,
            "GeometricalKikuchiPatternSimulation.plot": sim.plot}
    assert sorted(table) == sorted(ours)
    assert table["GeometricalKikuchiPatternSimulation.lines_coordinates"] == [["index", None], ["coordinates", "pixel"],
                                                                              ["exclude_nan", True]]
    for name, fn in ours.items():
        params = list(inspect.signature(fn).parameters.values())[1:]
        positional = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert [[p.name, "<required>" if p.default is p.empty else p.default] for p in positional] == table[name], name
        for p in params:  # what this package adds can only be given by keyword, and never has to be
            if p not in positional:
                assert p.kind == p.KEYWORD_ONLY and p.default is not p.empty, (name, p.name)
    assert "GeometricalKikuchiPatternSimulation" in kpa.__all__


def test_reflectors_basis_and_indexing():
    ref = kpa.Reflectors([[1, 1, 1], [2, 0, 0], [0, 2, 0], [2, 2, 0]], [0.1, 0.2, 0.3, 0.4], [1, 2j, 3, 4],
                         reciprocal_basis=cases.TRICLINIC, phase_name="x")
    assert np.allclose(ref.direct_basis @ ref.reciprocal_basis.T, np.eye(3), rtol=0, atol=1e-14)
    for key, rows in ((np.array([True, False, True, False]), [0, 2]), ([3, 1], [3, 1]), (slice(1, 3), [1, 2]), (2, [2])):
        sub = ref[key]
        assert isinstance(sub, kpa.Reflectors) and np.array_equal(sub.hkl, ref.hkl[rows]) and sub.phase_name == "x"
        assert np.array_equal(sub.theta, ref.theta[rows]) and np.array_equal(sub.structure_factor, ref.structure_factor[rows])
        assert np.array_equal(sub.reciprocal_basis, ref.reciprocal_basis) and sub.reciprocal_basis is not ref.reciprocal_basis


def test_refused_calls_and_their_texts():
    sim = kpa.KikuchiPatternSimulator(kpa.Reflectors([[1, 1, 1], [2, 0, 0]], None))
    det9 = kpa.EBSDDetector(shape=(60, 60), pc=np.full((3, 3, 3), 0.5))
    rot = cases.random_rotations(0, (3, 3))
    unused = object()  # refused before the context is touched
    with pytest.raises(ValueError, match=r"`detector.navigation_shape` is not \(1,\) or equal to `rotations.shape`"):
        sim.on_detector(det9, rot.reshape(9, 4), context=unused)
    with pytest.raises(ValueError, match=r"`detector.navigation_shape` is not \(1,\) or equal to `rotations.shape`"):
        sim.on_detector(det9, rot[:2], context=unused)
    with pytest.raises(ValueError, match=r"rotations of shape \(4,\)"):
        sim.on_detector(det9, rot[0, 0], context=unused)
    with pytest.raises(ValueError, match=r"rotations of shape \(3, 3, 3\)"):
        sim.on_detector(det9, rot[..., :3], context=unused)
    half = kpa.KikuchiPatternSimulator(kpa.Reflectors([[1, 0.5, 1]], None))
    with pytest.raises(ValueError, match="integer Miller indices"):
        half.on_detector(det9, rot, context=unused)
    assert simulations.parse_coordinate_format("pixel") == "pixel" and simulations.parse_coordinate_format("gnomonic") == "gnomonic"
    with pytest.warns(Warning, match="Pass 'pixel' instead. Passing 'detector' is deprecated"):
        assert simulations.parse_coordinate_format("detector") == "pixel"
    with pytest.raises(ValueError, match="Unknown coordinate format 'lambert'. Expected 'pixel' or 'gnomonic'."):
        simulations.parse_coordinate_format("lambert")


def test_simulation_object_without_a_gpu(capsys):
    """The holder's indexing, NaN exclusion, copies, repr and refused plotting, fed with the restatement's arrays."""
    case = [c for c in CASES if c["name"] == "map3x3_nine_pcs"][0]
    s = simulated(case)
    nav = (3, 3)
    det = cases.detector(case)
    ref = kpa.Reflectors(case["hkl"], None)[s["keep"]]
    chain = (case["rotations"].reshape(-1, 4), det.detector_to_sample, case["basis"], np.linalg.inv(case["basis"].T))
    lines = simulations.KikuchiPatternLine(ref.hkl, chain, nav, s["line_in"], s["line_gn"], s["r_max"])
    zones = simulations.KikuchiPatternZoneAxis(s["uvw"], chain, nav, s["zone_in"], s["zone_gn"], s["r_max"])
    sim = kpa.GeometricalKikuchiPatternSimulation(det, case["rotations"], ref, lines, zones, s["line_px"].reshape(nav + (-1, 4)),
                                                  s["zone_px"].reshape(nav + (-1, 2)))
    assert sim.navigation_shape == nav and sim.ndim == 2 and sim.reflectors.size == s["keep"].sum()
    assert repr(sim).startswith("GeometricalKikuchiPatternSimulation (3, 3):\nReflectors (")
    assert np.array_equal(sim.zone_axes, s["uvw"]) and sim.detector is not det
    full = sim.lines_coordinates((1, 2), exclude_nan=False)
    assert np.array_equal(full, s["line_px"][5], equal_nan=True)
    assert np.array_equal(sim.lines_coordinates(), s["line_px"][0][~np.isnan(s["line_px"][0]).any(axis=-1)])
    assert np.array_equal(sim.zone_axes_coordinates((2, 0), "gnomonic", False), s["zone_gn"][6], equal_nan=True)
    got = sim.zone_axes_coordinates((2, 0))
    assert got.shape[1] == 2 and not np.isnan(got).any() and got.shape[0] == (~np.isnan(s["zone_px"][6]).any(axis=-1)).sum()
    full[:] = 0  # a copy
    assert np.isnan(sim.lines_coordinates((1, 2), exclude_nan=False)).any()
    # the scalar features, formed from the vectors when asked for, against the reference's
    n = 9
    for feature, name, want in ((sim.lines, "hesse_distance", s["hesse_distance"]), (sim.lines, "hesse_alpha", s["hesse_alpha"]),
                                (sim.zone_axes_features, "r_gnomonic", s["r_gnomonic"])):
        got = getattr(feature, name).reshape(n, -1)
        assert np.allclose(got, want, rtol=0, atol=1e-10 * s["r_max"], equal_nan=True), name
    assert np.array_equal(sim.lines.within_r_gnomonic.reshape(n, -1), s["line_within"])
    assert np.array_equal(sim.zone_axes_features.within_r_gnomonic.reshape(n, -1), s["zone_within"])
    assert np.array_equal(sim.lines.in_pattern.reshape(n, -1), s["line_in"])
    assert sim.lines.plane_trace_coordinates.shape == nav + (int(s["keep"].sum()), 4)
    assert sim.zone_axes_features.x_gnomonic.shape == sim.zone_axes_features.y_gnomonic.shape == nav + (s["uvw"].shape[0],)
    for name in ("as_collections", "as_markers", "plot"):
        with pytest.raises(NotImplementedError, match="lines_coordinates.*zone_axes_coordinates"):
            getattr(sim, name)()
    assert capsys.readouterr().out == ""
