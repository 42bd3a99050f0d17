"""The yardstick of tests/test_gpu_projection_probes.py, checked without a GPU: the long-double restatement of the
projection (tests/_projection_cases.py) against the project's existing references, the float64 rounding floor it
measures them with, and the comparison helpers against mutants of the restatement - every one a mistake that
csrc/projection.h or csrc/project.hip could make and that tests/test_gpu_projection.py would let through."""

import contextlib
import io

import numpy as np
import pytest

import _projection_cases as pc
from conftest import load_golden
from oracle import kpdi_oracle as ko

pytestmark = pytest.mark.skipif(not pc.HAVE_LD, reason="np.longdouble has no 64-bit mantissa here")


def test_restatement_agrees_with_the_oracle():
    """float64 + libm against long double on the `generic` class: random master pattern, identity and the rotation
    set, within the tolerance the GPU tests use."""
    p = pc.generic()[0]
    up, lo = pc.masters("random", 401)
    q = pc.rotation_set()
    assert not pc.near_equator(q, p).any()
    got = ko.project_patterns(q, p, up, lo, dtype_out=np.float64)
    pc.check_values(got, pc.project_ld(q, p, up, lo), "generic", 401, "oracle")


def test_restatement_agrees_with_the_golden_patterns():
    """The reference's own float32 output (f32mp_f32: float32 master pattern, 60 x 60 detector, eight rotations) is
    the long-double value rounded once: half a float32 ulp, plus the float64 evaluation's own error (below 1e-9 on
    intensities up to 255)."""
    g = load_golden("projection.npz")
    want = g["f32mp_f32__patterns"]
    ld = pc.project_ld(g["rot8"], g["det60__dc"], g["mp_upper"].astype(np.float32), g["mp_lower"].astype(np.float32))
    assert want.dtype == np.float32 and want.shape == ld.shape
    assert (np.abs(want.astype(pc.LD) - ld) <= 0.5 * np.spacing(np.abs(want)).astype(pc.LD) + 1e-9).all()


@pytest.mark.parametrize("name", pc.CLASS_NAMES)
def test_floor_table_holds(name):
    for npx in pc.NPX:
        measured = pc.measure_floor(name, npx)
        print(f"{name} npx={npx}: measured {measured:.2e}, table {pc.FLOOR[name][npx]:.2e}")
        assert measured <= pc.FLOOR[name][npx]


@pytest.mark.parametrize("case", pc.NEAR_POLE_CASES)
def test_directions_near_the_pole(case):
    """A few rotated directions of the GPU tests (six pixels of the 70 x 90 varying-PC detector, five probes of the
    path-boundary test) come closer to a pole than any generic probe.  There float64 + libm itself is more than twice
    the generic floor off, which it is nowhere else (the floor was measured without a rotation; one costs less than as
    much again), so they have a floor of their own, measured at those very directions; it holds."""
    q, probes, polar = pc.near_pole_case(case)
    assert polar.sum(axis=1).tolist() == ([0, 0, 6] if case == "varying_pc_near_pole" else [0, 4, 1])
    assert not pc.varying_pc_case((5, 7))[4].any()
    worst_polar, worst_rest = pc.measure_near_pole(case)
    floor = pc.FLOOR["generic"][401]
    print(f"{case}: float64 + libm {worst_polar:.2e} near the pole (table {pc.FLOOR[case][401]:.2e}), {worst_rest:.2e} elsewhere, generic floor {floor:.2e}")
    assert worst_polar <= pc.FLOOR[case][401]
    assert worst_polar > 2 * floor >= worst_rest


def test_lattice_floor_holds_at_every_node():
    """The `lattice` class has 9 x 9 of the 401 x 401 nodes; the GPU also reads every node (mp[r][c] is the expected
    value there), within the same tolerance: the floor of the class holds at every node, and `project_ld` lands on
    every node to 1e-15 npx."""
    npx = 401
    p = pc.lattice(npx, every_node=True)[0]
    r, c, h = pc.lattice_nodes(npx, every_node=True)
    assert len(p) == npx * npx + (npx - 2) ** 2
    for kind, node in (("row", r), ("col", c)):
        up, lo = pc.masters(kind, npx, offset=0)
        ld = pc.project_ld(pc.IDENTITY, p, up, lo)[0]
        assert np.abs(ld - node).max() <= 1e-15 * npx
        got = ko.project_patterns(pc.IDENTITY, p, up, lo, dtype_out=np.float64)[0]
        assert np.abs(got - ld).max() <= pc.FLOOR["lattice"][npx]


def test_lattice_probes_land_on_their_nodes():
    """A lattice probe read through a ramp gives its node's row / column to 1e-15 npx, the hemisphere offset says
    which hemisphere, and a random master pattern gives mp[h][r][c] (a value between 0 and 1 with a slope below one
    per pixel along either axis: twice the bound)."""
    for npx in pc.NPX:
        p = pc.lattice(npx)[0]
        r, c, h = pc.lattice_nodes(npx)
        assert len(p) <= 400
        for kind, node in (("row", r), ("col", c)):
            got = pc.project_ld(pc.IDENTITY, p, *pc.masters(kind, npx))[0]
            assert np.abs(got - (node + 1000 * (h < 0))).max() <= 1e-15 * npx
        up, lo = pc.masters("random", npx)
        got = pc.project_ld(pc.IDENTITY, p, up, lo)[0]
        assert np.abs(got - np.where(h > 0, up[r, c], lo[r, c])).max() <= 2e-15 * npx


# ------------------------------------------------------------------ mutants
def _atan_last_term(t):
    """The last Horner step of atan_ratio (the coefficient of u itself) off by 1e-12 relative."""
    return np.arctan(t) + pc.LD(1e-12) * t


def _atan_seam_moved(t):
    """The seam constant 1e-6 too high: the arguments between tan(pi/8) and there take the branch that was not fitted
    for them and come out 1e-9 off."""
    a = np.abs(t)
    return np.arctan(t) + np.sign(t) * np.where((a > pc.ATAN_SEAM) & (a <= pc.ATAN_SEAM + 1e-6), pc.LD(1e-9), pc.LD(0))


MUTANTS = {
    "last arctan term off by 1e-12": dict(arctan=_atan_last_term),
    "seam moved by 1e-6, 1e-9 step": dict(arctan=_atan_seam_moved),
    "z > 0 reads upper": dict(zero_is_upper=False),
    "rows and columns swapped": dict(swap_rows_columns=True),
    "edge wraps around": dict(edge="wrap"),
}


def _rejections(**mutant):
    out = []
    for npx in pc.NPX:
        for kind, name, p, up, lo in pc.readout_cases(npx):
            got = pc.project_ld(pc.IDENTITY, p, up, lo, **mutant).astype(np.float64)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    pc.check_values(got, pc.project_ld(pc.IDENTITY, p, up, lo), name, npx)
            except AssertionError:
                out.append((npx, kind, name))
    return out


def test_readout_accepts_the_restatement_rounded_to_float64():
    assert _rejections() == []


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_readout_rejects(mutant):
    hits = _rejections(**MUTANTS[mutant])
    print(mutant, "rejected by", sorted({(kind, name) for _, kind, name in hits}))
    assert hits
    if mutant == "seam moved by 1e-6, 1e-9 step":  # at every size, by the class that was made for it
        assert {npx for npx, _, name in hits if name == "atan_seam"} == set(pc.NPX)
    if mutant == "z > 0 reads upper":
        assert {npx for npx, _, name in hits if name == "equator"} == set(pc.NPX)
    if mutant == "edge wraps around":
        assert {(npx, kind) for npx, kind, _ in hits} == {(npx, "moat") for npx in pc.NPX if npx > 2}


# ------------------------------------------------------------------ integer outputs
@pytest.mark.parametrize("out_max", [255, 65535])
def test_integer_check(out_max):
    """`project_ld` alone has no pixel within 1e-9 of an integer (so the GPU test leaves none out on the reference's
    account), passes its own check when truncated, and the check rejects float64 rescaling by a reciprocal gain
    `(v - lo) * ((omax - omin) / (hi - lo))`, which misses out_max in about one pattern of eight."""
    q, p, up, lo, ld = pc.integer_case()
    dtype = np.uint8 if out_max == 255 else np.uint16
    assert (ld[:, :pc.INT_NPIX[0]].argmax(axis=1) == pc.INT_NPIX[0] - 1).any()  # a brightest pixel that is the last
    missed = 0
    for npix in pc.INT_NPIX:
        want = pc.rescale_ld(ld[:, :npix], 0, out_max)
        assert pc.check_integer_patterns(np.trunc(want).astype(dtype), want, 0, out_max) == 0.0
        v = ld[:, :npix].astype(np.float64)
        vlo, vhi = v.min(axis=1, keepdims=True), v.max(axis=1, keepdims=True)
        mutant = ((v - vlo) * ((out_max - 0.0) / (vhi - vlo)) + 0.0).astype(dtype)
        missed += int((mutant.max(axis=1) != out_max).sum())
        with pytest.raises(AssertionError, match="pattern maximum"):
            pc.check_integer_patterns(mutant, want, 0, out_max)
    print(f"reciprocal gain misses {out_max} in {missed} of {64 * len(pc.INT_NPIX)} patterns")


def test_integer_check_without_rescale():
    want = pc.integer_case_plain()[2]
    assert pc.check_integer_patterns(np.trunc(want).astype(np.uint8), want) == 0.0
    with pytest.raises(AssertionError, match="truncated"):
        pc.check_integer_patterns(np.rint(want).astype(np.uint8), want)
