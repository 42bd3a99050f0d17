"""The restatement of the FFT filter and image quality in the kernels' own arithmetic (tests/_spectral_restate.py) and
its cases (tests/_spectral_cases.py) without a GPU: the float32 fused multiply-add against exact rational arithmetic,
the restatement pinned to the float64 reference restatements and the stored fixtures on every case, every deliberate
mistake (`wrong=`) caught by a named case, and every case's claimed path and batch count held to csrc/fftfilter_plan.h
and csrc/iq_plan.h compiled with the host compiler, with and without the switches."""

import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _spectral_cases as S
import _spectral_restate as R
from conftest import ROOT
from test_host_fft_filter import FF, INTEGER_KERNELS, assert_close, filter_f64
from test_host_image_quality import IQ, iq_f64

F32 = np.float32

# what the existing GPU tests allow between the kernels and the float64 restatements (test_gpu_fft_filter.py,
# test_gpu_image_quality.py); the restatement of the kernels' arithmetic is held to the same, no wider
FLOAT_TOL, INT_FRAC, UINT16_FRAC, IQ_TOL = 1e-5, 1e-3, 2e-2, 1e-5


# ---- fma_f32 ----------------------------------------------------------------------------------------------------------
def exact_fma(a, b, c):
    """float32 nearest-even of the exact a * b + c."""
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        return F32(0)
    lo = F32(float(v))  # (double rounding may be off by one ulp: examine the neighbours)
    cand = [lo, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf))]
    best = min(cand, key=lambda r: (abs(Fraction(float(r)) - v), int(r.view(np.uint32)) & 1))
    return F32(best)


def check_triples(a, b, c):
    got = R.fma_f32(a, b, c)
    assert got.dtype == F32
    for i in range(len(a)):
        want = exact_fma(a[i], b[i], c[i])
        assert got[i] == want, (float(a[i]), float(b[i]), float(c[i]), float(got[i]), float(want))


DOUBLE_ROUNDING = [  # (a, b, c): a b + c rounds to an f32 tie in f64, the exact value lies beside it
    (1 + 2.0 ** -23, 1 - 2.0 ** -23, 2.0 ** 24 + 2),
    (1 + 2.0 ** -23, 1 + 2.0 ** -23, 2.0 ** 24 + 2),
    (1 - 2.0 ** -24, 1 - 2.0 ** -24, 2.0 ** 25 + 4),
    (-(1 + 2.0 ** -23), 1 - 2.0 ** -23, -(2.0 ** 24 + 2)),
    (3.0, 2.0 ** -60, 1 + 2.0 ** -24),
    (-3.0, 2.0 ** -60, 1 + 3 * 2.0 ** -24),
]


def test_fma_f32_random_triples():
    rng = np.random.default_rng(11)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-8, 8, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-8, 8, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 12, n)).astype(F32)
    c[::7] = (-a[::7].astype(np.float64) * b[::7]).astype(F32)  # cancellation
    check_triples(a, b, c)


def test_fma_f32_on_float32_ties():
    """c = big + ulp / 2 - a b to f32 accuracy: the exact sum lands on, or a hair beside, an f32 tie."""
    rng = np.random.default_rng(12)
    n = 3000
    a = rng.standard_normal(n).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    big = (rng.integers(2 ** 23, 2 ** 24, n) * 2.0 ** rng.integers(-3, 6, n)).astype(F32)
    half = (np.nextafter(big, F32(np.inf)).astype(np.float64) - big) / 2
    c = (big.astype(np.float64) + half - a.astype(np.float64) * b).astype(F32)
    check_triples(a, b, c)
    # a b = half (1 + (i + j) 2^-23 + i j 2^-46): for i + j = 0 a hair off the tie, by less than f64 resolves
    i, j = rng.integers(-40, 41, n), rng.integers(-40, 41, n)
    j[::2] = -i[::2]
    a = (half * (1 + i * 2.0 ** -23)).astype(F32)
    b = (1 + j * 2.0 ** -23).astype(F32)
    check_triples(a, b, big)
    through_f64 = (a.astype(np.float64) * b + big).astype(F32)
    assert np.any(through_f64 != R.fma_f32(a, b, big))


def test_fma_f32_known_double_rounding_triples():
    a, b, c = (np.array(v, F32) for v in zip(*DOUBLE_ROUNDING))
    check_triples(a, b, c)
    assert R.fma_f32(a[:1], b[:1], c[:1])[0] == 2.0 ** 24 + 2
    through_f64 = (a.astype(np.float64) * b + c).astype(F32)
    assert through_f64[0] == 2.0 ** 24 + 4
    assert np.any(through_f64 != R.fma_f32(a, b, c))  # otherwise the list proves nothing


def test_twiddles_and_block_sum():
    c, s = R.twiddles(4)
    assert c.dtype == F32 and c[1] == F32(6.123233995736766e-17) and s[2] == F32(1.2246467991473532e-16)
    v = np.arange(256, dtype=np.float64) * 2.0 ** -40 + 2.0 ** 20
    t = v.reshape(4, 64)
    waves = []
    for w in range(4):  # lane 0 of the butterfly 32 ... 1, written out
        lane = list(t[w])
        for o in (32, 16, 8, 4, 2, 1):
            lane = [lane[i] + lane[i ^ o] for i in range(64)]
        waves.append(lane[0])
    assert R.block_sum(v) == ((0.0 + waves[0]) + waves[1]) + waves[2] + waves[3]


# ---- the restatement pinned to the reference -----------------------------------------------------------------------
def int_frac(c):
    if c.shape == (1, 64):
        return 5e-2  # test_host_fft_filter.test_restatement_matches_the_reference_on_synthetic_stacks: 128 pixels
    if c.tf in INTEGER_KERNELS or c.tf in ("one", "zero_k"):
        return 1e-2  # test_host_fft_filter.tie_fraction: integer taps on integer patterns make exact ties common
    # 16-bit outputs: one grey level is 1.5e-5 of the range, below what f32 DFT sums resolve on every pixel
    # (test_gpu_fft_filter.frac_for gives uint16 this share; int16 has as many levels)
    return UINT16_FRAC if c.dtype in ("uint16", "int16") else INT_FRAC


@pytest.mark.parametrize("name", [n for n in S.NAMES if S.CASES[n].op != "iq"])
def test_fft_filter_restatement_against_the_reference(name):
    c = S.CASES[name]
    got, stages = S.expected(name)
    stack = S.stack(name)
    assert got.dtype == stack.dtype and got.shape == stack.shape
    tf, shift = S.transfer(name)
    want = filter_f64(stack, c.op, shift, tf)
    deg = stages["degenerate"]
    if c.kind in ("degenerate", "constant"):
        # the kernels define a constant pattern, and a constant filtered result, as degenerate, where the reference
        # rescales its FFT's round-off (test_gpu_fft_filter.test_degenerate_patterns): compare the others
        flat = stack.reshape(len(stack), -1)
        const = (flat.min(axis=1) == flat.max(axis=1)) | (c.kind == "constant")
        assert np.array_equal(deg, const | ~np.isfinite(flat.astype(np.float64)).all(axis=1)), name
        zero = 0 if stack.dtype.kind in "iu" else np.nan
        assert np.array_equal(got[deg], np.full_like(got[deg], zero), equal_nan=True)
        got, want = got[~deg], want[~deg]
        if not len(got):
            return
    elif c.kind != "cancel":
        assert not deg.any(), name
    if c.kind == "cancel":
        return  # (2^60 next to ordinary pixels: the float32 DFT and the float64 one agree on the two spikes only)
    assert_close(got, want, name, int_frac(c), atol=FLOAT_TOL)
    if c.kind == "fixture":
        assert_close(got, FF[S.fixture_key(c)], name, int_frac(c), atol=FLOAT_TOL)


@pytest.mark.parametrize("name", [n for n in S.NAMES if S.CASES[n].op == "iq"])
def test_image_quality_restatement_against_the_reference(name):
    c = S.CASES[name]
    got, stages = S.expected(name)
    stack = S.stack(name)
    assert got.dtype == F32 and got.shape == (len(stack),)
    w, imax = S.iq_arguments(name)
    if c.kind == "cancel_weights":
        return  # (weights of +-2^50 that cancel: the reference's float64 sum keeps none of the ordinary terms)
    want = iq_f64(stack, c.normalize, w, imax or None)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (name, got, want)
    ok = ~np.isnan(got)
    assert np.max(np.abs(got[ok] - want[ok]), initial=0.0) <= IQ_TOL, (name, got, want)
    if c.kind == "fixture":
        assert np.max(np.abs(got - IQ[S.fixture_key(c)])) <= IQ_TOL, name


# ---- the cases discriminate -------------------------------------------------------------------------------------------
CAUGHT_BY = {  # wrong variant: the cases that catch it (the filter's, then image quality's or the spatial domain's)
    # (a one-hot table cannot: the min / max rescale divides a factor on its only column out again)
    "self_twice": [S.find("dtype", "frequency", (60, 60), 0, "float32"), S.find("shape", "iq", (4, 6), 0)],
    "last_once": [S.find("dtype", "frequency", (7, 9), 0, "float32"), S.find("shape", "iq", (3, 5), 1)],
    "twiddle_mod": [S.find("dtype", "frequency", (7, 9), 0, "float32"), S.find("shape", "iq", (5, 5), 0)],
    "no_fma": [S.find("dtype", "frequency", (60, 60), 0, "float32"), S.find("dtype", "iq", (60, 60), 1, "float32")],
    "mean_f64": [S.find("dtype", "iq", (60, 60), 0, "float32")],
    "batch_offset": [S.find("batch", "frequency", (12, 10), 1), S.find("batch", "iq", (12, 10), 1),
                     S.find("batch", "spatial", (17, 300), 1)],
    "int8_as_uint8": [S.find("dtype", "frequency", (7, 9), 0, "int8"), S.find("dtype", "spatial", (60, 60), 1, "int8")],
}


def differs(a, b):
    return not np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("wrong", sorted(CAUGHT_BY))
def test_every_mistake_changes_an_output(wrong):
    for name in CAUGHT_BY[wrong]:
        right, _ = S.expected(name)
        assert differs(S.expected(name, wrong)[0], right), (wrong, name)
    print(wrong, "is caught by", CAUGHT_BY[wrong])


def test_the_other_paths_summation_order_changes_an_output():
    """The f64 sums of a path feed the mean (rounded to f32) or the quotient of image quality (rounded to f32), and
    sums of float32 values in f64 are exact or within a few units of 2^-53 for ordinary patterns: no output of an
    ordinary stack can tell the two orders apart.  The `cancel` cases can (tests/_spectral_cases.py says how), at
    60 x 60 on every pattern; so a GPU run that equals the restatement of its path on them has taken that path."""
    for op in ("frequency", "iq"):
        for shape, dtype in (((60, 60), "float32"), ((17, 300), "float64")):
            a, b = (S.find("cancel", op, shape, path, dtype) for path in (0, 1))
            ra, rb = S.expected(a)[0], S.expected(b)[0]
            per_pattern = (ra != rb).reshape(len(ra), -1).any(axis=1)
            assert per_pattern.all() if shape == (60, 60) else per_pattern.any(), (a, b)
            assert np.array_equal(S.expected(a, "other_sum")[0], rb) and np.array_equal(S.expected(b, "other_sum")[0], ra)
            assert np.isfinite(ra.astype(np.float64)).all() and np.isfinite(rb.astype(np.float64)).all()
    for name, c in S.CASES.items():
        if c.batch and name.startswith("cancel-"):
            assert differs(S.expected(name, "other_sum")[0], S.expected(name)[0]), name
            assert differs(S.expected(name, "batch_offset")[0], S.expected(name)[0]), name


def test_integer_stacks_do_not_depend_on_the_path():
    """Sums of integers are exact in f64, so for integer dtypes both paths must give the same bits."""
    for name, c in S.CASES.items():
        if c.path == 0 and c.dtype in ("uint8", "int8", "uint16", "int16") and c.op != "iq":
            other = name.replace("-p0-", "-p1-")
            if other in S.CASES:
                assert np.array_equal(S.expected(name)[0], S.expected(other)[0]), name


def test_cases_cover_what_they_claim():
    cs = list(S.CASES.values())
    for op in S.OPS:
        for path in (0, 1):
            assert {c.dtype for c in cs if c.op == op and c.path == path} == set(S.DTYPES), (op, path)
        assert {c.shape for c in cs if c.op == op and c.forced} >= set(S.SMALL), op
        assert any(c.batch and S.batches(c) == 3 and c.n % c.batch for c in cs if c.op == op), op
    assert {c.normalize for c in cs if c.op == "iq"} == {True, False}
    stack = S.stack("narrow-frequency-6x7-float64-lowhigh-p0-n2")
    assert np.any(stack != stack.astype(F32)) and (stack < 0).any() and (stack == 0).any()
    for c in cs:
        assert c.shape[0] * c.shape[1] <= 139 * 139 and len(S.stack(c.name)) == c.n, c.name


# ---- bookkeeping against the compiled plan headers --------------------------------------------------------------------
PLAN_PROBE = r"""
#include "fftfilter_plan.h"
#include "iq_plan.h"
#include <cstdio>
struct C { int op, sy, sx; long n; int force; long cap; };
static void show(const kpdi::PatternPath &p) { std::printf(" %d %ld %zu", p.path, (long)p.batch, p.workspace_bytes); }
int main() {
  const C cases[] = {%s};
  for (const C &c : cases) {
    for (int sw = 0; sw < 2; ++sw) {
      const bool f = sw && c.force;
      const long cap = sw ? c.cap : 0;
      if (c.op == 2) show(kpdi::iq_plan(c.sy, c.sx, c.n, f, cap));
      else show(kpdi::ff_plan(c.op, c.sy, c.sx, c.n, f, cap));
    }
    std::printf(" %zu\n", c.op == 2 ? kpdi::iq_lds_path_bytes(c.sy, c.sx) : kpdi::ff_lds_path_bytes(c.op, c.sy, c.sx));
  }
}
"""


def test_claimed_paths_and_batches_are_the_plans(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    cs = list(S.CASES.values())
    rows = ", ".join("{%d, %d, %d, %dL, %d, %dL}" % (S.OPS.index(c.op), c.shape[0], c.shape[1], c.n, c.forced, c.batch or 0)
                     for c in cs)
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PLAN_PROBE.replace("%s", rows))
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert len(lines) == len(cs)
    for c, line in zip(cs, lines):
        path0, batch0, ws0, path1, batch1, ws1, lds = map(int, line.split())
        assert lds == S.lds_path_bytes(c.op, *c.shape), c.name
        # without the switches: the natural path, one batch
        assert path0 == S.natural_path(c.op, c.shape) and batch0 == c.n, c.name
        assert (path0 == 0) == (ws0 == 0), c.name
        assert c.forced == (path0 != c.path), c.name
        # with them: what the case claims
        assert path1 == c.path, c.name
        assert -(-c.n // batch1) == S.batches(c), c.name
        if c.path == 1:
            assert batch1 == (min(c.batch, c.n) if c.batch else c.n) and ws1 > 0 and ws1 % batch1 == 0, c.name
            if path0 == 1:  # the workspace follows the cap
                assert ws1 // batch1 == ws0 // batch0, c.name
        else:
            assert batch1 == c.n and ws1 == 0, c.name  # the cap belongs to path 1
    # the boundary cases sit on the sides they claim, next to each other
    for op, first in S.BOUNDARY.items():
        assert S.natural_path(op, (first - 1, first - 1)) == 0 and S.natural_path(op, (first, first)) == 1
        assert any(c.op == op and c.shape == (first - 1, first - 1) and c.path == 0 and not c.forced for c in cs)
        assert any(c.op == op and c.shape == (first, first) and c.path == 1 and not c.forced for c in cs)
