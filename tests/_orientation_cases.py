"""What the orientation tests share: the rotation groups enumerated in `np.longdouble` WITHOUT the generators of
kikuchipy_amd/sampling.py, the `np.longdouble` restatement of the disorientation angle (the brute-force double loop over
s1 and s2, the angle of every candidate product), of zone reduction and of KAM maps, the case tables, and the float64
error bound every comparison uses.  Nothing here calls kikuchipy_amd/orientations.py.

BOUND - what float64 may lose on the way from two raw rows to an angle, in units of U = 2^-53 (first order, every term
taken at its worst; magnitudes are <= 1 because the rows are normalised and the operations are unit quaternions):

  * normalisation: the sum of four squares carries (1 + U)^4, its root halves that and rounds once, the division rounds
    once: a component has a relative error of NORM = 4 U;
  * an operation of the group's table (cos and sin of multiples of pi / n, products of generators) is within TABLE = 8 U of
    the exact unit quaternion per component - tests/test_host_orientations.py asserts this of the table;
  * an equivalent s g: a component is a sum of four products s_a g_b.  The table contributes TABLE sum |g_b| <= 2 TABLE,
    the row NORM sum |s_a g_b| <= NORM, the four products and three additions 4 U sum |s_a g_b| <= 4 U:
    EQUIV = 2 TABLE + NORM + 4 = 24 U per component, 2 EQUIV = 48 U for the 4-vector (sqrt(4) components);
  * the dot product (s1 g1) . (s2 g2): both vectors' errors and four more products: DOT = 2 (2 EQUIV) + 4 = 100 U.  This is
    also what a component of the winning product (s2 g2)(s1 g1)^-1 loses, so |v| loses VEC = sqrt(3) DOT + 3 = 176.2 U (three
    components, the sum of squares and the root);
  * theta / 2 = atan2(|v|, |w|) has the gradient (|w|, -|v|) / (|v|^2 + w^2) of length 1: it inherits at most VEC + DOT, and
    atan2 itself is taken as good to 2 ulp of a result <= pi / 2: ATAN = 2 pi U < 7 U;
  * the factor 2 is exact: ANGLE = 2 (VEC + DOT + 7) = 566.4 U = 6.3e-14 rad.  Degrees multiply the bound by 180 / pi and add
    one rounding of a result <= 180.

THE CANDIDATE.  The search compares computed |dot| values, each DOT off at most: the candidate taken has a true |w| within
2 DOT of the true maximum, and may be ANY such candidate.  The restatement therefore returns, next to the smallest angle,
SLACK = (the largest angle among the candidates whose |w| is within 2 DOT U of the maximum) - (the smallest angle): 0 where
the winner is clear or the near candidates are the same rotation, as always at small angles (two different candidates lie
at least half the group's smallest rotation angle apart).  A comparison allows ANGLE + SLACK (+ 1e-16 for the restatement).

Zone reduction: a component of the result is a component of an equivalent, EQUIV = 24 U; the operation index is compared
only where the best and the second-best |w| differ by more than 2 EQUIV.  KAM: the mean of K angles is within the mean of
their bounds, plus the K - 1 additions and the division of a sum <= K pi: (K + 1) pi U."""

import os
import re

import numpy as np

from conftest import ROOT

L = np.longdouble
U = 2.0 ** -53
PI = L(np.pi) + L(1.2246467991473532e-16)  # pi to 2^-106: the double and what it leaves
assert np.finfo(L).eps < 2e-19, "np.longdouble is no wider than float64 here"

NORM, TABLE = 4, 8
EQUIV = 2 * TABLE + NORM + 4
DOT = 2 * (2 * EQUIV) + 4
VEC = np.sqrt(3) * DOT + 3
ANGLE = 2 * (VEC + DOT + 7)
RESTATEMENT = 1e-16

GROUPS = ("1", "2", "222", "4", "422", "3", "32", "6", "622", "23", "432")
ORDERS = {"1": 1, "2": 2, "222": 4, "4": 4, "422": 8, "3": 3, "32": 6, "6": 6, "622": 12, "23": 12, "432": 24}
MIXED = (("432", "622"), ("32", "1"), ("222", "4"))
REFUSED = ("m", "mm2", "-4", "4mm", "-42m", "3m", "-6", "6mm", "-6m2", "-43m")
POOL = 34  # rows of each pool: one more than the outer kernel's tile side


def header_constants():
    """The `constexpr int` constants of csrc/orientations_plan.h, read from the header."""
    text = open(os.path.join(ROOT, "kikuchipy_amd", "csrc", "orientations_plan.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (ORI_[A-Z_]+) = (\d+);", text)}


# ---- the groups, enumerated in longdouble --------------------------------------------------------------------------------
def ld_group(group):
    """(order, 4) longdouble unit quaternions of a rotation group in the package's settings (the n-fold axis along z, the
    first two-fold axis of a dihedral group along x, 23 and 432 on the cube axes), in no particular order."""
    if group in ("23", "432"):
        ops = [np.eye(4, dtype=L)[k] for k in range(4)]
        for sb in (1, -1):
            for sc in (1, -1):
                for sd in (1, -1):
                    ops.append(np.array([1, sb, sc, sd], dtype=L) / 2)
        if group == "432":
            r = np.sqrt(L(1) / 2)
            for i in range(4):
                for j in range(i + 1, 4):
                    for sign in (1, -1):
                        q = np.zeros(4, dtype=L)
                        q[i], q[j] = r, sign * r
                        ops.append(q)
        return np.array(ops)
    n = {"1": 1, "2": 2, "222": 2, "4": 4, "422": 4, "3": 3, "32": 3, "6": 6, "622": 6}[group]
    zero = L(0)
    ops = [np.array([np.cos(PI * k / n), zero, zero, np.sin(PI * k / n)]) for k in range(n)]
    if group in ("222", "422", "32", "622"):
        ops += [np.array([zero, np.cos(PI * k / n), np.sin(PI * k / n), zero]) for k in range(n)]
    return np.array(ops, dtype=L)


_LD_OPS = {}


def ld_operations(group):
    """The longdouble operations in the ORDER of the package's table (an operation index means the same thing), each
    with the table's sign; and the largest distance of a table component from them."""
    if group not in _LD_OPS:
        from kikuchipy_amd import sampling

        table = sampling.rotation_group_operations(group)
        exact = ld_group(group)
        assert table.shape == exact.shape == (ORDERS[group], 4)
        dots = table.astype(L) @ exact.T
        match = np.abs(dots).argmax(axis=1)
        assert sorted(match) == list(range(len(exact)))  # a one-to-one matching
        ordered = exact[match] * np.sign(dots[np.arange(len(match)), match])[:, None]
        _LD_OPS[group] = (ordered, float(np.abs(table.astype(L) - ordered).max()))
    return _LD_OPS[group]


# ---- the restatement -----------------------------------------------------------------------------------------------------
def ld_product(p, q):
    return np.stack([p[..., 0] * q[..., 0] - p[..., 1] * q[..., 1] - p[..., 2] * q[..., 2] - p[..., 3] * q[..., 3],
                     p[..., 0] * q[..., 1] + p[..., 1] * q[..., 0] + p[..., 2] * q[..., 3] - p[..., 3] * q[..., 2],
                     p[..., 0] * q[..., 2] - p[..., 1] * q[..., 3] + p[..., 2] * q[..., 0] + p[..., 3] * q[..., 1],
                     p[..., 0] * q[..., 3] + p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1] + p[..., 3] * q[..., 0]], axis=-1)


def ld_normalise(q):
    """Unit rows in longdouble; NaN for a row with a non-finite component or a zero norm."""
    q = np.asarray(q, dtype=np.float64)
    ok = np.isfinite(q).all(axis=-1) & (np.abs(q).max(axis=-1) > 0)
    safe = np.where(ok[..., None], q, 1.0).astype(L)
    g = safe / np.sqrt((safe * safe).sum(axis=-1))[..., None]
    return np.where(ok[..., None], g, L(np.nan))


def restate_pairs(q1, q2, group1, group2, chunk=128):
    """(P,) smallest rotation angle of (s2 g2)(s1 g1)^-1 over s1 in S1, s2 in S2 - both sides, every candidate's product
    and angle - in longdouble, and the float64 SLACK of the module docstring, of raw (P, 4) rows."""
    s1, s2 = ld_operations(group1)[0], ld_operations(group2)[0]
    g1, g2 = ld_normalise(q1), ld_normalise(q2)
    theta, slack = np.empty(g1.shape[0], dtype=L), np.empty(g1.shape[0])
    conj = np.array([1, -1, -1, -1], dtype=L)
    for lo in range(0, g1.shape[0], chunk):
        hi = min(lo + chunk, g1.shape[0])
        e1 = ld_product(s1[:, None, :], g1[None, lo:hi])                  # (n1, P, 4)
        e2 = ld_product(s2[:, None, :], g2[None, lo:hi])                  # (n2, P, 4)
        r = ld_product(e2[None], (e1 * conj)[:, None])                    # (n1, n2, P, 4)
        r = r.reshape(-1, hi - lo, 4)
        w = np.abs(r[..., 0])
        ang = 2 * np.arctan2(np.sqrt((r[..., 1:] * r[..., 1:]).sum(axis=-1)), w)
        theta[lo:hi] = ang.min(axis=0)
        near = w >= w.max(axis=0) - 2 * DOT * U
        slack[lo:hi] = (np.where(near, ang, -np.inf).max(axis=0) - theta[lo:hi]).astype(np.float64)
    return theta, slack


def angle_bound(slack, degrees=False):
    b = ANGLE * U + np.asarray(slack, dtype=np.float64) + RESTATEMENT
    return b * (180 / np.pi) + 180 * U if degrees else b


def lost(got, theta, slack, degrees=False):
    """(|got - restatement|, bound) with NaN where both are NaN taken as 0 lost; got NaN where the restatement is not (or
    the other way round) loses infinity."""
    got = np.asarray(got, dtype=np.float64)
    want = theta * (180 / PI) if degrees else theta
    err = np.abs(got.astype(L) - want).astype(np.float64)
    both = np.isnan(got) & np.isnan(want.astype(np.float64))
    err = np.where(both, 0.0, np.where(np.isnan(err), np.inf, err))
    return err, np.where(both, 0.0, angle_bound(np.where(both, 0.0, slack), degrees))


def restate_reduce(q, group):
    """(reduced rows in longdouble with a >= 0, the operation index, the gap between the best and the second-best |w|) of
    raw (P, 4) rows; NaN rows, index -1 and an infinite gap for invalid rows."""
    s = ld_operations(group)[0]
    g = ld_normalise(q)
    e = ld_product(s[:, None, :], g[None])  # (n, P, 4)
    w = np.abs(e[..., 0])
    index = np.where(np.isnan(w[0]), -1, np.nan_to_num(w.astype(np.float64), nan=-1.0).argmax(axis=0))
    best = e[np.maximum(index, 0), np.arange(g.shape[0])]
    lead = np.zeros(g.shape[0], dtype=L)
    for k in (3, 2, 1, 0):
        lead = np.where(np.abs(best[:, k]) > 1e-15, best[:, k], lead)
    best = np.where((lead < 0)[:, None], -best, best)
    ordered = np.sort(w, axis=0)
    gap = (ordered[-1] - ordered[-2]).astype(np.float64) if len(s) > 1 else np.full(g.shape[0], np.inf)
    return best, index, np.where(index < 0, np.inf, gap)


def window_offsets(window2d):
    """(dy, dx) of the non-zero coefficients of a 2-D window in C order, its origin (shape // 2) left out."""
    w = np.asarray(window2d)
    wy, wx = w.shape
    return [(y - wy // 2, x - wx // 2) for y in range(wy) for x in range(wx) if w[y, x] != 0 and (y, x) != (wy // 2, wx // 2)]


def restate_kam(q, ny, nx, group, offsets, in_data=None, max_angle=None):
    """(KAM map in longdouble radians, its bound, whether a decision against `max_angle` lies inside its own bound) of
    raw (ny nx, 4) rows: per point the pairs to its neighbours through restate_pairs, the mean in longdouble."""
    inside = np.ones((ny, nx), dtype=bool) if in_data is None else np.asarray(in_data, dtype=bool).reshape(ny, nx)
    pairs = [(y * nx + x, (y + dy) * nx + x + dx) for y in range(ny) for x in range(nx) for dy, dx in offsets
             if 0 <= y + dy < ny and 0 <= x + dx < nx and inside[y, x] and inside[y + dy, x + dx]]
    kam, bound = np.full(ny * nx, L(np.nan)), np.zeros(ny * nx)
    if not pairs:
        return kam.reshape(ny, nx), bound.reshape(ny, nx), False
    a, b = np.array(pairs).T
    theta, slack = restate_pairs(q[a], q[b], group, group)
    each = angle_bound(slack)
    keep = np.ones(len(a), dtype=bool)
    ambiguous = False
    if max_angle is not None:
        keep = ~(theta > max_angle)
        ambiguous = bool((np.abs((theta - max_angle).astype(np.float64)) <= each).any())
    for p in np.unique(a):
        mine = (a == p) & keep
        k = int(mine.sum())
        if k:
            kam[p] = theta[mine].sum() / k
            bound[p] = each[mine].sum() / k + (k + 1) * np.pi * U + RESTATEMENT
    return kam.reshape(ny, nx), bound.reshape(ny, nx), ambiguous


# ---- the case tables -------------------------------------------------------------------------------------------------------
def about(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    return np.concatenate([[np.cos(angle / 2)], axis / np.linalg.norm(axis) * np.sin(angle / 2)])


def f64_product(p, q):
    return ld_product(np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64))


_POOLS = {}


def pools(group1, group2):
    """Two pools of POOL raw rows, (A, B): row i of B is related to row i of A so that the DIAGONAL of the outer product
    (and the elementwise pairs) holds the special cases - identical rows, rows of another length, -q, exact symmetry
    equivalents of both groups, tiny angles down to 1e-9 rad, half turns, a NaN, an infinite and a zero row - and the
    off-diagonal pairs are random."""
    key = (group1, group2)
    if key in _POOLS:
        return _POOLS[key]
    rng = np.random.default_rng(sum(ord(c) for c in group1 + "/" + group2))
    a = rng.standard_normal((POOL, 4))
    a /= np.linalg.norm(a, axis=1)[:, None]
    b = rng.standard_normal((POOL, 4))
    b /= np.linalg.norm(b, axis=1)[:, None]
    s1 = ld_operations(group1)[0].astype(np.float64)
    s2 = ld_operations(group2)[0].astype(np.float64)
    b[0] = a[0]                                   # identical
    b[1] = 3.0 * a[1]                             # another length
    b[2] = -a[2]                                  # the same rotation
    b[3] = f64_product(s2[-1], a[3])              # an equivalent under the second group
    b[4] = f64_product(s2[len(s2) // 2], f64_product(s1[-1], a[4]))
    for k, angle in enumerate((1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-3)):
        b[5 + k] = f64_product(about(rng.standard_normal(3), angle), a[5 + k])  # tiny angles (group 1: exactly these)
    b[11] = f64_product(about(rng.standard_normal(3), np.pi), a[11])            # a half turn: |w| = 0 for the group 1
    a[12] = [1, 0, 0, 0]
    b[12] = [0, 0, 1, 0]                          # |w| = 0 exactly
    b[13] = f64_product(s2[-1], f64_product(about(rng.standard_normal(3), 1e-7), a[13]))  # tiny, behind an operation
    a[14] *= 0.25
    b[15, 2] = np.nan
    a[16, 0] = np.inf
    b[17] = 0.0
    a[18] = np.round(a[18] * 8)                   # integers
    if not a[18].any():
        a[18, 0] = 1.0
    a.setflags(write=False)
    b.setflags(write=False)
    _POOLS[key] = (a, b)
    return _POOLS[key]


_OUTER = {}


def outer_reference(group1, group2):
    """(theta, slack), each (POOL, POOL), of every row of pool A against every row of pool B: computed once."""
    key = (group1, group2)
    if key not in _OUTER:
        a, b = pools(group1, group2)
        i, j = np.divmod(np.arange(POOL * POOL), POOL)
        theta, slack = restate_pairs(a[i], b[j], group1, group2)
        theta, slack = theta.reshape(POOL, POOL), slack.reshape(POOL, POOL)
        theta.setflags(write=False)
        slack.setflags(write=False)
        _OUTER[key] = (theta, slack)
    return _OUTER[key]


GROUP_PAIRS = tuple((g, g) for g in GROUPS) + MIXED
INVALID_ROWS_A, INVALID_ROWS_B = (16,), (15, 17)  # rows of the pools that give NaN
