"""Dictionaries whose best matches are known BY CONSTRUCTION, in the orders that drive the slow paths of the fused top-k
(csrc/match16.hip, match.hip, tailgemm.hip, merge.hip): pure NumPy, seeded, no GPU.  tests/test_host_topk_cases.py checks
every builder against the float64 oracle on the CPU, tests/test_gpu_topk_adversarial.py runs them through every kernel form.

Ladder.  A "grain" g has a probe pattern p_g (zero mean, unit norm; the probes are orthogonal to each other).  Dictionary
entry j of grain g is  a_j p_g + sqrt(1 - a_j^2) q_j  with unit noise q_j made orthogonal (in float64) to every probe and to
the constant pattern, then given a gain and an offset and rounded to float32: its ncc score against any positive affine
image of p_g is a_j up to that rounding (~1e-7), and ~0 against the images of the other probes.  The best `n_sep` rungs of
every grain are `spacing` apart, the rest of the grain lies densely below them.  For ndp the same without mean removal:
positive probes, no offsets, noise orthogonal to the probes only.

`Case.key[g][j]` is the constructed score of entry j for the rows of grain g (duplicates carry EQUAL keys: they score
bit-equal in every arithmetic), `Case.expected(keep_n)` the ranking by (key descending, index ascending).
"""
import numpy as np

TIE = 2e-5            # the default `tie` of oracle.kpdi_oracle.assert_topk_parity
SPACING = 4e-3        # well above 2 * TIE, and 7 sigma of what rounding the experimental patterns to uint8 does to the
                      # difference of two neighbouring scores (measured on the oracle: a few 1e-4 at the lower rungs)
TOP = 0.97
TILE = 256            # dictionary rows per tile of match16.hip
# (experimental patterns, dictionary entries, grains) of the GPU test: one row block against 6 tiles - fewer than 32 lists per
# pattern, the PLAIN plan of the shared bound (kernels.h: bound_plan) - and 16 row blocks against 49 / 111 tiles, the last
# one partial (a partial last 32-row unit too): the GROUPED plan, 3 and 6 whole tiles per workgroup
SIZES = [(200, 1500, 2), (4096, 12500, 3), (4096, 28300, 2)]
ORDERS = ("shuffled", "ascending", "descending", "block_ascending", "lane_concentrated", "last_rows")


class Case:
    """dic (n, sy, sx) float32; exp (m, sy, sx) float32 and exp_u8 (the same patterns, as uint8 images); row_grain (m,);
    key (grains, n) float64."""

    def __init__(self, dic, exp, exp_u8, row_grain, key, metric):
        self.dic, self.exp, self.exp_u8, self.row_grain, self.key, self.metric = dic, exp, exp_u8, row_grain, key, metric

    def ranking(self, keep_n):
        """(grains, keep_n) dictionary indices: best first, ties by lower index first."""
        n = self.key.shape[1]
        return np.stack([np.lexsort((np.arange(n), -k))[:keep_n] for k in self.key])

    def expected(self, keep_n, rows=None, start=0):
        """(rows, keep_n) expected dictionary indices of a sweep pushed at dictionary index `start`."""
        g = self.row_grain if rows is None else self.row_grain[rows]
        return self.ranking(keep_n)[g] + start

    def expected_scores(self, keep_n, rows=None):
        g = self.row_grain if rows is None else self.row_grain[rows]
        rk = self.ranking(keep_n)
        return np.stack([self.key[i][rk[i]] for i in range(len(rk))])[g]

    def reorder(self, perm):
        """The same case with the dictionary in the order `perm` (entry i of the new dictionary = entry perm[i] of this)."""
        return Case(np.ascontiguousarray(self.dic[perm]), self.exp, self.exp_u8, self.row_grain, self.key[:, perm], self.metric)


def _unit(v, axis=-1):
    return v / np.sqrt(np.sum(v * v, axis=axis, keepdims=True))


def _probes(rng, grains, k, metric):
    """(grains, k) float64, unit norm, mutually orthogonal; ncc: zero mean; ndp: positive."""
    if metric == "ncc":
        basis = [np.ones(k) / np.sqrt(k)]
        out = []
        for _ in range(grains):
            v = rng.standard_normal(k)
            for _ in range(2):  # (twice: orthogonal to 1e-16)
                for b in basis:
                    v -= (v @ b) * b
            v = _unit(v)
            basis.append(v)
            out.append(v)
        return np.array(out)
    # ndp: positive patterns are orthogonal only on disjoint supports - pixel i belongs to probe i % grains
    out = np.zeros((grains, k))
    for g in range(grains):
        out[g, g::grains] = 0.5 + rng.random(len(out[g, g::grains]))
    return _unit(out)


def _noise(rng, n, basis):
    """(n, k) float64 unit rows orthogonal to every row of the orthonormal `basis`."""
    q = rng.standard_normal((n, basis.shape[1]))
    for _ in range(2):
        q -= (q @ basis.T) @ basis
    return _unit(q)


def rungs(n_g, n_sep, spacing, top=TOP, negative=False):
    """Scores of one grain, best first: `n_sep` rungs `spacing` apart from `top` down, the other n_g - n_sep spread evenly
    (densely) between the lowest of them and 0.02.  `negative`: the whole ladder mirrored below zero (-0.02 is then the
    best score, the dense part on top)."""
    n_sep = min(n_sep, n_g)
    a = top - spacing * np.arange(n_sep)
    floor = a[-1] - spacing
    assert floor > 0.05, f"{n_sep} rungs of {spacing} do not fit below {top}"
    if n_g > n_sep:
        a = np.concatenate([a, np.linspace(floor, 0.02, n_g - n_sep)])
    return -a[::-1] if negative else a


def ladder(n, m, keep_n_max=70, grains=3, spacing=SPACING, metric="ncc", sy=24, sx=20, seed=0, negative=False):
    """The canonical ladder: entry j belongs to grain j % grains and holds that grain's rung j // grains (0 = best), so
    the dictionary falls by score and the grains interleave; row i shows grain i % grains.  2 * keep_n_max
    well-separated rungs per grain."""
    rng = np.random.default_rng(seed)
    k = sy * sx
    probes = _probes(rng, grains, k, metric)
    basis = np.vstack([probes, np.ones((1, k)) / np.sqrt(k)]) if metric == "ncc" else probes
    grain = np.arange(n) % grains
    a = np.empty(n)
    for g in range(grains):
        a[grain == g] = rungs(int((grain == g).sum()), 2 * keep_n_max, spacing, negative=negative)
    d = a[:, None] * probes[grain] + np.sqrt(1 - a * a)[:, None] * _noise(rng, n, basis)
    gain = 20.0 + 40.0 * rng.random(n)
    if metric == "ncc":
        d = d * gain[:, None] + (30.0 + 20.0 * rng.random(n))[:, None]
    else:
        d = d * gain[:, None]
    assert grains == 1 or not negative  # (the other grains' entries score ~0: above every negative rung)
    key = np.where(grain[None, :] == np.arange(grains)[:, None], a[None, :], 0.0)
    row_grain = np.arange(m) % grains
    eg = 400.0 + 600.0 * rng.random(m)
    if metric == "ncc":
        # positive affine images g p + o; the uint8 image spans [0, 255] like a camera frame
        e = probes[row_grain] * eg[:, None] + (100.0 + 50.0 * rng.random(m))[:, None]
        p = probes[row_grain]
        lo, hi = p.min(axis=1, keepdims=True), p.max(axis=1, keepdims=True)
        span = 200.0 + 55.0 * rng.random((m, 1))
        e8 = np.rint((p - lo) / (hi - lo) * span).astype(np.uint8)
    else:
        e = probes[row_grain] * eg[:, None]
        p = probes[row_grain]
        span = 200.0 + 55.0 * rng.random((m, 1))
        e8 = np.rint(p / p.max(axis=1, keepdims=True) * span).astype(np.uint8)
    return Case(d.astype(np.float32).reshape(n, sy, sx), e.astype(np.float32).reshape(m, sy, sx), e8.reshape(m, sy, sx),
                row_grain, key, metric)


def lane_rows(h, groups):
    """Rows of a tile that ONE lane of one wave sees (match16.hip, "this lane's NCG lists"): 4 h + {0..3} + 8 j of
    consecutive 32-row groups."""
    r = np.arange(16)
    one = 4 * h + (r & 3) + 8 * (r >> 2)
    return (32 * np.arange(groups)[:, None] + one[None, :]).ravel()


def order(case, name, keep_n=20, seed=1):
    """(perm, inv): the dictionary in order `name` is case.dic[perm]; inv[perm] = arange (inv[j] = where entry j went).
    `case` must be a canonical ladder (falling by score: rung = index // grains)."""
    n = case.key.shape[1]
    grains = case.key.shape[0]
    rng = np.random.default_rng(seed)
    falling = np.arange(n)
    if name == "shuffled":
        perm = rng.permutation(n)
    elif name == "descending":
        perm = falling
    elif name == "ascending":
        perm = falling[::-1].copy()
    elif name == "block_ascending":
        # every tile beats the one before it and falls inside; the partial last tile takes the best n % TILE entries
        tail = n % TILE
        body = falling[tail:].reshape(-1, TILE)[::-1].ravel()
        perm = np.concatenate([body, falling[:tail]])
    elif name == "lane_concentrated":
        # the best keep_n + 8 entries of grain g on the rows lane-half h = g % 2 sees in tile t_g; the rest shuffled
        per = keep_n + 8
        n_tiles = n // TILE
        assert n_tiles >= grains + 1 and per <= 128
        perm = np.full(n, -1)
        best = []
        for g in range(grains):
            t = (g + 1) * n_tiles // (grains + 1)
            rows = t * TILE + lane_rows(g % 2, 8)[:per]
            mine = g + grains * np.arange(per)
            perm[rows] = mine[rng.permutation(per)]
            best.append(mine)
        rest = np.setdiff1d(falling, np.concatenate(best))
        perm[perm < 0] = rest[rng.permutation(len(rest))]
    elif name == "last_rows":
        # the best grains * (keep_n + 8) entries at the very end, rising: the final partial tile, the best of all in the
        # final 32-row unit; the rest shuffled
        cnt = grains * (keep_n + 8)
        rest = falling[cnt:]
        perm = np.concatenate([rest[rng.permutation(len(rest))], falling[:cnt][::-1]])
    else:
        raise ValueError(name)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    return perm.astype(np.int64), inv


def _scatter(rng, n, count, taken):
    """`count` free positions spread over the whole dictionary, one from each of `count` equal strata (every tile, split
    and chunk gets some)."""
    free = np.setdiff1d(np.arange(n), taken)
    assert len(free) >= 2 * count
    return free[(np.arange(count) * len(free)) // count + rng.integers(0, len(free) // count, count)]


def all_identical(n, m, sy=24, sx=20, seed=3):
    """Plateau 1: every dictionary entry is the same pattern - every row's answer is arange(keep_n)."""
    base = ladder(8, m, keep_n_max=1, grains=1, sy=sy, sx=sx, seed=seed)
    dic = np.ascontiguousarray(np.broadcast_to(base.dic[0], (n, sy, sx)))
    return Case(dic, base.exp, base.exp_u8, base.row_grain, np.full((1, n), base.key[0, 0]), "ncc")


def late_plateau(n, m, first, sy=24, sx=20, seed=6):
    """Plateau 1 with its lowest indices moved away from the tile a workgroup visits first: entries [first, n) are one
    pattern (the best score), entries [0, first) a falling ladder below it.  Every row's answer is first + arange(keep_n).
    Under the permuted tile order of match16.hip the winning ties then arrive AFTER higher-index ties of the same score
    have filled the lists: only non-strict thresholds and the (score, index) insertion let them in."""
    base = ladder(first + 1, m, keep_n_max=1, grains=1, sy=sy, sx=sx, seed=seed)
    dic = np.concatenate([base.dic[1:], np.broadcast_to(base.dic[0], (n - first, sy, sx))])
    key = np.concatenate([base.key[:, 1:], np.full((1, n - first), base.key[0, 0])], axis=1)
    return Case(np.ascontiguousarray(dic), base.exp, base.exp_u8, base.row_grain, key, "ncc")


def plateau(n, m, r, copies, placement="scattered", keep_n_max=70, grains=3, spacing=SPACING, sy=24, sx=20, seed=4):
    """Plateaus 2 (r = 0) and 3: a shuffled ladder in which, for every grain, `copies` entries from below the
    well-separated rungs are overwritten by exact copies of the grain's rung r (0-based): r better rungs, then
    copies + 1 bit-equal scores.  `placement`: "contiguous" (one run per grain) or "scattered" over the whole dictionary."""
    base = ladder(n, m, keep_n_max, grains, spacing, "ncc", sy, sx, seed)
    rng = np.random.default_rng(seed + 100)
    perm, inv = order(base, "shuffled", seed=seed + 1)
    c = base.reorder(perm)
    dic, key = c.dic.copy(), c.key.copy()
    keep = inv[np.arange(grains * 2 * keep_n_max)]  # where the well-separated rungs are: never overwritten
    taken = keep.copy()
    for g in range(grains):
        src = inv[g + grains * r]
        if placement == "contiguous":
            free = np.setdiff1d(np.arange(n), taken)
            pos = free[free >= g * n // grains + 7][:copies]
            assert len(pos) == copies
        else:
            pos = _scatter(rng, n, copies, taken)
        taken = np.concatenate([taken, pos])
        dic[pos] = dic[src]
        key[:, pos] = key[:, src][:, None]
    return Case(dic, c.exp, c.exp_u8, c.row_grain, key, "ncc")


def zero_plateau(n, m, copies=300, sy=24, sx=20, seed=5):
    """Plateau 4: one grain whose every rung is NEGATIVE, and `copies` constant (degenerate) patterns scattered through the
    dictionary - they score exactly +0.0 and are everybody's best matches."""
    base = ladder(n, m, keep_n_max=8, grains=1, sy=sy, sx=sx, seed=seed, negative=True)
    rng = np.random.default_rng(seed + 100)
    perm, _ = order(base, "shuffled", seed=seed + 1)
    c = base.reorder(perm)
    dic, key = c.dic.copy(), c.key.copy()
    pos = _scatter(rng, n, copies, np.empty(0, dtype=np.int64))
    dic[pos] = (37.0 + np.arange(len(pos)) % 5).astype(np.float32)[:, None, None]
    key[:, pos] = 0.0
    return Case(dic, c.exp, c.exp_u8, c.row_grain, key, "ncc")


def min_gap(scores):
    """Smallest difference between neighbouring scores of sorted lists (rows x k)."""
    return float(np.min(-np.diff(np.asarray(scores, dtype=np.float64), axis=1)))
