"""A NumPy restatement of the three stages of Hough indexing (csrc/hough_plan.h, csrc/hough_vote.h,
csrc/hough.hip), written from the definitions: the Radon transform in float32 in the kernel's order of operations (every
multiplication and addition rounded on its own, the steps along a line ascending), band detection in float32, and the
vote and the fit in float64 - the fit by an SVD (Kabsch), not by the kernel's Jacobi sweeps.  The cos / sin table and the
smoothing taps are inputs (the package computes them on the host and hands the same bits to the kernels).

`wrong` selects a deliberately wrong variant: "rho_not_flipped" (the theta seam keeps rho), "y_not_negated" (the band
normal's y component keeps its sign), "half_pixel" (the pattern centre taken at N / 2 instead of (N - 1) / 2).

Shared by tests/test_host_hough.py, tests/test_gpu_hough.py and tests/test_gpu_hough_workflow.py."""

import itertools

import numpy as np

F = np.float32
THREADS, WINDOW = 256, 3  # HOUGH_THREADS, HOUGH_WINDOW
MIN_MATCHES, MIN_PAIR = 3, np.deg2rad(10.0)  # HV_MIN_MATCHES, HV_MIN_PAIR


# ---- stage 1: the Radon transform ---------------------------------------------------------------------------------------
def geometry(ny, nx, n_theta, n_rho, wrong=None):
    r = (min(ny, nx) - 1) / 2.0
    shift = 0.5 if wrong == "half_pixel" else 0.0
    g = dict(ny=ny, nx=nx, n_theta=n_theta, n_rho=n_rho, t_half=int(np.ceil(r)), cx=F((nx - 1) / 2.0 + shift),
             cy=F((ny - 1) / 2.0 + shift), r2=F(r * r), drho=F(2.0 * np.floor(r) / (n_rho - 1)), dtheta=F(np.pi / n_theta))
    i, j = np.mgrid[0:ny, 0:nx]
    dx, dy = j.astype(F) - g["cx"], i.astype(F) - g["cy"]
    g["mask"] = dx * dx + dy * dy <= g["r2"]
    return g


def staged(pattern, g):
    """Mask applied, masked mean removed: float32.  The mean is summed in float64 the way the kernel's threads do."""
    flat, mask = pattern.astype(np.float64).ravel(), g["mask"].ravel()
    pad = -flat.size % THREADS
    rows = np.concatenate([flat, np.zeros(pad)]).reshape(-1, THREADS)
    use = np.concatenate([mask, np.zeros(pad, dtype=bool)]).reshape(-1, THREADS)
    acc = np.zeros(THREADS)
    with np.errstate(invalid="ignore", over="ignore"):
        for row, u in zip(rows, use):
            acc = np.where(u, acc + row, acc)
        total = 0.0
        for t in range(THREADS):
            total = total + acc[t]
        mean = F(total / float(mask.sum()))
        return np.where(g["mask"], pattern.astype(F) - mean, F(0)).astype(F)


def radon(pattern, g, cos_sin):
    """S[a][k], float32, bit for bit what the kernel computes."""
    p = np.zeros((g["ny"] + 2, g["nx"] + 2), dtype=F)
    p[1:-1, 1:-1] = staged(pattern, g)

    def pixel(i, j):
        return p[np.clip(i, -1, g["ny"]) + 1, np.clip(j, -1, g["nx"]) + 1]

    k = np.arange(g["n_rho"], dtype=F)
    rho = ((k - F(g["n_rho"] - 1) * F(0.5)) * g["drho"])[None, :]
    c, s = cos_sin[0].astype(F)[:, None], cos_sin[1].astype(F)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        x0, y0, rr = g["cx"] + rho * c, g["cy"] + rho * s, rho * rho
        acc = np.zeros((g["n_theta"], g["n_rho"]), dtype=F)
        for t in range(-g["t_half"], g["t_half"] + 1):
            tf = F(t)
            use = ~(rr + tf * tf > g["r2"])
            x, y = x0 - tf * s, y0 + tf * c
            xf, yf = np.floor(x), np.floor(y)
            fx, fy = x - xf, y - yf
            j, i = xf.astype(np.int64), yf.astype(np.int64)
            v00, v01, v10, v11 = pixel(i, j), pixel(i, j + 1), pixel(i + 1, j), pixel(i + 1, j + 1)
            top, bot = v00 + fx * (v01 - v00), v10 + fx * (v11 - v10)
            acc = np.where(use, acc + (top + fy * (bot - top)), acc)
    assert acc.dtype == F
    return acc


# ---- stage 2: band detection ----------------------------------------------------------------------------------------------
def theta_shift(u, d, wrong=None):
    """u(a + d, k) of the periodic sinogram: rows beyond the seam come from the other end with rho flipped."""
    n = u.shape[0]
    wrapped = u if wrong == "rho_not_flipped" else u[:, ::-1]
    ext = np.concatenate([wrapped, u, wrapped], axis=0)
    return ext[n + d:2 * n + d]


def smooth(s, wt, wr, wrong=None):
    n_rho = s.shape[1]
    rr, rt = len(wr) // 2, len(wt) // 2
    with np.errstate(invalid="ignore", over="ignore"):
        tmp = np.zeros_like(s)
        for d in range(-rr, rr + 1):
            lo, hi = max(0, -d), min(n_rho, n_rho - d)
            term = np.zeros_like(s)
            term[:, lo:hi] = F(wr[d + rr]) * s[:, lo + d:hi + d]
            inside = np.zeros(n_rho, dtype=bool)
            inside[lo:hi] = True
            tmp = np.where(inside[None, :], tmp + term, tmp)
        u = np.zeros_like(s)
        for d in range(-rt, rt + 1):
            u = u + F(wt[d + rt]) * theta_shift(tmp, d, wrong)
    assert u.dtype == F
    return u


def vertex(left, c, right):
    den = (left - F(2) * c) + right
    with np.errstate(invalid="ignore", divide="ignore"):
        d = F(0.5) * (left - right) / den
    d = np.where(den < 0, d, F(0))
    return np.clip(d, F(-0.5), F(0.5)).astype(F)


def bands(s, g, wt, wr, rim, n_bands, wrong=None):
    """The band records of one sinogram: a structured array like the library's (theta, rho, value, valid, a, k, da, dk)."""
    from kikuchipy_amd import _lib

    u = smooth(s, wt, wr, wrong)
    n_theta, n_rho = u.shape
    ok = peaks(u, rim, wrong)
    cells = np.flatnonzero(ok.ravel())
    order = sorted(cells, key=lambda o: (-float(u.ravel()[o]), int(o)))[:n_bands]
    out = np.zeros(n_bands, dtype=_lib.HOUGH_BAND_DTYPE)
    out["a"], out["k"] = -1, -1
    for b, o in enumerate(order):
        a, k = divmod(int(o), n_rho)
        left, right = theta_shift(u, -1, wrong)[a, k], theta_shift(u, 1, wrong)[a, k]
        c = u[a, k]
        da, dk = vertex(left, c, right), vertex(u[a, k - 1], c, u[a, k + 1])
        theta = (F(a) + da) * g["dtheta"]
        rho = ((F(k) + dk) - F(n_rho - 1) * F(0.5)) * g["drho"]
        out[b] = (theta, rho, c, 1, a, k, da, dk)
    return out, u


def peaks(u, rim, wrong=None):
    """Boolean (n_theta, n_rho): the positive local maxima of the 7 x 7 window - larger than every other cell of it, or
    equal with the lower cell index -, the window continuing across the theta seam with rho flipped."""
    n_theta, n_rho = u.shape
    a, k = np.mgrid[0:n_theta, 0:n_rho]
    here = a * n_rho + k
    with np.errstate(invalid="ignore"):
        ok = (u > 0) & (k >= rim) & (k < n_rho - rim)
        for da in range(-WINDOW, WINDOW + 1):
            for dk in range(-WINDOW, WINDOW + 1):
                if da == 0 and dk == 0:
                    continue
                aa, kk = a + da, k + dk
                over = (aa < 0) | (aa >= n_theta)
                aw = np.mod(aa, n_theta)
                kw = kk if wrong == "rho_not_flipped" else np.where(over, n_rho - 1 - kk, kk)
                exists = (kw >= 0) & (kw < n_rho)
                kc = np.clip(kw, 0, n_rho - 1)
                there = aw * n_rho + kc
                v = u[aw, kc]
                ok &= ~exists | (there == here) | (u > v) | ((u == v) & (here < there))
    return ok


# ---- stage 3: normals, vote, fit --------------------------------------------------------------------------------------------
def band_normals(theta, rho, pc, ny, nx, wrong=None):
    """Unit normals (n, 3) in the detector frame of bands (theta [rad], rho [px]) under one PC."""
    theta, rho = np.asarray(theta, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    aspect = nx / ny
    xs, ys = aspect / pc[2] / (nx - 1), 1.0 / pc[2] / (ny - 1)
    xoff, yoff = aspect * pc[0] / pc[2], pc[1] / pc[2]
    cx, cy, c, s = (nx - 1) / 2.0, (ny - 1) / 2.0, np.cos(theta), np.sin(theta)
    sign = 1.0 if wrong == "y_not_negated" else -1.0
    n = np.stack([c / xs, sign * s / ys, c * (xoff / xs - cx) + s * (yoff / ys - cy) - rho], axis=-1)
    return n / np.sqrt(np.sum(n * n, axis=-1))[..., None]


def kabsch(a, b):
    """The rotation R that maximises sum b_i . (R a_i)."""
    u, _, vt = np.linalg.svd(b.T @ a)
    d = np.sign(np.linalg.det(u @ vt))
    return u @ np.diag([1.0, 1.0, d]) @ vt


def om2qu(om):
    """The inverse of tests/_geometrical_cases.py: to_matrix, a >= 0."""
    s = np.array([1 + om[0, 0] + om[1, 1] + om[2, 2], 1 + om[0, 0] - om[1, 1] - om[2, 2], 1 - om[0, 0] + om[1, 1] - om[2, 2],
                  1 - om[0, 0] - om[1, 1] + om[2, 2]])
    top = int(np.argmax(s))
    ab, ac, ad = om[2, 1] - om[1, 2], om[0, 2] - om[2, 0], om[1, 0] - om[0, 1]
    bc, bd, cd = om[0, 1] + om[1, 0], om[0, 2] + om[2, 0], om[1, 2] + om[2, 1]
    r = 0.5 * np.sqrt(max(s[top], 0.0))
    f = 0.25 / r
    q = [np.array([r, ab * f, ac * f, ad * f]), np.array([ab * f, r, bc * f, bd * f]), np.array([ac * f, bc * f, r, cd * f]),
         np.array([ad * f, bd * f, cd * f, r])][top]
    return -q if q[0] < 0 else q


def match(R, normals, phase_normals, tol):
    d = normals @ (phase_normals @ R.T).T  # (bands, reflectors)
    at = np.argmax(np.abs(d), axis=1)
    best = np.abs(d)[np.arange(len(normals)), at]
    ok = best >= np.cos(tol)
    sign = np.where(d[np.arange(len(normals)), at] < 0, -1.0, 1.0)
    soft = (best[ok] - np.cos(tol)) / (1.0 - np.cos(tol))  # 1 - (deviation / tol)^2, nearly
    return np.where(ok, at, -1), sign, int(ok.sum()), float(soft.sum())


def votes(ang, phase_angles, family, n_families, tol):
    nb, P = ang.shape[0], phase_angles.shape[0]
    out = np.zeros((nb, n_families), dtype=np.int64)
    distinct = ~np.eye(P, dtype=bool)
    for i, j, k in itertools.combinations(range(nb), 3):
        pq = (np.abs(phase_angles - ang[i, j]) < tol) & distinct
        pr = (np.abs(phase_angles - ang[i, k]) < tol) & distinct
        qr = (np.abs(phase_angles - ang[j, k]) < tol) & distinct
        hits = pq[:, :, None] & pr[:, None, :] & qr[None, :, :]
        p, q, r = np.nonzero(hits)
        for band, refl in ((i, p), (j, q), (k, r)):
            out[band] += np.bincount(family[refl], minlength=n_families)
    return out


def index(normals, n_bands, phase_normals, family, phase_angles, tol, s2d):
    """(quat, fit [deg], nmatch, indexed) of one pattern's band normals under one phase."""
    none = (np.array([1.0, 0, 0, 0]), 180.0, 0, False)
    nb = len(normals)
    if nb < MIN_MATCHES:
        return none
    raw = normals @ normals.T
    ang = np.arccos(np.clip(np.abs(raw), None, 1.0))
    n_families = int(family.max()) + 1
    v = votes(ang, phase_angles, family, n_families, tol)
    top = v.max(axis=1)
    candidate = (top[:, None] > 0) & (2 * v >= top[:, None])  # (bands, families)
    best = (0, -1.0, None)
    P = len(phase_normals)
    for i, j in itertools.combinations(range(nb), 2):
        if not ang[i, j] > MIN_PAIR:
            continue
        for p in range(P):
            if not candidate[i, family[p]]:
                continue
            for q in range(P):
                if q == p or not candidate[j, family[q]] or not abs(phase_angles[p, q] - ang[i, j]) < tol:
                    continue
                dg = float(phase_normals[p] @ phase_normals[q])
                for s in (1.0, -1.0):
                    if not abs(np.arccos(np.clip(s * dg, -1, 1)) - np.arccos(np.clip(raw[i, j], -1, 1))) < tol:
                        continue
                    R = triad(phase_normals[p], s * phase_normals[q], normals[i], normals[j])
                    if R is None:
                        continue
                    _, _, count, score = match(R, normals, phase_normals, tol)
                    if count >= MIN_MATCHES and score > best[1]:
                        best = (count, score, R)
    if best[0] < MIN_MATCHES:
        return none
    R = best[2]
    for _ in range(2):
        at, sign, count, _ = match(R, normals, phase_normals, tol)
        if count < MIN_MATCHES:
            return none
        use = at >= 0
        R = kabsch(sign[use, None] * phase_normals[at[use]], normals[use])
    at, sign, count, _ = match(R, normals, phase_normals, tol)
    if count < MIN_MATCHES:
        return none
    use = at >= 0
    dev = np.arccos(np.clip(np.abs(np.sum((phase_normals[at[use]] @ R.T) * normals[use], axis=1)), None, 1.0))
    return om2qu(R.T @ s2d), float(np.degrees(dev.mean())), count, True


def triad(a1, a2, b1, b2):
    ea2, eb2 = np.cross(a1, a2), np.cross(b1, b2)
    na, nb = np.linalg.norm(ea2), np.linalg.norm(eb2)
    if not (na > 0 and nb > 0):
        return None
    ea2, eb2 = ea2 / na, eb2 / nb
    ea, eb = np.stack([a1, ea2, np.cross(a1, ea2)]), np.stack([b1, eb2, np.cross(b1, eb2)])
    return eb.T @ ea


def index_pattern(pattern, indexer, pc, wrong=None):
    """The whole pipeline on the CPU for one pattern and the indexer's first phase: (quat, fit, nmatch, indexed, bands)."""
    plan = indexer.bandDetectPlan
    ny, nx = plan.patDim
    cos_sin, wt, wr, rim = plan.tables()
    g = geometry(ny, nx, plan.nTheta, plan.nRho, wrong)
    b, _ = bands(radon(pattern, g, cos_sin), g, wt, wr, rim, plan.nBands, wrong)
    b = b[b["valid"] != 0]
    normals = band_normals(b["theta"], b["rho"], pc, ny, nx, wrong)
    phase = indexer.phaselist[0]
    tol = indexer.tolerance(pc)
    return index(normals, plan.nBands, phase.normals, phase.family, phase.angles, tol, indexer.sample_to_detector) + (b,)
