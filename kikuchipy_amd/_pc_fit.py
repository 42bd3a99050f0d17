"""Plane fits to a grid of projection centres (PCs): what `EBSDDetector.estimate_xtilt`, `estimate_xtilt_ztilt` and
`fit_pc` compute (detectors/_fit_projection_center.py of the reference).  Host NumPy in float64,
like the rest of the detector.

The reference leans on three libraries this package does not use.  Rotations by orix become 3 x 3 matrices
(`Rotation.from_axes_angles(axis, angle) * v` turns v by `angle` about `axis`).  The homography of
scikit-image 0.18.3's `ProjectiveTransform.estimate` is the normalised direct linear transformation, restated in
`projective_matrix`.  scikit-learn's `LinearRegression` is ordinary least squares with an intercept (`linear_fit`); its
`RANSACRegressor` draws random pairs, which `robust_linear_fit` replaces by all pairs in a fixed order."""

import numpy as np


def linear_fit(x, y):
    """(slope, intercept) of the ordinary least-squares line y = slope x + intercept."""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    xm, ym = x.mean(), y.mean()
    dx = x - xm
    ssx = float(np.sum(dx * dx))
    slope = float(np.sum(dx * (y - ym)) / ssx) if ssx > 0 else 0.0  # (equal x: the minimum-norm solution)
    return slope, float(ym - slope * xm)


def _r2(y, pred):
    res, tot = float(np.sum((y - pred) ** 2)), float(np.sum((y - y.mean()) ** 2))
    if tot == 0.0:
        return 1.0 if res == 0.0 else 0.0
    return 1.0 - res / tot


def robust_linear_fit(x, y):
    """(slope, intercept, inlier mask) of a robust line through (x, y) by scikit-learn's RANSAC rules with its defaults -
    a model is the line through two points, the residual threshold is the median absolute deviation of y, a point is an
    inlier when its absolute residual is below it - run over ALL pairs (i, j), i < j, in lexicographic order instead
    of random trials: deterministic, and no pair is missed.  The pair with the most inliers wins; among equals the one
    with the higher R^2 on its inliers, then the first.  The line is fitted again to the winner's inliers."""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    threshold = float(np.median(np.abs(y - np.median(y))))
    best_n, best_score, best = 1, -np.inf, None
    for i in range(x.size - 1):
        for j in range(i + 1, x.size):
            slope, intercept = linear_fit(x[[i, j]], y[[i, j]])
            inlier = np.abs(y - (slope * x + intercept)) < threshold
            n = int(inlier.sum())
            if n == 0 or n < best_n:
                continue
            score = _r2(y[inlier], slope * x[inlier] + intercept)
            if n == best_n and not score > best_score:
                continue
            best_n, best_score, best = n, score, inlier
    if best is None:
        raise ValueError("The robust fit found no consensus set: the PCy values have a median absolute deviation of "
                         f"{threshold}, below which no pair of PCs lies")
    slope, intercept = linear_fit(x[best], y[best])
    return slope, intercept, best


def _rotation(axis, angle):
    """The matrix that turns a column vector by `angle` about the x (0) or the z (2) axis."""
    c, s = np.cos(angle), np.sin(angle)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


def fit_hyperplane(pc_centered):
    """(x_tilt, z_tilt, R, trimmed mean) of the plane through centred PCs (n, 3): the 10 % trimmed mean is removed, the
    plane's normal is the right singular vector of the smallest singular value, made to point towards the screen
    (z >= 0); x_tilt = acos(n_z), z_tilt = pi / 2 - atan2(n_y, n_x); R = Rz(-z_tilt) Rx(-x_tilt) takes [001] onto the
    normal."""
    from scipy.stats import trim_mean

    pc_centered = np.asarray(pc_centered, dtype=np.float64)
    mean = trim_mean(pc_centered, proportiontocut=0.1)
    _, _, vh = np.linalg.svd(pc_centered - mean[np.newaxis, :], full_matrices=False)
    normal = vh[2] / np.sqrt(np.sum(vh[2] * vh[2]))
    if normal[2] < 0:
        normal = -normal
    x_tilt = np.arccos(normal[2])
    z_tilt = np.pi / 2 - np.arctan2(normal[1], normal[0])
    return x_tilt, z_tilt, _rotation(2, -z_tilt) @ _rotation(0, -x_tilt), mean


def _center_and_normalize(points):
    centroid = np.mean(points, axis=0)
    rms = np.sqrt(np.sum((points - centroid) ** 2) / points.shape[0])
    if rms == 0:
        raise ZeroDivisionError
    f = np.sqrt(2) / rms
    matrix = np.array([[f, 0, -f * centroid[0]], [0, f, -f * centroid[1]], [0, 0, 1]])
    return matrix, (matrix @ np.vstack([points.T, np.ones(points.shape[0])])).T[:, :2]


def projective_matrix(src, dst):
    """The homography H (3 x 3, H[2, 2] of the normalised problem = 1) with dst ~ H (src, 1) in the least-squares sense of
    the normalised direct linear transformation: both point sets are centred and scaled to an RMS distance of sqrt(2),
    the 2 n x 9 system is solved by its last right singular vector, and the result is taken back.  Raises ValueError
    where the points span no plane."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    try:
        src_matrix, s = _center_and_normalize(src)
        dst_matrix, d = _center_and_normalize(dst)
    except ZeroDivisionError:
        raise ValueError("PC fit using the projective transform failed: all points coincide") from None
    n = s.shape[0]
    a = np.zeros((2 * n, 9))
    a[:n, 0], a[:n, 1], a[:n, 2] = s[:, 0], s[:, 1], 1
    a[:n, 6], a[:n, 7] = -d[:, 0] * s[:, 0], -d[:, 0] * s[:, 1]
    a[n:, 3], a[n:, 4], a[n:, 5] = s[:, 0], s[:, 1], 1
    a[n:, 6], a[n:, 7] = -d[:, 1] * s[:, 0], -d[:, 1] * s[:, 1]
    a[:n, 8], a[n:, 8] = d[:, 0], d[:, 1]
    _, _, v = np.linalg.svd(a)
    if np.isclose(v[-1, -1], 0):
        raise ValueError("PC fit using the projective transform failed: the map points or the PCs lie on a line, which "
                         "determines no homography; use transformation='affine'")
    h = np.zeros((3, 3))
    h.flat[:8] = -v[-1, :-1] / v[-1, -1]
    h[2, 2] = 1
    return np.linalg.inv(dst_matrix) @ h @ src_matrix


def fit_pc_affine(pc_flat, pc_indices_flat, map_indices_flat):
    matrix = np.linalg.lstsq(pc_indices_flat, pc_flat, rcond=None)[0]
    return pc_indices_flat @ matrix, map_indices_flat @ matrix


def fit_pc_projective(pc_centered_flat, pc_indices_flat, map_indices_flat):
    """Rotate the PCs into their fitted plane, estimate the homography from the map indices to the in-plane
    coordinates, project the indices through it and rotate back."""
    _, _, rot, mean = fit_hyperplane(pc_centered_flat)
    in_plane = (pc_centered_flat - mean) @ rot  # rows: R^T v
    matrix = projective_matrix(pc_indices_flat[:, :2], in_plane[:, :2]).T
    out = []
    for indices in (pc_indices_flat, map_indices_flat):
        fit = indices @ matrix
        fit /= fit[:, 2, None]
        fit[:, 2] = 0
        out.append(fit @ rot.T + mean)
    return out[0], out[1]


def fit_plane_to_pc(pc_flat, pc_indices, map_indices, is_outlier, transformation):
    """(fitted PCs at `pc_indices`, fitted PCs at `map_indices` in the map's shape + (3,), the PCs used, x_tilt,
    intercept, slope of the fitted PCy on PCz)."""
    from scipy.stats import linregress

    n_pc = pc_flat.shape[0]
    pc_indices_flat = np.column_stack((pc_indices.reshape((2, -1)).T, np.ones(n_pc)))
    map_indices_flat = map_indices.reshape((2, -1)).T
    map_indices_flat = np.column_stack((map_indices_flat, np.ones(map_indices_flat.shape[0])))
    if isinstance(is_outlier, np.ndarray):
        is_inlier = ~is_outlier.ravel()
        pc_flat, pc_indices_flat = pc_flat[is_inlier], pc_indices_flat[is_inlier]
    if transformation == "projective":
        average = np.mean(pc_flat, axis=0)
        pc_fit, pc_fit_map = fit_pc_projective(pc_flat - average, pc_indices_flat, map_indices_flat)
        pc_fit, pc_fit_map = pc_fit + average, pc_fit_map + average
    else:
        pc_fit, pc_fit_map = fit_pc_affine(pc_flat, pc_indices_flat, map_indices_flat)
    result = linregress(pc_fit[..., 2], pc_fit[..., 1])
    x_tilt = np.pi / 2 + np.arctan(result.slope)
    return pc_fit, pc_fit_map.reshape(map_indices.shape[1:] + (3,)), pc_flat, x_tilt, result.intercept, result.slope
