"""Orientation sampling for dictionaries: `get_sample_fundamental(resolution, point_group)`.

The reference builds its dictionaries from `orix.sampling.get_sample_fundamental(resolution=..., point_group=...)`
(benchmarks/indexing/test_dictionary_indexing.py:37; doc/tutorials/pattern_matching.ipynb cell 8:
`method="cubochoric", resolution=3, point_group=ni.point_group`).  orix (>= 0.12.1, pyproject.toml:54) is a third-party
dependency that is neither vendored in the reference nor installed here; this module restates the published algorithm
behind that call - cubochoric sampling of SO(3), Rosca, Morawiec & De Graef, Modelling Simul. Mater. Sci. Eng. 22 (2014)
075013; Singh & De Graef, ibid. 24 (2016) 085013 - for the cases the reference uses:

  * a cubic grid of (2 n + 1)^3 points over the cube of semi-edge pi^(2/3) / 2, n = round(131.97049 / (resolution -
    0.03732)) (the grid INCLUDES the cube's surface), in lexicographic order (x slowest) - the order the dictionary is
    emitted in;
  * cube -> homochoric ball (the volume-preserving Lambert-type map) -> axis-angle -> unit quaternion (a, b, c, d), a >= 0;
  * kept where the Rodrigues vector lies in the fundamental zone of the point group's proper subgroup - 432 for
    m-3m / 432: |r_i| <= sqrt(2) - 1 and |r_1| + |r_2| + |r_3| <= 1.

Every other rotation group (1, 2, 222, 4, 422, 3, 32, 6, 622, 23, 432 and, by their proper subgroup, the eleven Laue
groups) goes through one rule that needs nothing but the group's proper operations, generated from their generators:
every non-identity operation with unit axis a and smallest angle w in (0, pi] about it bounds the zone by the face pair
|r . a| <= tan(w / 4) - the Voronoi cell of the identity among the group's elements, closed.  It is evaluated on the
quaternion, |q_v . a| <= tan(w / 4) q_0 + 1e-9, so that w = pi needs no infinity.  Settings: the n-fold axis along z,
the first two-fold axis of the dihedral groups along x (a || x; 32 in its 321 setting), 23 and 432 on the cube axes.
The four names above keep their own code path, so what the benchmarks and the reference's known answer rest on does
not move by a bit.  The ten non-centrosymmetric groups with improper operations are refused: orix would sample their
proper subgroup, an EBSD pattern distinguishes their Laue class, and the caller has to say which rotation group is meant.

With `device=` or `context=` the sampler runs as a kernel (csrc/sampling.hip, csrc/sampling_plan.h; DESIGN.md section
23): the same grid in the same order for all 22 names, every name through the face rule.

Pinned by what the reference itself holds for this path: 30 443 orientations at `resolution=3` (the tutorial's printed
`Rotation (30443,)`) and the benchmark's known answer - nine Ni patterns against the 3557-orientation dictionary of
`resolution=6`: `scores.mean() = 0.1887 +- 1e-4` (tests/test_reference_benchmark.py, CPU through the oracle and GPU through
the engine)."""

import numpy as np

_SEMI_EDGE = np.pi ** (2 / 3) / 2


def resolution_to_semi_edge_steps(resolution):
    """Grid points per semi-edge of the cubochoric cube for an average disorientation of `resolution` degrees between
    neighbouring samples (EMsoft's fit, as orix uses it)."""
    if not resolution > 0.03732:
        raise ValueError("resolution must be positive (degrees)")
    return int(np.round(131.97049 / (resolution - 0.03732)))


def cubochoric_to_homochoric(xyz):
    """(N, 3) points of the cube [-pi^(2/3)/2, pi^(2/3)/2]^3 -> the ball of radius (3 pi / 4)^(1/3), volume preserving
    (Rosca et al. 2014, eqs. 2-4: scale the cube, map each square pyramid to a curved one, inverse Lambert projection)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    pyramid = np.argmax(np.abs(xyz), axis=1)  # the axis of largest magnitude goes last
    order = np.array([[1, 2, 0], [2, 0, 1], [0, 1, 2]])[pyramid]
    x, y, z = (np.pi ** (5 / 6) / 6 ** (1 / 6) / np.pi ** (2 / 3) * np.take_along_axis(xyz, order, axis=1)).T
    r1, beta = (3 * np.pi / 4) ** (1 / 3), np.pi ** (5 / 6) / 6 ** (1 / 6) / 2
    prek, sr2 = r1 * 2 ** 0.25 / beta, np.sqrt(2.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        flat = np.abs(y) <= np.abs(x)
        q = np.where(flat, np.pi / 12 * y / x, np.pi / 12 * x / y)
        q = np.where(np.isfinite(q), q, 0.0)
        c, s = np.cos(q), np.sin(q)
        qq = np.where(flat, x, y) * prek / np.sqrt(sr2 - c)
        t1 = np.where(flat, (sr2 * c - 1) * qq, sr2 * s * qq)
        t2 = np.where(flat, sr2 * s * qq, (sr2 * c - 1) * qq)
        cc = t1 * t1 + t2 * t2
        shrink = np.sqrt(np.maximum(1 - np.pi * cc / (24 * z * z), 0))
        ball = np.stack([t1 * shrink, t2 * shrink, np.sqrt(6 / np.pi) * z - np.sqrt(np.pi) * cc / np.sqrt(24) / z], axis=1)
    on_axis = np.maximum(np.abs(x), np.abs(y)) == 0
    ball[on_axis] = np.stack([np.zeros(on_axis.sum()), np.zeros(on_axis.sum()), np.sqrt(6 / np.pi) * z[on_axis]], axis=1)
    ball[~np.isfinite(ball).all(axis=1)] = 0.0  # (the cube's centre)
    return np.take_along_axis(ball, np.argsort(order, axis=1), axis=1)


def homochoric_to_axis_angle(ho):
    """|ho| = (3/4 (w - sin w))^(1/3): (unit axes (N, 3), angles w in [0, pi]); bisection, exact to float64."""
    h = np.linalg.norm(ho, axis=1)
    lo, hi = np.zeros_like(h), np.full_like(h, np.pi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        below = (0.75 * (mid - np.sin(mid))) ** (1 / 3) < h
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    axis = np.divide(ho, h[:, None], out=np.zeros_like(ho), where=h[:, None] > 0)
    return axis, 0.5 * (lo + hi)


_FUNDAMENTAL_ZONES = {"m-3m": "432", "432": "432", "1": "1", "-1": "1"}

# Every rotation group, its Laue group, and the generators of the rotation group as unit quaternions: the n-fold axis
# along z, the first two-fold axis of the dihedral groups along x (a || x; 32 in its 321 setting), 23 and 432 on the
# cube axes (two-fold / four-fold along z, three-fold along [111]).
ROTATION_GROUPS = ("1", "2", "222", "4", "422", "3", "32", "6", "622", "23", "432")
LAUE_GROUPS = ("-1", "2/m", "mmm", "4/m", "4/mmm", "-3", "-3m", "6/m", "6/mmm", "m-3", "m-3m")
# non-centrosymmetric groups with improper operations: orix samples their proper subgroup, an EBSD pattern distinguishes
# their Laue class, and the setting of some (-6m2) cannot be pinned by the name alone
IMPROPER_GROUPS = ("m", "mm2", "-4", "4mm", "-42m", "3m", "-6", "6mm", "-6m2", "-43m")
_ROTATION_GROUP_OF = {**{g: g for g in ROTATION_GROUPS}, **dict(zip(LAUE_GROUPS, ROTATION_GROUPS))}
_TWO_FOLD_X = (0.0, 1.0, 0.0, 0.0)
_THREE_FOLD_111 = (0.5, 0.5, 0.5, 0.5)


def _n_fold_z(n):
    return (np.cos(np.pi / n), 0.0, 0.0, np.sin(np.pi / n))


_GENERATORS = {
    "1": (), "2": (_n_fold_z(2),), "222": (_n_fold_z(2), _TWO_FOLD_X), "4": (_n_fold_z(4),),
    "422": (_n_fold_z(4), _TWO_FOLD_X), "3": (_n_fold_z(3),), "32": (_n_fold_z(3), _TWO_FOLD_X), "6": (_n_fold_z(6),),
    "622": (_n_fold_z(6), _TWO_FOLD_X), "23": (_n_fold_z(2), _TWO_FOLD_X, _THREE_FOLD_111),
    "432": (_n_fold_z(4), _THREE_FOLD_111),
}


def quaternion_product(p, q):
    """Hamilton product of (..., 4) quaternions (a, b, c, d)."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    a = p[..., 0] * q[..., 0] - np.sum(p[..., 1:] * q[..., 1:], axis=-1)
    v = p[..., :1] * q[..., 1:] + q[..., :1] * p[..., 1:] + np.cross(p[..., 1:], q[..., 1:])
    return np.concatenate([a[..., None], v], axis=-1)


def rotation_group_name(point_group):
    """The rotation group whose fundamental zone is sampled for `point_group` (a name or an object with `.name`): the
    group itself for the eleven rotation groups, the proper subgroup for the eleven Laue groups.  The ten
    non-centrosymmetric groups with improper operations are refused with `ValueError`."""
    name = getattr(point_group, "name", point_group)
    if name in IMPROPER_GROUPS:
        raise ValueError(f"point group {name!r} has improper operations but no inversion centre: its proper subgroup and "
                         f"the Laue class an EBSD pattern distinguishes differ, pass the rotation group you want (one "
                         f"of {', '.join(ROTATION_GROUPS)})")
    if name not in _ROTATION_GROUP_OF:
        raise NotImplementedError(f"point group {name!r}: the rotation groups {', '.join(ROTATION_GROUPS)} and the Laue "
                                  f"groups {', '.join(LAUE_GROUPS)} have their fundamental zone restated")
    return _ROTATION_GROUP_OF[name]


def rotation_group_operations(group):
    """(order, 4) unit quaternions, a >= 0, of the proper operations of a rotation group, the identity first: the
    closure of the group's generators under the product, q and -q being one rotation."""
    ops = [np.array([1.0, 0.0, 0.0, 0.0])]
    generators = [np.array(g, dtype=np.float64) for g in _GENERATORS[group]]
    grown = True
    while grown:
        grown = False
        for p in list(ops):
            for g in generators:
                q = quaternion_product(p, g)
                if not any(abs(abs(q @ o) - 1) < 1e-9 for o in ops):
                    ops.append(q)
                    grown = True
    ops = np.array(ops)
    # one sign per rotation: a > 0, or the first non-zero component positive for the half turns
    lead = np.where(np.abs(ops) > 1e-9, np.sign(ops), 0)
    sign = np.array([row[np.flatnonzero(row)[0]] for row in lead])
    return ops * sign[:, None]


_FACES = {}  # per group, formed once (the closure of 432 takes milliseconds, a sampling call on the device as long)


def fundamental_zone_faces(group):
    """(f, 4) rows (a_x, a_y, a_z, tan(w / 4)) of the face pairs |r . a| <= tan(w / 4) that bound the Rodrigues
    fundamental zone of a rotation group: one per rotation axis, from the non-identity operation of the smallest angle
    w in (0, pi] about it (a larger angle about the same axis gives a wider, implied pair).  The zone is the Voronoi cell
    of the identity among the group's elements.  tan(w / 4) = |q_v| / (1 + q_0) needs no trigonometric call."""
    if group in _FACES:
        return _FACES[group].copy()
    faces = {}
    for q in rotation_group_operations(group)[1:]:
        s = np.linalg.norm(q[1:])
        a = q[1:] / s
        a = a * np.sign(a[np.flatnonzero(np.abs(a) > 1e-9)[0]])
        key = tuple(np.round(a, 9) + 0.0)
        t = s / (1 + q[0])
        if key not in faces or t < faces[key][3]:
            faces[key] = np.append(a, t)
    _FACES[group] = np.array([faces[k] for k in sorted(faces)]).reshape(-1, 4)
    return _FACES[group].copy()


FACE_SLACK = 1e-9  # the zone is closed: a point on a face is kept whatever its last bits are


def in_fundamental_zone(quaternions, faces):
    """The face rule in quaternion form (w = pi needs no infinity): q = (q_0 >= 0, q_v) is kept iff
    |q_v . a| <= tan(w / 4) q_0 + 1e-9 for every face."""
    q = np.asarray(quaternions, dtype=np.float64)
    keep = np.ones(q.shape[0], dtype=bool)
    for a0, a1, a2, t in faces:
        keep &= np.abs(q[:, 1] * a0 + q[:, 2] * a1 + q[:, 3] * a2) <= t * q[:, 0] + FACE_SLACK
    return keep


def get_sample_fundamental(resolution=2, point_group="m-3m", method="cubochoric", semi_edge_steps=None, *, device=None,
                           context=None):
    """(N, 4) unit quaternions (a, b, c, d), a >= 0, sampling the Rodrigues fundamental zone of `point_group` with an
    average disorientation of `resolution` degrees, in the sampler's (lexicographic) order.

    `point_group`: a name or an object with a `.name` (an orix `Symmetry`).  The rotation groups 1, 2, 222, 4, 422, 3,
    32, 6, 622, 23 and 432 name themselves; the Laue groups -1, 2/m, mmm, 4/m, 4/mmm, -3, -3m, 6/m, 6/mmm, m-3 and m-3m
    map to them in that order ("1" = all of SO(3)).  Settings: the n-fold axis is along z; the first two-fold axis of
    the dihedral groups is along x (a || x; 32 in its 321 setting); 23 and 432 are on the cube axes.  The ten
    non-centrosymmetric groups with improper operations (m, mm2, -4, 4mm, -42m, 3m, -6, 6mm, -6m2, -43m) raise
    `ValueError`: pass the rotation group you want.

    With neither `device` nor `context` the sampler runs on the host.  `device` (a GPU's number) or `context` (a
    `Context`) runs it as a kernel (csrc/sampling.hip): the same grid points in the same order, every name through the
    one face rule."""
    if method != "cubochoric":
        raise NotImplementedError("only the cubochoric sampling of the reference's benchmark and tutorial is restated")
    name = getattr(point_group, "name", point_group)
    generic = name not in _FUNDAMENTAL_ZONES  # the four names of the reference's benchmark and tutorial keep their path
    group = rotation_group_name(name)
    n = int(semi_edge_steps) if semi_edge_steps is not None else resolution_to_semi_edge_steps(resolution)
    if n < 1:
        raise ValueError(f"semi_edge_steps {n}: at least one step per semi-edge")
    if device is not None or context is not None:
        from kikuchipy_amd import _lib

        ctx = context if context is not None else _lib.Context(device)
        try:
            return ctx.sample_fundamental(n, fundamental_zone_faces(group))
        finally:
            if context is None:
                ctx.close()
    if generic:
        faces = fundamental_zone_faces(group)
    g = np.arange(-n, n + 1) * (_SEMI_EDGE / n)
    out = []
    for x in g:  # one slab of the cube at a time: (2 n + 1)^2 points
        yy, zz = np.meshgrid(g, g, indexing="ij")
        xyz = np.column_stack([np.full(yy.size, x), yy.ravel(), zz.ravel()])
        axis, w = homochoric_to_axis_angle(cubochoric_to_homochoric(xyz))
        if generic:
            q = np.column_stack([np.cos(w / 2), axis * np.sin(w / 2)[:, None]])
            out.append(q[in_fundamental_zone(q, faces)])
            continue
        if _FUNDAMENTAL_ZONES[name] == "432":
            with np.errstate(invalid="ignore"):
                r = np.abs(axis * np.tan(w / 2)[:, None])
                keep = (r.max(axis=1) <= np.sqrt(2) - 1 + 1e-9) & (r.sum(axis=1) <= 1 + 1e-9)
            axis, w = axis[keep], w[keep]
        out.append(np.column_stack([np.cos(w / 2), axis * np.sin(w / 2)[:, None]]))
    return np.concatenate(out)
