"""The projection kernel (csrc/projection.h `project_pixel`, csrc/project.hip `project_kernel`) read out in float64 at
the places where its hand-written arithmetic can go wrong - poles, equator, diagonals, the arctan seam, the last row
and column of the master pattern, the 4096-pixel boundary between its two paths, every master-pattern and output
dtype - against the long-double restatement of the reference's formulas in tests/_projection_cases.py, which also
says where the tolerance `4 * FLOOR[class][npx] + 8 ulp` comes from.  tests/test_host_projection.py shows on the CPU
that these comparisons reject a wrong polynomial coefficient, a moved seam, `z > 0`, swapped rows and columns, a
wrapping edge and a reciprocal-gain rescale."""

import numpy as np
import pytest

import _projection_cases as pc
from oracle import kpdi_oracle as ko

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pc.HAVE_LD, reason="np.longdouble has no 64-bit mantissa here")]


@pytest.fixture(scope="module")
def ctx():
    from kikuchipy_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def readout(ctx, probes, upper, lower=None, rotations=pc.IDENTITY, **kwargs):
    ctx.set_master_pattern(upper, lower)
    ctx.set_direction_cosines(probes)
    return ctx.project_patterns(rotations, dtype_out=np.float64, **kwargs)


@pytest.mark.parametrize("npx", pc.NPX)
def test_probe_readout(ctx, npx):
    """Every probe class through the row ramp, the column ramp and a random master pattern (the `lattice` class reads
    mp[r][c] there: rows against columns, the hemisphere offset, the padded last row and column of the packed
    layout), and the equator through the 'moat'.  Equator and pole probes name their hemisphere exactly."""
    failures = []
    for kind, name, p, up, lo in pc.readout_cases(npx):
        got = readout(ctx, p, up, lo)
        want = pc.project_ld(pc.IDENTITY, p, up, lo)
        try:
            pc.check_values(got, want, name, npx, kind)
            if kind in ("row", "col") and name in ("equator", "poles"):
                assert np.array_equal(got >= 500, want >= 500), f"{kind} {name} npx={npx}: hemisphere"
        except AssertionError as err:
            failures.append(str(err))
    assert not failures, "\n".join(failures)


def test_every_lattice_node(ctx):
    """All 401 x 401 nodes of the upper hemisphere and the inner ones of the lower: the kernel returns mp[r][c] of a
    random master pattern (`project_ld` is within 2e-15 npx of it: tests/test_host_projection.py)."""
    npx = 401
    p = pc.lattice(npx, every_node=True)[0]
    r, c, h = pc.lattice_nodes(npx, every_node=True)
    up, lo = pc.masters("random", npx)
    want = np.where(h > 0, up[r, c], lo[r, c]).astype(pc.LD)[None]
    got = readout(ctx, p, up, lo)
    assert not np.isnan(got).any()
    ratio = float((np.abs(got - want) / (pc.tolerance("lattice", npx, want) + 2e-15 * npx)).max())
    print(f"every node lattice npx={npx}: worst error / tolerance = {ratio:.3g}")
    assert ratio <= 1


def test_master_pattern_dtypes(ctx):
    """uint8, uint16, float32 and float64 master patterns are held as the same float32 values: identical readouts.
    One hemisphere alone is both."""
    p = np.concatenate([f()[0] for f in pc.FIXED_CLASSES])
    for npx, offset, dtypes in ((11, 100, (np.uint8, np.uint16, np.float32, np.float64)),
                                (401, 1000, (np.uint16, np.float32, np.float64))):  # values beyond 255
        for kind in ("row", "col"):
            up, lo = pc.masters(kind, npx, offset)
            outs = [readout(ctx, p, up.astype(t), lo.astype(t)) for t in dtypes]
            pc.check_values(outs[0][:, -4096:], pc.project_ld(pc.IDENTITY, p[-4096:], up, lo), "generic", npx, f"{kind} {dtypes[0].__name__}")
            for t, out in zip(dtypes[1:], outs[1:]):
                assert np.array_equal(out, outs[0]), f"{kind} npx={npx}: {t.__name__} differs from {dtypes[0].__name__}"
            for t in dtypes:
                assert np.array_equal(readout(ctx, p, up.astype(t)), readout(ctx, p, up.astype(t), up.astype(t)))


def test_rotations(ctx):
    """The generic probes under unit quaternions, one with a < 0, a half turn about x (upper <-> lower), a quarter
    turn about z and quaternions of length 0.5 and 2, which the reference does not normalise."""
    p = pc.generic()[0]
    q = pc.rotation_set()
    up, lo = pc.masters("random", 401)
    left_out = pc.near_equator(q, p)
    assert left_out.sum() == 0
    pc.check_values(readout(ctx, p, up, lo, q), pc.project_ld(q, p, up, lo), "generic", 401, "rotations")


@pytest.fixture(scope="module")
def prefixes():
    p, q, polar = pc.path_boundary_case()
    up, lo = pc.masters("random", 401)
    return p, q, up, lo, pc.project_ld(q, p, up, lo), polar


@pytest.mark.parametrize("npix", [1, 63, 512, 513, 4095, 4096, 4097, 5000])
def test_path_boundary_and_tails(ctx, prefixes, npix):
    """Register-resident up to 4096 pixels, recompute above, a partial last slot in each; without rescale and with.
    Five of the 3 x 5000 rotated probes come closer to a pole than any generic probe (1 - |z| down to 9e-6, where
    float64 + libm itself is ten generic floors off) and are judged by four times what float64 + libm loses at those
    very directions, FLOOR["path_boundary_near_pole"] (tests/test_host_projection.py::test_directions_near_the_pole).

    Tolerance of a rescaled value r = (v - lo) / (hi - lo) * 2 - 1 when v, lo and hi each carry an error up to t (the
    unscaled tolerance): |dr| <= g (|dv| + |dlo|) + (v - lo) / (hi - lo) g (|dhi| + |dlo|) <= 4 g t with
    g = 2 / (hi - lo), plus the 8 ulp of the arithmetic at magnitude 1."""
    p, q, up, lo, ld, polar = prefixes
    assert polar.sum() == 5
    want, polar = ld[:, :npix], polar[:, :npix]
    got = readout(ctx, p[:npix], up, lo, q)
    pc.check_values(got[~polar], want[~polar], "generic", 401, f"npix={npix}")
    pc.check_values(got[polar], want[polar], "path_boundary_near_pole", 401, f"npix={npix}")
    got = readout(ctx, p[:npix], up, lo, q, rescale=True, out_min=-1, out_max=1)
    if npix == 1:  # the reference divides 0 by 0
        assert np.isnan(got).all()
        return
    assert not np.isnan(got).any()
    gain = 2 / (want.max(axis=1, keepdims=True) - want.min(axis=1, keepdims=True))
    tol = 4 * gain * pc.tolerance("generic", 401, want).max() + 8 * np.spacing(1.0)
    ratio = float((np.abs(got - pc.rescale_ld(want, -1, 1)) / tol).max())
    print(f"npix={npix} rescaled: worst error / tolerance = {ratio:.3g}")
    assert ratio <= 1
    assert (got.min(axis=1) == -1).all() and (got.max(axis=1) == 1).all()


@pytest.mark.parametrize("shape", [(5, 7), (70, 90)])
def test_varying_pc(ctx, shape):
    """Direction cosines formed on the device from one PC per pattern (register-resident and recompute path) against
    `project_ld` fed with the oracle's direction cosines; float64 within the generic tolerance, float32 within one
    float32 ulp of the value.  The third pattern of the larger detector looks down the pole: the few pixels closer to
    it than any generic probe (1 - |z| down to 2e-5, where 1 - |z| cancels and float64 + libm itself is four generic
    floors off) are judged by four times what float64 + libm loses at those very pixels,
    FLOOR["varying_pc_near_pole"] (tests/test_host_projection.py::test_directions_near_the_pole)."""
    q, pcs, om, dcs, polar = pc.varying_pc_case(shape)
    assert polar.sum() == (0 if shape == (5, 7) else 6)  # the generic tolerance judges all the others
    for kind in ("row", "col"):
        up, lo = pc.masters(kind, 401)
        want = np.concatenate([pc.project_ld(q[i:i + 1], dcs[i], up, lo) for i in range(3)])
        ctx.set_master_pattern(up, lo)
        got = ctx.project_patterns_varying_pc(q, pcs, shape, om, dtype_out=np.float64)
        pc.check_values(got[~polar], want[~polar], "generic", 401, f"varying PC {shape} {kind}")
        pc.check_values(got[polar], want[polar], "varying_pc_near_pole", 401, f"varying PC {shape} {kind}")
        got = ctx.project_patterns_varying_pc(q, pcs, shape, om, dtype_out=np.float32)
        assert got.dtype == np.float32
        assert (np.abs(got.astype(pc.LD) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


@pytest.mark.parametrize("npix", pc.INT_NPIX)
@pytest.mark.parametrize("dtype,out_max", [(np.uint8, 255), (np.uint16, 65535)])
def test_integer_outputs_rescaled(ctx, dtype, out_max, npix):
    """64 patterns: each has the minimum 0 and the maximum out_max exactly (the reference divides by hi - lo, so its
    brightest pixel is 1 * out_max), every other pixel is the truncated long-double value."""
    q, p, up, lo, ld = pc.integer_case()
    ctx.set_master_pattern(up, lo)
    ctx.set_direction_cosines(p[:npix])
    got = ctx.project_patterns(q, True, 0, out_max, dtype)
    assert got.dtype == dtype
    pc.check_integer_patterns(got, pc.rescale_ld(ld[:, :npix], 0, out_max), 0, out_max, f"{dtype.__name__} npix={npix}")


@pytest.mark.parametrize("npix", [63, 600, 3600, 4100])
def test_extreme_at_the_last_pixel(ctx, npix):
    """The register-resident path computes the last pixel once more in every slot beyond it, and the recompute path
    every pixel twice: the brightest (darkest) pixel must still be exactly out_max (out_min) when it is the last."""
    q, p, up, lo, ld = pc.integer_case()
    ctx.set_master_pattern(up, lo)
    for n in range(4):
        for pick in (np.argmax, np.argmin):
            order = np.arange(npix)
            k = pick(ld[n, :npix])
            order[[k, npix - 1]] = order[[npix - 1, k]]
            ctx.set_direction_cosines(p[:npix][order])
            got = ctx.project_patterns(q[n:n + 1], True, 0, 255, np.uint8)
            assert (got.min(), got.max(), got[0, -1]) == (0, 255, 255 if pick is np.argmax else 0)
            got = ctx.project_patterns(q[n:n + 1], True, -1, 1, np.float64)
            assert (got.min(), got.max(), got[0, -1]) == (-1, 1, 1 if pick is np.argmax else -1)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_integer_outputs_truncate(ctx, dtype):
    """Without rescale, on a master pattern with values in [0, 250]."""
    q, p = pc.integer_case()[:2]
    up, lo, ld = pc.integer_case_plain()
    ctx.set_master_pattern(up, lo)
    for npix in pc.INT_NPIX:
        ctx.set_direction_cosines(p[:npix])
        got = ctx.project_patterns(q, dtype_out=dtype)
        assert got.dtype == dtype
        pc.check_integer_patterns(got, ld[:, :npix], label=f"{dtype.__name__} npix={npix} no rescale")
