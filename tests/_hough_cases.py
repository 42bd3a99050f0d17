"""Inputs and bounds of the Hough indexing tests: seeded simulated Ni patterns, the reference's nine
experimental Ni patterns, hand-made sinograms and band normals, and the host program that runs csrc/hough_plan.h and
csrc/hough_vote.h under the host compiler.  Shared by tests/test_host_hough.py, tests/test_gpu_hough.py and
tests/test_gpu_hough_workflow.py."""

import os
import shutil
import subprocess

import numpy as np

import kikuchipy_amd as kpa
from kikuchipy_amd.indexing._refinement import rotation_from_euler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kikuchipy_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
POINT_GROUP = "m-3m"  # Ni; the default reflectors {111}, {200}, {220}, {311}
SIMULATED_SHAPES = ((60, 60), (96, 80), (120, 120))
N_SIMULATED = 12
WRONG = ("rho_not_flipped", "y_not_negated", "half_pixel")


def cell_bound(pcz, ny):
    """One rho cell seen from the source point, in degrees: 1.91 at 60 rows and PCz = 0.5, 0.95 at 120."""
    return float(np.degrees(np.arctan(1.0 / (pcz * ny))))


# ---- simulated patterns ---------------------------------------------------------------------------------------------------
def master_pattern():
    g = np.load(os.path.join(GOLDEN, "projection.npz"))
    return g["mp_upper"].astype(np.float32), g["mp_lower"].astype(np.float32)


def simulated_inputs(shape):
    """(rotations (12, 4) with a >= 0, PCs (12, 3)) of a detector shape: seeded by the shape."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    q = rng.standard_normal((N_SIMULATED, 4))
    q /= np.sqrt(np.sum(q * q, axis=1))[:, None]
    q = np.where(q[:, :1] < 0, -q, q)
    pcs = np.array([0.42, 0.22, 0.5]) + 0.02 * (rng.random((N_SIMULATED, 3)) - 0.5)
    return q, pcs


def simulated_patterns_host(shape):
    """The patterns of `simulated_inputs` projected on the CPU by the oracle: (12, ny, nx) float32."""
    from oracle import kpdi_oracle as ko

    q, pcs = simulated_inputs(shape)
    mpu, mpl = master_pattern()
    return np.stack([ko.project_patterns(q[i:i + 1], ko.detector_direction_cosines(shape, tuple(pcs[i])), mpu, mpl).reshape(shape)
                     for i in range(N_SIMULATED)]).astype(np.float32)


def indexer(shape, pc, **kwargs):
    return kpa.EBSDDetector(shape, pc=pc).get_indexer(POINT_GROUP, **kwargs)


# ---- the reference's nine experimental Ni patterns ----------------------------------------------------------------------------
def ni_experimental():
    """(patterns (3, 3, 60, 60) uint8, static background, PCs (9, 3), orientations (9, 4)) - the orientations are those of
    the `CrystalMap` stored with the patterns, committed as Bunge angles in tests/golden/hough_ni.npz."""
    d = np.load(os.path.join(GOLDEN, "h5ebsd_expected.npz"))
    e = np.load(os.path.join(GOLDEN, "hough_ni.npz"))
    truth = rotation_from_euler(np.stack([e["phi1"], e["Phi"], e["phi2"]], axis=1))
    return d["scan1"], d["static_background"], d["pc1"], truth


# ---- hand-made inputs ---------------------------------------------------------------------------------------------------------
def drawn_line(shape, theta_deg, rho, width=1.5):
    """An image of one bright line cos(theta) (j - cx) + sin(theta) (i - cy) = rho with a Gaussian profile: uint8."""
    ny, nx = shape
    i, j = np.mgrid[0:ny, 0:nx]
    t = np.deg2rad(theta_deg)
    d = np.cos(t) * (j - (nx - 1) / 2) + np.sin(t) * (i - (ny - 1) / 2) - rho
    return np.round(20 + 200 * np.exp(-0.5 * (d / width) ** 2)).astype(np.uint8)


def radon_patterns(shape, dtype, n=2, seed=3):
    rng = np.random.default_rng(seed + shape[0])
    if np.dtype(dtype).kind == "f":
        return (rng.random((n,) + tuple(shape)) * 100 - 20).astype(dtype)
    return rng.integers(0, np.iinfo(dtype).max, (n,) + tuple(shape), endpoint=True).astype(dtype)


def sinogram_cases(n_theta=24, n_rho=21):
    """Hand-made sinograms for the band detection: name -> (S, what must come out).  Cell values are small integers, so
    every smoothed value is exact whatever the order."""
    z = np.zeros((n_theta, n_rho), dtype=np.float32)
    out = {}
    s = z.copy()
    s[0, 6] = 64  # on the seam: its window reaches row n_theta - 1 at the flipped rho
    s[n_theta - 1, n_rho - 1 - 6] = 64  # the same height across the seam, one cell away: a tie -> the lower index wins
    out["seam_tie"] = s
    s = z.copy()
    s[5:8, 8:11] = 32  # a plateau: one band, its first cell
    out["plateau"] = s
    s = z.copy()
    s[3, 5], s[12, 14] = 48, 16  # fewer maxima than bands
    out["two_peaks"] = s
    s = z.copy()
    s[10, 0], s[10, n_rho - 1], s[10, 10] = 200, 200, 8  # the rim holds no band
    out["rim"] = s
    return out


def synthetic_normals(seed=7, n_true=6, n_false=3):
    """(band normals in the detector frame, the rotation om they were made with): `n_true` reflectors of the default Ni
    phase seen through a seeded rotation and an untilted frame, with seeded outliers in between."""
    from _geometrical_cases import to_matrix

    rng = np.random.default_rng(seed)
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    q = -q if q[0] < 0 else q
    phase = indexer((60, 60), (0.5, 0.5, 0.5)).phaselist[0]
    pick = rng.choice(len(phase.normals), n_true, replace=False)
    s2d = kpa.EBSDDetector((60, 60)).sample_to_detector
    true = (phase.normals[pick] @ (to_matrix(q[None])[0] @ s2d.T)) * rng.choice([-1.0, 1.0], n_true)[:, None]
    false = rng.standard_normal((n_false, 3))
    false /= np.linalg.norm(false, axis=1)[:, None]
    normals = np.concatenate([true, false])[rng.permutation(n_true + n_false)]
    return normals, q, phase, s2d


# ---- the headers under the host compiler --------------------------------------------------------------------------------------
PROBE = r"""
#include <cstdio>
#include <vector>
#include "hough_plan.h"
#include "hough_vote.h"
using namespace kpdi;
template <typename T> std::vector<T> rd(FILE *f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) exit(2); return v; }
int main(int argc, char **argv) {
  FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
  if (!in || !out) return 3;
  if (argv[1][0] == 'b') {  // staged pattern -> sinogram, smoothed sinogram, bands
    auto h = rd<int32_t>(in, 8);
    const int ny = h[0], nx = h[1], nt = h[2], nr = h[3], nb = h[4];
    HoughGeom g = hough_geom(ny ? ny : 60, ny ? nx : 60, nt, nr);
    HoughSmooth w{};
    w.rt = h[5], w.rr = h[6], w.rim = h[7];
    // ny == 0: the input is a sinogram, not a staged pattern
    auto p = rd<float>(in, ny ? (size_t)ny * nx : (size_t)nt * nr), cs = rd<float>(in, 2 * nt), wt = rd<float>(in, 2 * w.rt + 1), wr = rd<float>(in, 2 * w.rr + 1);
    for (size_t i = 0; i < wt.size(); ++i) w.wt[i] = wt[i];
    for (size_t i = 0; i < wr.size(); ++i) w.wr[i] = wr[i];
    const int cells = nt * nr;
    std::vector<float> s(cells), tmp(cells), u(cells);
    for (int o = 0; o < cells; ++o) s[o] = ny ? hough_line_sum(p.data(), g, cs[o / nr], cs[nt + o / nr], o % nr) : p[o];
    for (int o = 0; o < cells; ++o) tmp[o] = hough_smooth_rho(s.data(), g, w, o / nr, o % nr);
    for (int o = 0; o < cells; ++o) u[o] = hough_smooth_theta(tmp.data(), g, w, o / nr, o % nr);
    std::vector<HoughBand> bands;
    float lv = INFINITY; int li = -1;
    for (int b = 0; b < nb; ++b) {
      float v = 0; int at = -1;
      for (int o = 0; o < cells; ++o) {
        if (!hough_is_peak(u.data(), g, w, o / nr, o % nr) || !hough_before(lv, li, u[o], o)) continue;
        if (at < 0 || hough_before(u[o], o, v, at)) { v = u[o]; at = o; }
      }
      if (at < 0) { bands.push_back(HoughBand{0, 0, 0, 0, -1, -1, 0, 0}); continue; }
      bands.push_back(hough_band_at(u.data(), g, at / nr, at % nr));
      lv = v; li = at;
    }
    int32_t n_mask = g.n_mask;
    fwrite(&n_mask, 4, 1, out);
    fwrite(s.data(), 4, cells, out);
    fwrite(u.data(), 4, cells, out);
    fwrite(bands.data(), sizeof(HoughBand), nb, out);
  } else if (argv[1][0] == 'v') {  // band normals -> votes and the indexed orientation
    auto h = rd<int32_t>(in, 4);
    const int nb = h[0], P = h[1], nf = h[2], asked = h[3];
    auto tol = rd<double>(in, 1), s2d = rd<double>(in, 9), n = rd<double>(in, 3 * nb), g = rd<double>(in, 3 * P), ang = rd<double>(in, (size_t)P * P);
    auto fam = rd<int32_t>(in, P);
    HvPhase ph{P, nf, g.data(), fam.data(), ang.data(), tol[0]};
    HvDetector det{60, 60, {}};
    for (int k = 0; k < 9; ++k) det.s2d[k] = s2d[k];
    double bands[HV_MAX_BANDS][3];
    for (int i = 0; i < nb; ++i) for (int k = 0; k < 3; ++k) bands[i][k] = n[3 * i + k];
    double a[HV_MAX_BANDS][HV_MAX_BANDS];
    for (int i = 0; i < nb; ++i) for (int j = 0; j < nb; ++j) a[i][j] = hv_acos(fabs(hv_dot(bands[i], bands[j])));
    int votes[HV_MAX_BANDS][HV_MAX_FAMILIES];
    hv_vote(a, nb, ph, votes);
    const HvResult r = hv_index(bands, nb, asked, ph, det);
    for (int i = 0; i < nb; ++i) fwrite(votes[i], 4, nf, out);
    fwrite(r.quat, 8, 4, out);
    fwrite(&r.fit, 8, 1, out);
    fwrite(&r.nmatch, 4, 1, out);
    fwrite(&r.indexed, 4, 1, out);
  } else {  // band (theta, rho) under a PC -> its normal
    auto v = rd<double>(in, 5);
    auto d = rd<int32_t>(in, 2);
    double n[3];
    hv_band_normal(v[0], v[1], v.data() + 2, d[0], d[1], n);
    fwrite(n, 8, 3, out);
  }
  fclose(out);
  return 0;
}
"""


def build_probe(tmp):
    """The probe program, or None without a host C++ compiler."""
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        return None
    src, exe = os.path.join(tmp, "hough_probe.cpp"), os.path.join(tmp, "hough_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, src, "-o", exe], check=True)
    return exe


def run_probe(exe, mode, tmp, parts):
    fin, fout = os.path.join(tmp, "probe.in"), os.path.join(tmp, "probe.out")
    with open(fin, "wb") as f:
        for part in parts:
            f.write(np.ascontiguousarray(part).tobytes())
    subprocess.run([exe, mode, fin, fout], check=True)
    with open(fout, "rb") as f:
        return f.read()


def probe_bands(exe, tmp, data, n_theta, n_rho, n_bands, cos_sin, wt, wr, rim, sinogram=False):
    """(n_mask, sinogram, smoothed sinogram, bands) through the header's functions, of a staged float32 pattern `data`
    (ny, nx), or - `sinogram` - of a sinogram `data` (n_theta, n_rho) taken as it is."""
    from kikuchipy_amd import _lib

    ny, nx = (0, 0) if sinogram else data.shape
    head = np.array([ny, nx, n_theta, n_rho, n_bands, len(wt) // 2, len(wr) // 2, rim], dtype=np.int32)
    raw = run_probe(exe, "b", tmp, [head, data.astype(np.float32), cos_sin.astype(np.float32), wt, wr])
    cells = n_theta * n_rho
    n_mask = int(np.frombuffer(raw, np.int32, 1)[0])
    s = np.frombuffer(raw, np.float32, cells, 4).reshape(n_theta, n_rho)
    u = np.frombuffer(raw, np.float32, cells, 4 + 4 * cells).reshape(n_theta, n_rho)
    b = np.frombuffer(raw, _lib.HOUGH_BAND_DTYPE, n_bands, 4 + 8 * cells)
    return n_mask, s, u, b


def probe_index(exe, tmp, normals, phase, tol, s2d, asked=9):
    """(votes (bands, families), quat, fit, nmatch, indexed) of band normals through the header's functions."""
    nb, P, nf = len(normals), len(phase.normals), int(phase.family.max()) + 1
    raw = run_probe(exe, "v", tmp, [np.array([nb, P, nf, asked], dtype=np.int32), np.array([tol]), np.asarray(s2d, dtype=np.float64),
                                    np.asarray(normals, dtype=np.float64), phase.normals, phase.angles, phase.family])
    votes = np.frombuffer(raw, np.int32, nb * nf).reshape(nb, nf)
    o = 4 * nb * nf
    return (votes, np.frombuffer(raw, np.float64, 4, o), float(np.frombuffer(raw, np.float64, 1, o + 32)[0]),
            int(np.frombuffer(raw, np.int32, 1, o + 40)[0]), bool(np.frombuffer(raw, np.int32, 1, o + 44)[0]))


def probe_normal(exe, tmp, theta, rho, pc, shape):
    raw = run_probe(exe, "n", tmp, [np.array([theta, rho, *pc], dtype=np.float64), np.array(shape, dtype=np.int32)])
    return np.frombuffer(raw, np.float64, 3)
