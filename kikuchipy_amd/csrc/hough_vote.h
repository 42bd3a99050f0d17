// hough_vote.h - indexing of the detected bands of one pattern (hough.hip, kernel 3): band normals from the pattern's
// projection centre, triplet voting against the table of interplanar angles, orientation by an orthogonal fit.  Float64,
// integer votes, pure functions: `__host__ __device__` under hipcc, plain inline functions under a host compiler
// (tests/test_host_hough.py compiles this header).  Definitions: DESIGN.md section 26.
//
// Frames: a band (theta, rho) is the line cos(theta) (x - cx) + sin(theta) (y - cy) = rho in pixels (x column, y row).
// With x = (xg + xoff) / xs, y = (-yg + yoff) / ys (gnomonic xg, yg; xoff = aspect pcx / pcz, yoff = pcy / pcz; xs, ys the
// gnomonic size of a pixel) the plane through the source point that holds the line has the normal
//   n_d ~ (cos(theta) / xs, -sin(theta) / ys, cos(theta) (xoff / xs - cx) + sin(theta) (yoff / ys - cy) - rho)
// in the detector frame, where a reflector g (crystal Cartesian, a row vector) lies along g U, U = om(q) s2d^T.
//
// Voting.  Reflectors are lines (g and -g are one), each of a family (equal |g|).  Angles between lines are folded into
// [0, pi / 2].  Every triplet of bands i < j < k votes for every ordered triple of distinct reflectors (p, q, r) whose
// three angles agree with the bands' within `tol`: one vote each for (i, family p), (j, family q), (k, family r).  A band's
// candidate families are those with at least half of its best family's votes.  Every pair of bands further apart than
// HOUGH_MIN_PAIR with a pair of candidate reflectors at the same angle (signs included) is a hypothesis: the rotation
// that takes the reflector pair onto the band pair; the bands that come within `tol` of a reflector under it are its
// matches, and with HV_MIN_MATCHES or more it is scored by their sum of (|cos dev| - cos tol) / (1 - cos tol), nearly
// 1 - (dev / tol)^2: many close matches beat more loose ones.  The first among equals wins.  The best hypothesis' matches
// are fitted (Horn's closed form, the largest eigenvector of a 4 x 4 matrix by Jacobi sweeps), matched again, and fitted
// again.  `fit` is the mean angular deviation of the matches in degrees.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define HV_HD __host__ __device__ inline
#else
#define HV_HD inline
#endif

namespace kpdi {

constexpr int HV_MAX_BANDS = 16;       // = HOUGH_MAX_BANDS
constexpr int HV_MAX_REFLECTORS = 96;  // lines of one phase
constexpr int HV_MAX_FAMILIES = 16;
constexpr int HV_MIN_MATCHES = 3;      // fewer matched bands: not indexed
constexpr double HV_MIN_PAIR = 0.17453292519943295;  // 10 degrees: band pairs closer than this span no rotation
constexpr double HV_DEGREES = 57.29577951308232;
constexpr int HV_JACOBI_SWEEPS = 16;

struct HvPhase {
  int n;                   // reflectors (lines)
  int n_families;
  const double *normals;   // [n][3] unit vectors, crystal Cartesian
  const int32_t *family;   // [n]
  const double *angles;    // [n][n] folded interplanar angles, radians (host-built)
  double tol;              // radians
};

struct HvDetector {
  int ny, nx;
  double s2d[9];           // sample to detector, row-major
};

struct HvResult {
  double quat[4];
  double fit;      // degrees; 180 when not indexed
  double cm;       // matched bands / bands
  int32_t nmatch;
  int32_t indexed;
};

HV_HD double hv_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

HV_HD void hv_cross(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

HV_HD bool hv_unit(double *v) {
  const double n = sqrt(hv_dot(v, v));
  if (!(n > 0.0) || !(n <= 1.79e308)) return false;
  v[0] /= n;
  v[1] /= n;
  v[2] /= n;
  return true;
}

HV_HD double hv_acos(double c) { return acos(c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c)); }

// the unit normal of band (theta, rho) under the projection centre pc; false when it is not finite
HV_HD bool hv_band_normal(double theta, double rho, const double *pc, int ny, int nx, double *n) {
  const double aspect = (double)nx / (double)ny;
  const double xs = aspect / pc[2] / (double)(nx - 1), ys = 1.0 / pc[2] / (double)(ny - 1);
  const double xoff = aspect * pc[0] / pc[2], yoff = pc[1] / pc[2];
  const double cx = (nx - 1) / 2.0, cy = (ny - 1) / 2.0, c = cos(theta), s = sin(theta);
  n[0] = c / xs;
  n[1] = -s / ys;
  n[2] = c * (xoff / xs - cx) + s * (yoff / ys - cy) - rho;
  return hv_unit(n);
}

// R (row-major) with R a1 = b1 and R a2 in the plane of b1, b2 on b2's side: from the triads of the two pairs
HV_HD bool hv_triad(const double *a1, const double *a2, const double *b1, const double *b2, double *R) {
  double ea[3][3], eb[3][3];
  for (int k = 0; k < 3; ++k) {
    ea[0][k] = a1[k];
    eb[0][k] = b1[k];
  }
  hv_cross(a1, a2, ea[1]);
  hv_cross(b1, b2, eb[1]);
  if (!hv_unit(ea[1]) || !hv_unit(eb[1])) return false;
  hv_cross(ea[0], ea[1], ea[2]);
  hv_cross(eb[0], eb[1], eb[2]);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[3 * r + c] = eb[0][r] * ea[0][c] + eb[1][r] * ea[1][c] + eb[2][r] * ea[2][c];
  return true;
}

HV_HD void hv_apply(const double *R, const double *v, double *out) {
  for (int r = 0; r < 3; ++r) out[r] = R[3 * r] * v[0] + R[3 * r + 1] * v[1] + R[3 * r + 2] * v[2];
}

// per band the reflector that R brings closest (|cosine| largest, the first among equals) if within tol: match[i] = its
// index or -1, sign[i] the sign of the cosine.  Returns the number of matches; *score = the sum over them of
// (|cosine| - cos tol) / (1 - cos tol)
HV_HD int hv_match(const double *R, const double (*bands)[3], int nb, const HvPhase &ph, int *match, double *sign, double *score) {
  const double cos_tol = cos(ph.tol);
  int count = 0;
  *score = 0.0;
  for (int i = 0; i < nb; ++i) {
    double best = -1.0, sg = 1.0;
    int at = -1;
    for (int p = 0; p < ph.n; ++p) {
      double v[3];
      hv_apply(R, ph.normals + 3 * p, v);
      const double d = hv_dot(v, bands[i]), ad = fabs(d);
      if (ad > best) {
        best = ad;
        at = p;
        sg = d < 0.0 ? -1.0 : 1.0;
      }
    }
    const bool ok = at >= 0 && best >= cos_tol;
    match[i] = ok ? at : -1;
    sign[i] = sg;
    if (ok) {
      ++count;
      *score += (best - cos_tol) / (1.0 - cos_tol);
    }
  }
  return count;
}

// Horn's closed form: the rotation R (row-major) that maximises sum_i b_i . (R a_i); false when the sweeps meet a NaN
HV_HD bool hv_fit(const double (*a)[3], const double (*b)[3], int n, double *R) {
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int i = 0; i < n; ++i)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) S[r][c] += a[i][r] * b[i][c];
  double N[4][4] = {{S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
                    {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
                    {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
                    {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < HV_JACOBI_SWEEPS; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        if (N[p][q] == 0.0) continue;
        const double th = (N[q][q] - N[p][p]) / (2.0 * N[p][q]);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {
          const double kp = N[k][p], kq = N[k][q];
          N[k][p] = c * kp - s * kq;
          N[k][q] = s * kp + c * kq;
        }
        for (int k = 0; k < 4; ++k) {
          const double pk = N[p][k], qk = N[q][k];
          N[p][k] = c * pk - s * qk;
          N[q][k] = s * pk + c * qk;
        }
        for (int k = 0; k < 4; ++k) {
          const double kp = V[k][p], kq = V[k][q];
          V[k][p] = c * kp - s * kq;
          V[k][q] = s * kp + c * kq;
        }
      }
  int top = 0;
  for (int k = 1; k < 4; ++k)
    if (N[k][k] > N[top][top]) top = k;
  double e[4] = {V[0][top], V[1][top], V[2][top], V[3][top]};
  const double n2 = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
  if (!(n2 > 0.0)) return false;
  for (int k = 0; k < 4; ++k) e[k] /= n2;
  const double w = e[0], x = e[1], y = e[2], z = e[3];
  R[0] = w * w + x * x - y * y - z * z;
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = w * w - x * x + y * y - z * z;
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = w * w - x * x - y * y + z * z;
  return R[0] == R[0];
}

// the unit quaternion (a >= 0) whose matrix, in the convention of orix's qu2om (om[0][1] = 2 (b c - a d)), is `om`
HV_HD void hv_om2qu(const double *om, double *q) {
  const double tr = om[0] + om[4] + om[8];
  const double s[4] = {1.0 + tr, 1.0 + om[0] - om[4] - om[8], 1.0 - om[0] + om[4] - om[8], 1.0 - om[0] - om[4] + om[8]};
  int top = 0;
  for (int k = 1; k < 4; ++k)
    if (s[k] > s[top]) top = k;
  const double ab = om[7] - om[5], ac = om[2] - om[6], ad = om[3] - om[1];  // 4 a b, 4 a c, 4 a d
  const double bc = om[1] + om[3], bd = om[2] + om[6], cd = om[5] + om[7];  // 4 b c, 4 b d, 4 c d
  const double r = 0.5 * sqrt(s[top] > 0.0 ? s[top] : 0.0), f = 0.25 / r;
  if (top == 0) {
    q[0] = r, q[1] = ab * f, q[2] = ac * f, q[3] = ad * f;
  } else if (top == 1) {
    q[0] = ab * f, q[1] = r, q[2] = bc * f, q[3] = bd * f;
  } else if (top == 2) {
    q[0] = ac * f, q[1] = bc * f, q[2] = r, q[3] = cd * f;
  } else {
    q[0] = ad * f, q[1] = bd * f, q[2] = cd * f, q[3] = r;
  }
  if (q[0] < 0.0)
    for (int k = 0; k < 4; ++k) q[k] = -q[k];
}

// votes[i][f] of the bands' triplets; ang[i][j]: folded angles of the band pairs
HV_HD void hv_vote(const double (*ang)[HV_MAX_BANDS], int nb, const HvPhase &ph, int (*votes)[HV_MAX_FAMILIES]) {
  for (int i = 0; i < nb; ++i)
    for (int f = 0; f < HV_MAX_FAMILIES; ++f) votes[i][f] = 0;
  const int P = ph.n;
  for (int i = 0; i < nb; ++i)
    for (int j = i + 1; j < nb; ++j)
      for (int k = j + 1; k < nb; ++k)
        for (int p = 0; p < P; ++p)
          for (int q = 0; q < P; ++q) {
            if (q == p || !(fabs(ph.angles[(size_t)p * P + q] - ang[i][j]) < ph.tol)) continue;
            for (int r = 0; r < P; ++r) {
              if (r == p || r == q) continue;
              if (fabs(ph.angles[(size_t)p * P + r] - ang[i][k]) < ph.tol && fabs(ph.angles[(size_t)q * P + r] - ang[j][k]) < ph.tol) {
                ++votes[i][ph.family[p]];
                ++votes[j][ph.family[q]];
                ++votes[k][ph.family[r]];
              }
            }
          }
}

HV_HD bool hv_candidate(const int *votes, int n_families, int family) {
  int top = 0;
  for (int f = 0; f < n_families; ++f) top = votes[f] > top ? votes[f] : top;
  return top > 0 && 2 * votes[family] >= top;
}

// the whole of one pattern and one phase: `bands` are unit normals in the detector frame (nb <= HV_MAX_BANDS valid bands)
HV_HD HvResult hv_index(const double (*bands)[3], int nb, int n_bands_asked, const HvPhase &ph, const HvDetector &det) {
  HvResult out;
  out.quat[0] = 1.0, out.quat[1] = out.quat[2] = out.quat[3] = 0.0;
  out.fit = 180.0;
  out.cm = 0.0;
  out.nmatch = 0;
  out.indexed = 0;
  if (nb < HV_MIN_MATCHES) return out;
  double ang[HV_MAX_BANDS][HV_MAX_BANDS], raw[HV_MAX_BANDS][HV_MAX_BANDS];
  for (int i = 0; i < nb; ++i)
    for (int j = 0; j < nb; ++j) {
      raw[i][j] = hv_dot(bands[i], bands[j]);
      ang[i][j] = hv_acos(fabs(raw[i][j]));
    }
  int votes[HV_MAX_BANDS][HV_MAX_FAMILIES];
  hv_vote(ang, nb, ph, votes);
  bool cand[HV_MAX_BANDS][HV_MAX_FAMILIES];
  for (int i = 0; i < nb; ++i)
    for (int f = 0; f < ph.n_families; ++f) cand[i][f] = hv_candidate(votes[i], ph.n_families, f);
  // hypotheses
  double bestR[9], best_score = -1.0;
  int best_count = 0, match[HV_MAX_BANDS];
  double sign[HV_MAX_BANDS];
  const int P = ph.n;
  for (int i = 0; i < nb; ++i)
    for (int j = i + 1; j < nb; ++j) {
      if (!(ang[i][j] > HV_MIN_PAIR)) continue;
      for (int p = 0; p < P; ++p) {
        if (!cand[i][ph.family[p]]) continue;
        for (int q = 0; q < P; ++q) {
          if (q == p || !cand[j][ph.family[q]]) continue;
          if (!(fabs(ph.angles[(size_t)p * P + q] - ang[i][j]) < ph.tol)) continue;
          const double *gp = ph.normals + 3 * p, *gq = ph.normals + 3 * q;
          // the sign of g_q that puts it on n_j's side of n_i (both when the pair is at a right angle within tol)
          const double dg = hv_dot(gp, gq);
          for (int sg = 0; sg < 2; ++sg) {
            const double s = sg ? -1.0 : 1.0;
            if (!(fabs(hv_acos(s * dg) - hv_acos(raw[i][j])) < ph.tol)) continue;
            const double gqs[3] = {s * gq[0], s * gq[1], s * gq[2]};
            double R[9], score;
            if (!hv_triad(gp, gqs, bands[i], bands[j], R)) continue;
            const int count = hv_match(R, bands, nb, ph, match, sign, &score);
            if (count >= HV_MIN_MATCHES && score > best_score) {
              best_count = count;
              best_score = score;
              for (int k = 0; k < 9; ++k) bestR[k] = R[k];
            }
          }
        }
      }
    }
  if (best_count < HV_MIN_MATCHES) return out;
  // fit, match again, fit again
  double a[HV_MAX_BANDS][3], b[HV_MAX_BANDS][3], score = 0.0;
  int count = best_count;
  for (int round = 0; round < 2; ++round) {
    count = hv_match(bestR, bands, nb, ph, match, sign, &score);
    if (count < HV_MIN_MATCHES) return out;
    int n = 0;
    for (int i = 0; i < nb; ++i) {
      if (match[i] < 0) continue;
      for (int k = 0; k < 3; ++k) {
        a[n][k] = sign[i] * ph.normals[3 * match[i] + k];
        b[n][k] = bands[i][k];
      }
      ++n;
    }
    if (!hv_fit(a, b, n, bestR)) return out;
  }
  count = hv_match(bestR, bands, nb, ph, match, sign, &score);
  if (count < HV_MIN_MATCHES) return out;
  double dev = 0.0;
  for (int i = 0; i < nb; ++i) {
    if (match[i] < 0) continue;
    double v[3];
    hv_apply(bestR, ph.normals + 3 * match[i], v);
    dev += hv_acos(fabs(hv_dot(v, bands[i])));
  }
  // n_d = R g = U^T g  ->  om = U s2d = R^T s2d
  double om[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      om[3 * r + c] = bestR[r] * det.s2d[c] + bestR[3 + r] * det.s2d[3 + c] + bestR[6 + r] * det.s2d[6 + c];
  hv_om2qu(om, out.quat);
  out.fit = dev / count * HV_DEGREES;
  out.nmatch = count;
  out.cm = (double)count / (double)(n_bands_asked > 0 ? n_bands_asked : 1);
  out.indexed = 1;
  return out;
}

}  // namespace kpdi
