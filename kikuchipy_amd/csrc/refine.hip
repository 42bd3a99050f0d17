// refine.hip - refinement of orientations and/or projection centres (PCs): the objective
// functions AND the optimiser on the device.
//   indexing/_refinement/_objective_functions.py:36-190   1 - NCC(exp, project(euler, pc))
//   indexing/_refinement/_solvers.py:51-74               _prepare_pattern
//   indexing/_refinement/_solvers.py:79-460              *_solver_scipy with method=minimize
//   similarity_metrics/_normalized_cross_correlation.py:200-225   NCC of a centred pattern
//   _utils/numba.py:43-57 (rotation_from_euler), _utils/_gnonomic_bounds.py:25-65,
//   signals/util/_master_pattern.py:133-204 (direction cosines for one PC)
// The optimisers are plain C++17 headers, each restating its original operation for operation in f64 without fused
// multiply-add and each pinned on the analytic objectives of analytic_objectives.h by a self-test kernel below:
//   nelder_mead.h             scipy.optimize.minimize(method="Nelder-Mead"), what the reference calls by default
//   powell.h                  scipy.optimize.minimize(method="Powell")
//   nlopt_simplex.h           the search NLopt offers as LN_NELDERMEAD, from the text of DESIGN.md section 21
//   differential_evolution.h  scipy.optimize.differential_evolution, strategy="best1bin", NumPy's legacy RandomState
//   basinhopping.h            scipy.optimize.basinhopping around the Nelder-Mead above, on the same RandomState
// Every other optimiser stays on the host and calls `refine_objective_kernel`.
//
// One workgroup per (experimental pattern, start) runs the WHOLE optimisation.  In
// `refine_solve_kernel` and `refine_solve_basinhopping_kernel` thread 0 owns the search (LDS) and decides the next
// point; in the other three solve kernels every thread runs the optimiser on the same values.  All 256
// threads evaluate the objective (each pixel: direction cosine for the current PC -> rotate
// -> Lambert -> one 16-byte master-pattern gather -> float32 value; three f64 block sums give
// the NCC).  No host round trip and no kernel launch per evaluation: a refinement of M
// patterns is one launch.  The objective is f64-VALU-bound like project.hip; the centred
// pattern (k x 4 B) and the master pattern stay in L2.
#include "kernels.h"
#include "../../include/kpdi.h"

#pragma clang fp contract(fast)
#include "projection.h"
#pragma clang fp contract(off)

#include <climits>

#include "analytic_objectives.h"
#include "basinhopping.h"
#include "differential_evolution.h"
#include "nelder_mead.h"
#include "nlopt_simplex.h"
#include "powell.h"

namespace kpdi {

constexpr int REF_THREADS = 256;
constexpr int NV_MAX = 6;

__device__ __forceinline__ double block_sum3(double &a, double &b, double &c, double *red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
    c += __shfl_xor(c, o, 64);
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();  // `red` may still be read from the previous evaluation
  if ((threadIdx.x & 63) == 0) {
    red[3 * w] = a;
    red[3 * w + 1] = b;
    red[3 * w + 2] = c;
  }
  __syncthreads();
  a = b = c = 0.0;
#pragma unroll
  for (int i = 0; i < REF_THREADS / 64; ++i) {
    a += red[3 * i];
    b += red[3 * i + 1];
    c += red[3 * i + 2];
  }
  return a;
}

// ---- _prepare_pattern: gather kept pixels, float32, optional rescale to [-1, 1] (float32
// arithmetic in the reference's order), centre, squared norm of the centred pattern
template <typename T>
__global__ __launch_bounds__(REF_THREADS) void refine_prep_kernel(const T *raw, int npix, const int *pix_map, int k,
                                                                  int rescale, float *out, double *sqnorm) {
  __shared__ double red[3 * REF_THREADS / 64];
  __shared__ float mm[2 * REF_THREADS / 64];
  const int64_t n = blockIdx.x;
  const T *p = raw + n * npix;
  float *o = out + n * k;
  const int tid = threadIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  if (rescale) {
    for (int c = tid; c < k; c += REF_THREADS) {
      const float v = (float)p[pix_map ? pix_map[c] : c];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, s, 64));
      hi = fmaxf(hi, __shfl_xor(hi, s, 64));
    }
    if ((tid & 63) == 0) {
      mm[2 * (tid >> 6)] = lo;
      mm[2 * (tid >> 6) + 1] = hi;
    }
    __syncthreads();
    for (int i = 0; i < REF_THREADS / 64; ++i) {
      lo = fminf(lo, mm[2 * i]);
      hi = fmaxf(hi, mm[2 * i + 1]);
    }
  }
  const float span = hi - lo;
  double s1 = 0.0, d0 = 0.0, d1 = 0.0;
  for (int c = tid; c < k; c += REF_THREADS) {
    float v = (float)p[pix_map ? pix_map[c] : c];
    if (rescale) v = (v - lo) / span * 2.0f + -1.0f;
    s1 += (double)v;
  }
  block_sum3(s1, d0, d1, red);
  const float mean = (float)(s1 / (double)k);
  double s2 = 0.0;
  d0 = d1 = 0.0;
  for (int c = tid; c < k; c += REF_THREADS) {
    float v = (float)p[pix_map ? pix_map[c] : c];
    if (rescale) v = (v - lo) / span * 2.0f + -1.0f;
    v -= mean;
    o[c] = v;
    s2 += (double)v * (double)v;
  }
  block_sum3(s2, d0, d1, red);
  if (tid == 0) sqnorm[n] = (double)(float)s2;  // the reference keeps it as a float32
}

// ---- geometry shared by every evaluation of a launch
struct RefineGeom {
  int nrows, ncols, k;
  const unsigned *rowcol;  // [k] (row << 16 | col) of every kept pixel
  double om[9];            // detector -> sample orientation matrix, row-major
  MasterView mp;
};

// _utils/numba.py:43-57
__device__ inline void rotation_from_euler(double phi1, double Phi, double phi2, double *q) {
  const double sigma = 0.5 * (phi1 + phi2), delta = 0.5 * (phi1 - phi2);
  double c, s, cs, ss, cd, sd;
  sincos(0.5 * Phi, &s, &c);
  sincos(sigma, &ss, &cs);
  sincos(delta, &sd, &cd);
  q[0] = c * cs;
  q[1] = -s * cd;
  q[2] = -s * sd;
  q[3] = -c * ss;
  if (q[0] < 0.0) {
    q[0] = -q[0];
    q[1] = -q[1];
    q[2] = -q[2];
    q[3] = -q[3];
  }
}

#pragma clang fp contract(fast)
// 1 - NCC between the centred experimental pattern `pat` and the pattern projected for
// quaternion `q` and PC `pc`; every thread returns the same value
__device__ inline double refine_objective(const double *q, const double *pc, const RefineGeom &g, const float *pat,
                                          double sqn, double *red) {
  const RotCoeff r = rot_coeff(q);
  // get_gnomonic_bounds + _get_direction_cosines_for_fixed_pc
  const double aspect = (double)g.ncols / (double)g.nrows;
  const double pcx = pc[0], pcy = pc[1], pcz = pc[2];
  const double x_min = -aspect * (pcx / pcz), x_max = aspect * (1.0 - pcx) / pcz;
  const double y_min = -(1.0 - pcy) / pcz, y_max = pcy / pcz;
  const double x_scale = (x_max - x_min) / (double)g.ncols, y_scale = (y_max - y_min) / (double)g.nrows;
  const double x_half = x_scale / 2.0, y_half = y_scale / 2.0;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int c = threadIdx.x; c < g.k; c += REF_THREADS) {
    const unsigned rc = g.rowcol[c];
    const double gx = x_min + (double)(rc & 0xffffu) * x_scale;
    const double gy = y_max + (double)(rc >> 16) * (-y_scale);
    const double v0 = (gx + x_half) * pcz, v1 = (gy - y_half) * pcz, v2 = pcz;
    const double w0 = v0 * g.om[0] + v1 * g.om[1] + v2 * g.om[2];
    const double w1 = v0 * g.om[3] + v1 * g.om[4] + v2 * g.om[5];
    const double w2 = v0 * g.om[6] + v1 * g.om[7] + v2 * g.om[8];
    const double rn = rsq_fast(w0 * w0 + w1 * w1 + w2 * w2);
    const double sim = (double)(float)project_pixel(r, w0 * rn, w1 * rn, w2 * rn, g.mp);  // dtype_out=float32
    s1 += sim;
    s2 += sim * sim;
    s3 += (double)pat[c] * sim;
  }
  block_sum3(s1, s2, s3, red);
  // sum(exp * (sim - mean)) = sum(exp * sim) because exp is centred; sum((sim - mean)^2) = s2 - s1^2 / k
  const double var = s2 - s1 * s1 / (double)g.k;
  return 1.0 - s3 / sqrt(sqn * var);
}
#pragma clang fp contract(off)

// control variables -> (quaternion, PC) for the three refinement modes
__device__ inline void unpack_variables(int mode, const double *x, const double *fixed, double *q, double *pc) {
  if (mode == KPDI_REFINE_ORI) {  // x = Euler angles, fixed = PC
    rotation_from_euler(x[0], x[1], x[2], q);
    pc[0] = fixed[0]; pc[1] = fixed[1]; pc[2] = fixed[2];
  } else if (mode == KPDI_REFINE_PC) {  // x = PC, fixed = quaternion
    q[0] = fixed[0]; q[1] = fixed[1]; q[2] = fixed[2]; q[3] = fixed[3];
    pc[0] = x[0]; pc[1] = x[1]; pc[2] = x[2];
  } else {  // x = Euler angles + PC
    rotation_from_euler(x[0], x[1], x[2], q);
    pc[0] = x[3]; pc[1] = x[4]; pc[2] = x[5];
  }
}

// result row of job `job`: fun, nfev, a third number (nit, or the status of the LN_NELDERMEAD search), x[0..nvar).
// Called by one thread.
constexpr int RESULT_STRIDE = REFINE_RESULT_STRIDE;
static_assert(RESULT_STRIDE == 3 + NV_MAX, "result row = fun, nfev, nit + control variables");

__device__ __forceinline__ void write_result(double *results, int64_t job, double fun, double nfev, double third,
                                             const double *x, int nvar) {
  double *o = results + job * RESULT_STRIDE;
  o[0] = fun;
  o[1] = nfev;
  o[2] = third;
  for (int i = 0; i < nvar; ++i) o[3 + i] = x[i];
}

// ---- SciPy's Nelder-Mead (nelder_mead.h) on the device: a state machine that thread 0 steps
using NelderMeadState = NelderMead<NV_MAX>;

__global__ __launch_bounds__(REF_THREADS) void refine_solve_kernel(int mode, int nvar, int nfixed, int n_starts,
                                                                    const double *x0, const double *fixed,
                                                                    const double *lower, const double *upper,
                                                                    RefineGeom g, const float *patterns,
                                                                    const double *sqnorm, double xatol, double fatol,
                                                                    int maxiter, int maxfun, double *results) {
  __shared__ NelderMeadState nm;
  __shared__ double red[3 * REF_THREADS / 64];
  const int64_t job = blockIdx.x;  // (pattern, start)
  const int64_t pat_id = job / n_starts;
  const float *pat = patterns + pat_id * g.k;
  const double sqn = sqnorm[pat_id];
  const double *fx = fixed + job * nfixed;
  if (threadIdx.x == 0)
    nm.begin(nvar, x0 + job * nvar, lower ? lower + job * nvar : nullptr, upper ? upper + job * nvar : nullptr, xatol,
             fatol, maxiter, maxfun);
  __syncthreads();
  while (nm.state != NelderMeadState::S_DONE) {
    double q[4], pc[3];
    unpack_variables(mode, nm.xeval, fx, q, pc);
    const double f = refine_objective(q, pc, g, pat, sqn, red);
    __syncthreads();  // every thread has read nm.xeval / nm.state
    if (threadIdx.x == 0) nm.feed(f);
    __syncthreads();
  }
  if (threadIdx.x == 0) write_result(results, job, nm.fun(), (double)nm.fcalls, (double)nm.iterations, nm.sim[0], nvar);
}

// batched objective: one workgroup per evaluation
__global__ __launch_bounds__(REF_THREADS) void refine_objective_kernel(int mode, int nvar, int nfixed, const int *pattern_index,
                                                                        const double *x, const double *fixed, RefineGeom g,
                                                                        const float *patterns, const double *sqnorm,
                                                                        double *out) {
  __shared__ double red[3 * REF_THREADS / 64];
  const int64_t e = blockIdx.x;
  const int64_t pat_id = pattern_index[e];
  double q[4], pc[3];
  unpack_variables(mode, x + e * nvar, fixed + e * nfixed, q, pc);
  const double f = refine_objective(q, pc, g, patterns + pat_id * g.k, sqnorm[pat_id], red);
  if (threadIdx.x == 0) out[e] = f;
}

// ---- the self-tests: one optimiser alone, in one thread, on an analytic f64 objective (analytic_objectives.h); the
// host and GPU tests compare the row with SciPy's (with the restatement's for LN_NELDERMEAD) bit for bit.
// nelder_mead.h, kinds 0..4.  result: fun, nfev, nit, x[0..nvar)
__global__ void nelder_mead_selftest_kernel(int kind, int nvar, const double *x0, const double *lower, const double *upper,
                                            double xatol, double fatol, int maxiter, int maxfun, double *result) {
  __shared__ NelderMeadState nm;
  if (threadIdx.x != 0) return;
  const AnalyticObjective ev{kind, nvar};
  nm.begin(nvar, x0, lower, upper, xatol, fatol, maxiter, maxfun);
  while (nm.state != NelderMeadState::S_DONE) nm.feed(ev.eval(nm.xeval));
  write_result(result, 0, nm.fun(), (double)nm.fcalls, (double)nm.iterations, nm.sim[0], nvar);
}

// ---- the other three solvers on the device.  `refine_objective` returns the same bits in every thread and has
// barriers inside, so the optimiser is not handed to one thread: EVERY thread runs it, as straight-line code on those
// uniform values, with its state in private memory.  Control flow is then uniform by construction - all 256 threads
// ask for the same evaluations in the same order and meet at the same barriers - and nothing is shared but `red`.
// RefineEval is the `E` of the three headers: the objective of one job.
struct RefineEval {
  int mode, nvar;
  const double *fx;
  const RefineGeom *g;
  const float *pat;
  double sqn;
  double *red;
  double *trace;  // rows (x[0..nvar), f) of this job's evaluations, or nullptr
  int trace_capacity;
  long long n_eval;
  // the job of this workgroup; its evaluations are traced when it is `trace_job` (and `trace` is given)
  __device__ __forceinline__ static RefineEval of_job(int mode, int nvar, int nfixed, int n_starts, const double *fixed,
                                                      const RefineGeom &g, const float *patterns, const double *sqnorm,
                                                      double *red, long long trace_job, double *trace,
                                                      int trace_capacity) {
    const int64_t job = blockIdx.x;  // (pattern, start)
    const int64_t pat_id = job / n_starts;
    RefineEval ev;
    ev.mode = mode;
    ev.nvar = nvar;
    ev.fx = fixed + job * nfixed;
    ev.g = &g;
    ev.pat = patterns + pat_id * g.k;
    ev.sqn = sqnorm[pat_id];
    ev.red = red;
    ev.trace = job == trace_job ? trace : nullptr;
    ev.trace_capacity = trace_capacity;
    ev.n_eval = 0;
    return ev;
  }
  __device__ double eval(const double *x) {
    double q[4], pc[3];
    unpack_variables(mode, x, fx, q, pc);
    const double f = refine_objective(q, pc, *g, pat, sqn, red);
    if (trace != nullptr && threadIdx.x == 0 && n_eval < (long long)trace_capacity) {
      double *row = trace + n_eval * (nvar + 1);
      for (int i = 0; i < nvar; ++i) row[i] = x[i];
      row[nvar] = f;
    }
    ++n_eval;
    return f;
  }
};

// ---- SciPy's Powell (powell.h)
__global__ __launch_bounds__(REF_THREADS, 4) void refine_solve_powell_kernel(
    int mode, int nvar, int nfixed, int n_starts, const double *x0, const double *fixed, const double *lower,
    const double *upper, RefineGeom g, const float *patterns, const double *sqnorm, double xtol, double ftol, int maxiter,
    int maxfev, double *results, long long trace_job, double *trace, int trace_capacity) {
  __shared__ double red[3 * REF_THREADS / 64];
  const int64_t job = blockIdx.x;  // (pattern, start)
  RefineEval ev = RefineEval::of_job(mode, nvar, nfixed, n_starts, fixed, g, patterns, sqnorm, red, trace_job, trace,
                                     trace_capacity);
  Powell<NV_MAX, RefineEval> pw(ev);
  pw.minimize(nvar, x0 + job * nvar, lower ? lower + job * nvar : nullptr, upper ? upper + job * nvar : nullptr, xtol,
              ftol, maxiter, maxfev);
  if (threadIdx.x == 0) write_result(results, job, pw.fval, (double)pw.fcalls, (double)pw.iter, pw.x, nvar);
}

// self-test row of powell.h and differential_evolution.h: fun, nfev, nit, a flag (status / success), x[0..nvar)
__device__ __forceinline__ void write_selftest_result(double *result, double fun, double nfev, double nit, double flag,
                                                      const double *x, int nvar) {
  result[0] = fun;
  result[1] = nfev;
  result[2] = nit;
  result[3] = flag;
  for (int i = 0; i < nvar; ++i) result[4 + i] = x[i];
}

// powell.h alone, kinds 0..4
__global__ void powell_selftest_kernel(int kind, int nvar, const double *x0, const double *lower, const double *upper,
                                       double xtol, double ftol, int maxiter, int maxfev, double *result) {
  if (threadIdx.x != 0) return;
  AnalyticObjective ev{kind, nvar};
  Powell<NV_MAX, AnalyticObjective> pw(ev);
  pw.minimize(nvar, x0, lower, upper, xtol, ftol, maxiter, maxfev);
  write_selftest_result(result, pw.fval, (double)pw.fcalls, (double)pw.iter, (double)pw.status, pw.x, nvar);
}

// ---- the LN_NELDERMEAD search (nlopt_simplex.h) on the device, run like Powell: every thread walks the same simplex on
// the uniform objective values.  Each (pattern, start) is one `optimize` call with its own evaluation count.
// result row: minf, nevals, status, x (the best point seen)
__global__ __launch_bounds__(REF_THREADS, 4) void refine_solve_nlopt_kernel(
    int mode, int nvar, int nfixed, int n_starts, const double *x0, const double *fixed, const double *lower,
    const double *upper, RefineGeom g, const float *patterns, const double *sqnorm, NloptStep xstep, double ftol_rel,
    int maxeval, double *results) {
  __shared__ double red[3 * REF_THREADS / 64];
  const int64_t job = blockIdx.x;  // (pattern, start)
  RefineEval ev = RefineEval::of_job(mode, nvar, nfixed, n_starts, fixed, g, patterns, sqnorm, red, -1, nullptr, 0);
  NloptSimplex<NV_MAX, RefineEval> ns(ev);
  ns.optimize(nvar, x0 + job * nvar, lower ? lower + job * nvar : nullptr, upper ? upper + job * nvar : nullptr,
              xstep.given ? xstep.v : nullptr, ftol_rel, maxeval);
  if (threadIdx.x == 0) write_result(results, job, ns.minf, (double)ns.nevals, (double)ns.status, ns.x, nvar);
}

// nlopt_simplex.h alone, kinds 0..4 and 5 = ANALYTIC_ARMS.  result: minf, nevals, status, x[0..nvar)
__global__ void nlopt_simplex_selftest_kernel(int kind, int nvar, const double *x0, const double *lower, const double *upper,
                                              const double *xstep, double ftol_rel, int maxeval, double *result) {
  if (threadIdx.x != 0) return;
  AnalyticObjective ev{kind, nvar};
  NloptSimplex<NV_MAX, AnalyticObjective> ns(ev);
  ns.optimize(nvar, x0, lower, upper, xstep, ftol_rel, maxeval);
  write_result(result, 0, ns.minf, (double)ns.nevals, (double)ns.status, ns.x, nvar);
}

// ---- SciPy's differential evolution (differential_evolution.h) on the device, run like Powell: every thread runs the
// solver on the uniform objective values, so all 256 meet at the barriers inside `refine_objective`.  What Powell keeps
// in private memory is too large here - the population, the trial population, the energies, the index array and the
// 624 words of the random stream - and lives in LDS: thread 0 alone draws and writes, `DeTeam::sync` separates its
// writes from the reads of the others.
// LDS: DeStorage<6, 256> = 2500 (stream) + 2 x 12288 (population, trial) + 2 x 2048 (energies) + 2 x 1024 (index, fill)
// + 48 = 33 272 B, + `red` = 32.6 KiB: four workgroups per CU (what __launch_bounds__(REF_THREADS, 4) leaves registers
// for) take 130 of the CU's 160 KiB.  The population of the defaults is 45 (three variables) or 90 (six); larger ones than
// DE_POP_MAX stay on the host.
// The evaluations of one job stay serial: with updating="immediate" every trial is built from the population the trial
// before it may have changed, and the number of draws of _ensure_constraint depends on the values.
constexpr int DE_POP_MAX = KPDI_DE_POP_MAX;
using DeState = DeStorage<NV_MAX, DE_POP_MAX>;
static_assert(sizeof(DeState) + 3 * REF_THREADS / 64 * sizeof(double) <= 40 * 1024, "four workgroups per CU: 160 KiB of LDS");

struct DeTeam {
  __device__ bool leader() const { return threadIdx.x == 0; }
  __device__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(REF_THREADS, 4) void refine_solve_de_kernel(
    int mode, int nvar, int nfixed, int n_starts, const double *fixed, const double *lower, const double *upper,
    RefineGeom g, const float *patterns, const double *sqnorm, DeOptions de, double *results, long long trace_job,
    double *trace, int trace_capacity) {
  __shared__ DeState st;
  __shared__ double red[3 * REF_THREADS / 64];
  const int64_t job = blockIdx.x;  // (pattern, start)
  RefineEval ev = RefineEval::of_job(mode, nvar, nfixed, n_starts, fixed, g, patterns, sqnorm, red, trace_job, trace,
                                     trace_capacity);
  DifferentialEvolution<NV_MAX, DE_POP_MAX, RefineEval, DeTeam> solver(ev, st);
  solver.solve(nvar, lower + job * nvar, upper + job * nvar, de.members, de.maxiter, de.tol, de.atol, de.mutation_lo,
               de.mutation_hi, de.recombination, de.init, de.updating, de.seeds[job]);
  if (threadIdx.x == 0) write_result(results, job, solver.fun, (double)solver.nfev, (double)solver.nit, solver.x, nvar);
}

// differential_evolution.h alone, kinds 0..4 and its own 5..7 (`analytic_kind_de`): 5 = ANALYTIC_HUG, on which trial
// vectors leave [0, 1] and are drawn again, 6 = +inf everywhere, 7 = 0.1 everywhere
__global__ void de_selftest_kernel(int kind, int nvar, const double *lower, const double *upper, DeOptions de,
                                   unsigned seed, double *result) {
  __shared__ DeState st;
  if (threadIdx.x != 0) return;
  AnalyticObjective ev{analytic_kind_de(kind), nvar};
  DifferentialEvolution<NV_MAX, DE_POP_MAX, AnalyticObjective> solver(ev, st);
  solver.solve(nvar, lower, upper, de.members, de.maxiter, de.tol, de.atol, de.mutation_lo, de.mutation_hi,
               de.recombination, de.init, de.updating, seed);
  write_selftest_result(result, solver.fun, (double)solver.nfev, (double)solver.nit, solver.success ? 1.0 : 0.0, solver.x,
                        nvar);
}

// ---- SciPy's basinhopping around Nelder-Mead (basinhopping.h) on the device, run like `refine_solve_kernel`: thread 0
// owns the search - the hops, the quench that runs, the lowest result - and the random stream, both in LDS (the 624
// words of the stream where the differential evolution keeps them), and decides the next point; all 256 threads
// evaluate it through `RefineEval`.  Unbounded: the reference's basinhopping takes no trust region.
// LDS: BasinHopping<6> (the simplex of the quench and three points, ~1 KiB) + 2500 B (stream) + `red`.
// result row: fun, nfev, nit, x of the lowest result
using BhState = BasinHopping<NV_MAX>;

__global__ __launch_bounds__(REF_THREADS, 4) void refine_solve_basinhopping_kernel(
    int mode, int nvar, int nfixed, int n_starts, const double *x0, const double *fixed, RefineGeom g,
    const float *patterns, const double *sqnorm, BhOptions opt, double xatol, double fatol, int maxiter, int maxfun,
    double *results, long long trace_job, double *trace, int trace_capacity) {
  __shared__ BhState bh;
  __shared__ Mt19937 mt;
  __shared__ double red[3 * REF_THREADS / 64];
  const int64_t job = blockIdx.x;  // (pattern, start)
  RefineEval ev = RefineEval::of_job(mode, nvar, nfixed, n_starts, fixed, g, patterns, sqnorm, red, trace_job, trace,
                                     trace_capacity);
  if (threadIdx.x == 0) {
    mt_seed(mt, opt.seeds[job]);
    bh.begin(mt, nvar, x0 + job * nvar, opt.niter, opt.T, opt.stepsize, opt.interval, (long long)opt.niter_success,
             opt.target_accept_rate, opt.stepwise_factor, xatol, fatol, maxiter, maxfun);
  }
  __syncthreads();
  while (bh.state != BhState::S_DONE) {
    const double f = ev.eval(bh.xeval());
    __syncthreads();  // every thread has read the point and the state
    if (threadIdx.x == 0) bh.feed(mt, f);
    __syncthreads();
  }
  if (threadIdx.x == 0) write_result(results, job, bh.fun, (double)bh.nfev, (double)bh.nit, bh.xbest, nvar);
}

// basinhopping.h alone, kinds 0..4.  result: fun, nfev, nit, success, minimization_failures, x[0..nvar)
__global__ void basinhopping_selftest_kernel(int kind, int nvar, const double *x0, BhOptions opt, double xatol,
                                             double fatol, int maxiter, int maxfun, unsigned seed, double *result) {
  __shared__ BhState bh;
  __shared__ Mt19937 mt;
  if (threadIdx.x != 0) return;
  const AnalyticObjective ev{kind, nvar};
  mt_seed(mt, seed);
  bh.begin(mt, nvar, x0, opt.niter, opt.T, opt.stepsize, opt.interval, (long long)opt.niter_success,
           opt.target_accept_rate, opt.stepwise_factor, xatol, fatol, maxiter, maxfun);
  while (bh.state != BhState::S_DONE) bh.feed(mt, ev.eval(bh.xeval()));
  result[0] = bh.fun;
  result[1] = (double)bh.nfev;
  result[2] = (double)bh.nit;
  result[3] = bh.success ? 1.0 : 0.0;
  result[4] = (double)bh.minimization_failures;
  for (int i = 0; i < nvar; ++i) result[5 + i] = bh.xbest[i];
}

// the random stream alone: `mt_program` from RandomState(seed); out[0..capacity) the words, out[capacity] their count
__global__ void mt19937_selftest_kernel(unsigned seed, const double *program, int n, unsigned long long *out,
                                        long long capacity) {
  __shared__ Mt19937 mt;
  __shared__ int index[DE_POP_MAX], scratch[DE_POP_MAX];
  if (threadIdx.x != 0) return;
  mt_seed(mt, seed);
  out[capacity] = (unsigned long long)mt_program(mt, program, n, index, scratch, DE_POP_MAX, (uint64_t *)out, capacity);
}

// ---- launchers
static RefineGeom make_geom(const RefineLaunch &a) {
  RefineGeom g;
  g.nrows = a.nrows;
  g.ncols = a.ncols;
  g.k = a.k;
  g.rowcol = a.rowcol;
  for (int i = 0; i < 9; ++i) g.om[i] = a.om[i];
  g.mp.packed = (const float2 *)a.master_packed;
  g.mp.npx = a.npx;
  g.mp.npy = a.npy;
  g.mp.scale = (double)(a.npx - 1) / 2.0;
  g.mp.lam2px = g.mp.scale / 1.2533141373155002512;
  return g;
}

hipError_t launch_refine_prep(const void *raw, int dtype, int64_t n, int npix, const int *pix_map, int k, int rescale,
                              float *out, double *sqnorm, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  dim3 grid((unsigned)n), block(REF_THREADS);
#define KPDI_RPREP(T)                                                                                            \
  hipLaunchKernelGGL((refine_prep_kernel<T>), grid, block, 0, s, (const T *)raw, npix, pix_map, k, rescale, out, \
                     sqnorm);                                                                                    \
  break;
  switch (dtype) {
    case KPDI_U8: KPDI_RPREP(uint8_t)
    case KPDI_I8: KPDI_RPREP(int8_t)
    case KPDI_U16: KPDI_RPREP(uint16_t)
    case KPDI_I16: KPDI_RPREP(int16_t)
    case KPDI_I32: KPDI_RPREP(int32_t)
    case KPDI_U32: KPDI_RPREP(uint32_t)
    case KPDI_F32: KPDI_RPREP(float)
    case KPDI_F64: KPDI_RPREP(double)
    case KPDI_F16: KPDI_RPREP(_Float16)
    default: return hipErrorInvalidValue;
  }
#undef KPDI_RPREP
  return hipGetLastError();
}

hipError_t launch_refine_solve(const RefineLaunch &a, hipStream_t s) {
  if (a.n_jobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(refine_solve_kernel, dim3((unsigned)a.n_jobs), dim3(REF_THREADS), 0, s, a.mode, a.nvar, a.nfixed,
                     a.n_starts, a.x0, a.fixed, a.lower, a.upper, make_geom(a), a.patterns, a.sqnorm, a.xatol, a.fatol,
                     a.maxiter, a.maxfun, a.results);
  return hipGetLastError();
}

hipError_t launch_refine_objective(const RefineLaunch &a, const int *pattern_index, double *out, hipStream_t s) {
  if (a.n_jobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(refine_objective_kernel, dim3((unsigned)a.n_jobs), dim3(REF_THREADS), 0, s, a.mode, a.nvar,
                     a.nfixed, pattern_index, a.x0, a.fixed, make_geom(a), a.patterns, a.sqnorm, out);
  return hipGetLastError();
}

// a.xatol / a.fatol: Powell's xtol / ftol; a.maxiter / a.maxfun as given (<= 0 = unset: powell.h resolves them)
hipError_t launch_refine_solve_powell(const RefineLaunch &a, int64_t trace_job, double *trace, int trace_capacity,
                                      hipStream_t s) {
  if (a.n_jobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(refine_solve_powell_kernel, dim3((unsigned)a.n_jobs), dim3(REF_THREADS), 0, s, a.mode, a.nvar,
                     a.nfixed, a.n_starts, a.x0, a.fixed, a.lower, a.upper, make_geom(a), a.patterns, a.sqnorm, a.xatol,
                     a.fatol, a.maxiter, a.maxfun, a.results, (long long)trace_job, trace, trace_capacity);
  return hipGetLastError();
}

hipError_t launch_powell_selftest(int kind, int nvar, const double *x0, const double *lower, const double *upper,
                                  double xtol, double ftol, int maxiter, int maxfev, double *result, hipStream_t s) {
  hipLaunchKernelGGL(powell_selftest_kernel, dim3(1), dim3(64), 0, s, kind, nvar, x0, lower, upper, xtol, ftol, maxiter,
                     maxfev, result);
  return hipGetLastError();
}

// a.fatol = ftol_rel, a.maxfun = maxeval (<= 0 = none), a.xstep
hipError_t launch_refine_solve_nlopt(const RefineLaunch &a, hipStream_t s) {
  if (a.n_jobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(refine_solve_nlopt_kernel, dim3((unsigned)a.n_jobs), dim3(REF_THREADS), 0, s, a.mode, a.nvar,
                     a.nfixed, a.n_starts, a.x0, a.fixed, a.lower, a.upper, make_geom(a), a.patterns, a.sqnorm, a.xstep,
                     a.fatol, a.maxfun, a.results);
  return hipGetLastError();
}

hipError_t launch_nlopt_simplex_selftest(int kind, int nvar, const double *x0, const double *lower, const double *upper,
                                         const double *xstep, double ftol_rel, int maxeval, double *result,
                                         hipStream_t s) {
  hipLaunchKernelGGL(nlopt_simplex_selftest_kernel, dim3(1), dim3(64), 0, s, kind, nvar, x0, lower, upper, xstep, ftol_rel,
                     maxeval, result);
  return hipGetLastError();
}

// a.de: the options and the device array of one seed per job; bounds are required
hipError_t launch_refine_solve_de(const RefineLaunch &a, int64_t trace_job, double *trace, int trace_capacity,
                                  hipStream_t s) {
  if (a.n_jobs <= 0) return hipSuccess;
  if (a.de.members < 5 || a.de.members > DE_POP_MAX || !a.lower || !a.upper || !a.de.seeds) return hipErrorInvalidValue;
  hipLaunchKernelGGL(refine_solve_de_kernel, dim3((unsigned)a.n_jobs), dim3(REF_THREADS), 0, s, a.mode, a.nvar, a.nfixed,
                     a.n_starts, a.fixed, a.lower, a.upper, make_geom(a), a.patterns, a.sqnorm, a.de, a.results,
                     (long long)trace_job, trace, trace_capacity);
  return hipGetLastError();
}

hipError_t launch_de_selftest(int kind, int nvar, const double *lower, const double *upper, const DeOptions &de,
                              unsigned seed, double *result, hipStream_t s) {
  if (de.members < 5 || de.members > DE_POP_MAX || nvar < 1 || nvar > NV_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(de_selftest_kernel, dim3(1), dim3(64), 0, s, kind, nvar, lower, upper, de, seed, result);
  return hipGetLastError();
}

// a.bh: the options and the device array of one seed per job; the quench's budget is resolved (both >= 1)
hipError_t launch_refine_solve_basinhopping(const RefineLaunch &a, int64_t trace_job, double *trace, int trace_capacity,
                                            hipStream_t s) {
  if (a.n_jobs <= 0) return hipSuccess;
  if (a.bh.niter < 0 || a.bh.interval < 1 || a.maxiter < 1 || a.maxfun < 1 || !a.x0 || !a.bh.seeds)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(refine_solve_basinhopping_kernel, dim3((unsigned)a.n_jobs), dim3(REF_THREADS), 0, s, a.mode, a.nvar,
                     a.nfixed, a.n_starts, a.x0, a.fixed, make_geom(a), a.patterns, a.sqnorm, a.bh, a.xatol, a.fatol,
                     a.maxiter, a.maxfun, a.results, (long long)trace_job, trace, trace_capacity);
  return hipGetLastError();
}

hipError_t launch_basinhopping_selftest(int kind, int nvar, const double *x0, const BhOptions &bh, double xatol,
                                        double fatol, int maxiter, int maxfun, unsigned seed, double *result,
                                        hipStream_t s) {
  if (bh.niter < 0 || bh.interval < 1 || maxiter < 1 || maxfun < 1 || nvar < 1 || nvar > NV_MAX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(basinhopping_selftest_kernel, dim3(1), dim3(64), 0, s, kind, nvar, x0, bh, xatol, fatol, maxiter,
                     maxfun, seed, result);
  return hipGetLastError();
}

hipError_t launch_mt19937_selftest(unsigned seed, const double *program, int n, uint64_t *out, long long capacity,
                                   hipStream_t s) {
  hipLaunchKernelGGL(mt19937_selftest_kernel, dim3(1), dim3(64), 0, s, seed, program, n, (unsigned long long *)out,
                     capacity);
  return hipGetLastError();
}

hipError_t launch_nelder_mead_selftest(int kind, int nvar, const double *x0, const double *lower, const double *upper,
                                       double xatol, double fatol, int maxiter, int maxfun, double *result,
                                       hipStream_t s) {
  hipLaunchKernelGGL(nelder_mead_selftest_kernel, dim3(1), dim3(64), 0, s, kind, nvar, x0, lower, upper, xatol, fatol,
                     maxiter, maxfun, result);
  return hipGetLastError();
}

}  // namespace kpdi
