// differential_evolution.h - scipy.optimize.differential_evolution of SciPy 1.15.3 with strategy="best1bin", restated
// operation for operation in f64 for the host and the device (plain C++17, no HIP headers), over NumPy's legacy
// RandomState restated in integers.
//   scipy/optimize/_differentialevolution.py
//     :845-930    limits, __scale_arg1 / __scale_arg2, num_population_members  -> DifferentialEvolution::solve
//     :989-1025   init_population_lhs                                          -> init_lhs
//     :1063-1076  init_population_random                                       -> init_random
//     :1131-1140  converged                                                    -> converged
//     :1142-1222  solve (the for ... else over the generations)                -> solve
//     :1310-1363  _calculate_population_energies                               -> evaluate
//     :1365-1383  _promote_lowest_energy                                       -> promote
//     :1498-1541  _accept_trial (no constraints: energy_trial <= energy_orig)  -> accepts
//     :1543-1666  __next__, both updating modes                                -> next
//     :1668-1686  _scale_parameters, _ensure_constraint                        -> scale_parameters, ensure_constraint
//     :1711-1738  _mutate_many                                                 -> mutate_many
//     :1752-1778  _mutate                                                      -> mutate
//     :1790-1797  _best1                                                       -> best1
//     :1840-1847  _select_samples                                              -> select_samples
//   numpy/random (the legacy stream behind `seed=<int>`): mt19937 seeding, generation and tempering, the 53-bit
//   double, `uniform`, the masked rejection of `randint` / `random_interval`, `shuffle` of a 1-D array and
//   `permutation` as a shuffle of arange; numpy's pairwise summation behind np.mean / np.std.
// Every sum, product and comparison is written in SciPy's / NumPy's order and form (a comparison with a NaN takes
// their branch) and the file must be compiled WITHOUT fused multiply-add: with the same seed and the same objective
// values the search then draws the same numbers, evaluates the same points in the same order and returns the same
// bits (tests/test_host_de.py, tests/test_gpu_de.py).
//
// Not restated: `maxfun` is infinite in `differential_evolution`, so the StopIteration branches of __next__ and the
// padding of _calculate_population_energies never run; constraints, integrality, x0, callbacks, workers, every
// strategy but best1bin, the sobol / halton / array initialisations and the polish (`solve` after the loop) stay
// with SciPy on the host.
//
// The state that is large - population, energies, trial population, index array, the 624 words of the stream -
// lives in a `DeStorage` the caller places (LDS on the device).  `Team` says who writes it: on the device every
// thread of a workgroup runs `solve` on the same values, the leader alone writes the storage, and `sync` (a
// barrier) separates its writes from the reads of the others.  The default `DeSolo` is one thread on its own.
//
// KPDI_DE_COUNT (host tests only): every if / else arm and every loop exit below increments one entry of
// `kpdi_de_count`.  KPDI_DE_WRONG = 1..4 (host tests only) builds a deliberately wrong variant, see the tests.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KPDI_HD __host__ __device__
#else
#define KPDI_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// clang-format off
#define KPDI_DE_BRANCHES(X)                                                                                          \
  X(mt_twist) X(mt_ready) X(interval_zero) X(interval_reject) X(interval_accept)                                      \
  X(init_lhs) X(init_random) X(recalc_all_inf) X(recalc_not) X(dither_draw) X(dither_none)                           \
  X(gen_immediate) X(gen_deferred) X(sample_candidate_skipped) X(sample_taken)                                       \
  X(cross_fill) X(cross_drawn) X(cross_kept) X(oob_redraw) X(oob_inside)                                             \
  X(trial_accepted) X(trial_rejected) X(imm_promote) X(imm_no_promote)                                               \
  X(argmin_nan) X(argmin_lower) X(argmin_not_lower) X(promote_swap) X(promote_stay)                                  \
  X(conv_infinite) X(conv_yes) X(conv_no) X(psum_small) X(psum_block) X(psum_tail) X(psum_split)                     \
  X(exit_converged) X(exit_maxiter)
// clang-format on

namespace kpdi {

enum DeBranch {
#define KPDI_DE_ENUM(name) DEB_##name,
  KPDI_DE_BRANCHES(KPDI_DE_ENUM)
#undef KPDI_DE_ENUM
      DEB_COUNT
};

#ifdef KPDI_DE_COUNT
inline long long kpdi_de_count[DEB_COUNT] = {};
inline const char *const kpdi_de_branch_names[DEB_COUNT] = {
#define KPDI_DE_NAME(name) #name,
    KPDI_DE_BRANCHES(KPDI_DE_NAME)
#undef KPDI_DE_NAME
};
#define KPDI_DE_HIT(name) (++::kpdi::kpdi_de_count[::kpdi::DEB_##name])
#else
#define KPDI_DE_HIT(name) ((void)0)
#endif

#ifndef KPDI_DE_WRONG
#define KPDI_DE_WRONG 0
#endif

// ---- numpy.random.RandomState over MT19937, in integers
struct Mt19937 {
  uint32_t key[624];
  int pos;
};

// RandomState(seed) with 0 <= seed < 2^32: mt19937_seed
KPDI_HD inline void mt_seed(Mt19937 &s, uint32_t seed) {
  for (int pos = 0; pos < 624; ++pos) {
    s.key[pos] = seed;
    seed = 1812433253u * (seed ^ (seed >> 30)) + (uint32_t)pos + 1u;
  }
  s.pos = 624;
}

KPDI_HD inline uint32_t mt_twist_word(uint32_t hi, uint32_t lo, uint32_t far) {
  const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
}

KPDI_HD inline uint32_t mt_next32(Mt19937 &s) {
  if (s.pos == 624) {
    KPDI_DE_HIT(mt_twist);
    int i = 0;
    for (; i < 624 - 397; ++i) s.key[i] = mt_twist_word(s.key[i], s.key[i + 1], s.key[i + 397]);
    for (; i < 623; ++i) s.key[i] = mt_twist_word(s.key[i], s.key[i + 1], s.key[i + (397 - 624)]);
    s.key[623] = mt_twist_word(s.key[623], s.key[0], s.key[396]);
    s.pos = 0;
  } else {
    KPDI_DE_HIT(mt_ready);
  }
  uint32_t y = s.key[s.pos++];
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// random_sample: 53 bits from two words
KPDI_HD inline double mt_double(Mt19937 &s) {
  const uint32_t a = mt_next32(s) >> 5, b = mt_next32(s) >> 6;
  return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}

// uniform(low, high) = low + (high - low) * random_sample
KPDI_HD inline double mt_uniform(Mt19937 &s, double low, double high) {
  const double range = high - low;
  return low + range * mt_double(s);
}

// a number in [0, max] by masked rejection on 32-bit words (max < 2^32): what randint(0, max + 1) and the
// random_interval(max) of shuffle do; max = 0 draws nothing
KPDI_HD inline uint32_t mt_interval(Mt19937 &s, uint32_t max) {
  if (max == 0) {
    KPDI_DE_HIT(interval_zero);
    return 0;
  }
  uint32_t mask = max;
  mask |= mask >> 1;
  mask |= mask >> 2;
  mask |= mask >> 4;
  mask |= mask >> 8;
  mask |= mask >> 16;
  for (;;) {
    const uint32_t value = mt_next32(s) & mask;
    if (value > max) {
      KPDI_DE_HIT(interval_reject);
      continue;
    }
    KPDI_DE_HIT(interval_accept);
    return value;
  }
}

// shuffle of a 1-D integer array
KPDI_HD inline void mt_shuffle(Mt19937 &s, int *a, int n) {
  for (int i = n - 1; i >= 1; --i) {
    const int j = (int)mt_interval(s, (uint32_t)i);
    const int t = a[i];
    a[i] = a[j];
    a[j] = t;
  }
}

// permutation(range(n)) = shuffle of arange(n)
KPDI_HD inline void mt_permutation(Mt19937 &s, int *a, int n) {
  for (int i = 0; i < n; ++i) a[i] = i;
  mt_shuffle(s, a, n);
}

KPDI_HD inline uint64_t de_bits(double v) {
  union {
    double d;
    uint64_t u;
  } c;
  c.d = v;
  return c.u;
}

// A short program of draws for the self-tests: `n` rows (op, a, b) - 0: uniform(), 1: uniform(a, b), 2: randint(0, a),
// 3: shuffle of the persistent index array of `a` entries (arange when its length changes), 4: permutation(range(a)) -
// and the raw 64 bits of what they return (one word, or `a` words for 3 and 4).  Returns the words written; nothing
// is written beyond `capacity` and no array longer than `scratch_len` is shuffled.
KPDI_HD inline long long mt_program(Mt19937 &s, const double *program, int n, int *index, int *scratch, int scratch_len,
                                    uint64_t *out, long long capacity) {
  long long w = 0;
  int index_len = 0;
  for (int r = 0; r < n; ++r) {
    const int op = (int)program[3 * r];
    const double a = program[3 * r + 1], b = program[3 * r + 2];
    if (op == 0 || op == 1) {
      const double v = op == 0 ? mt_double(s) : mt_uniform(s, a, b);
      if (w < capacity) out[w] = de_bits(v);
      ++w;
    } else if (op == 2) {
      const uint32_t v = mt_interval(s, (uint32_t)((int)a - 1));
      if (w < capacity) out[w] = v;
      ++w;
    } else {
      int len = (int)a;
      if (len < 0) len = 0;
      if (len > scratch_len) len = scratch_len;
      int *arr = op == 3 ? index : scratch;
      if (op == 3) {
        if (index_len != len)
          for (int i = 0; i < len; ++i) index[i] = i;
        index_len = len;
        mt_shuffle(s, index, len);
      } else {
        mt_permutation(s, scratch, len);
      }
      for (int i = 0; i < len; ++i, ++w)
        if (w < capacity) out[w] = (uint64_t)arr[i];
    }
  }
  return w;
}

// ---- NumPy's elementwise forms
KPDI_HD inline bool de_isnan(double v) { return v != v; }
KPDI_HD inline bool de_isinf(double v) { return v == HUGE_VAL || v == -HUGE_VAL; }

// numpy's pairwise sum of get(off) .. get(off + n - 1): below 8 elements a plain loop, up to 128 eight running sums
// combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) with the remainder added in order, above that two halves, the first
// a multiple of 8.  DEPTH bounds the halving: 128 << DEPTH elements.
template <int DEPTH, class G>
KPDI_HD inline double de_pairwise(const G &get, int off, int n) {
  if (n < 8) {
    KPDI_DE_HIT(psum_small);
    double res = -0.0;
    for (int i = 0; i < n; ++i) res += get(off + i);
    return res;
  }
  if (n <= 128 || DEPTH == 0) {
    KPDI_DE_HIT(psum_block);
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = get(off + j);
    int i = 8;
#if KPDI_DE_WRONG == 2
    double res = 0.0;  // wrong on purpose: a plain sum
    for (int j = 0; j < 8; ++j) res += r[j];
#else
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += get(off + i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#endif
    for (; i < n; ++i) {
      KPDI_DE_HIT(psum_tail);
      res += get(off + i);
    }
    return res;
  }
  KPDI_DE_HIT(psum_split);
  int n2 = n / 2;
  n2 -= n2 % 8;
  return de_pairwise<(DEPTH > 0 ? DEPTH - 1 : 0)>(get, off, n2) + de_pairwise<(DEPTH > 0 ? DEPTH - 1 : 0)>(get, off + n2, n - n2);
}

struct DeSolo {
  KPDI_HD bool leader() const { return true; }
  KPDI_HD void sync() const {}
};

template <int NV, int SMAX>
struct DeStorage {
  Mt19937 mt;
  double population[SMAX][NV];
  double trial[SMAX][NV];  // immediate: row 0 is the trial; deferred: the trial population; init: the samples
  double energies[SMAX];
  double trial_energies[SMAX];
  int index[SMAX];  // _random_population_index: persists across _select_samples
  int fill[SMAX];   // deferred: the fill points; init: the permutation
  double xeval[NV];
};

constexpr int DE_INIT_LHS = 0, DE_INIT_RANDOM = 1;
constexpr int DE_IMMEDIATE = 0, DE_DEFERRED = 1;

// E: `double eval(const double *x)`, the objective at n variables, the same value in every thread of a team.
template <int NV, int SMAX, class E, class Team = DeSolo>
struct DifferentialEvolution {
  static_assert(SMAX <= 1024, "de_pairwise halves at most three times");
  using Storage = DeStorage<NV, SMAX>;
  E &ev;
  Storage &st;
  Team team;
  int n, S;
  double arg1[NV], arg2[NV];  // __scale_arg1, __scale_arg2
  double tol, atol, cr, dither_lo, dither_hi, scale;
  bool dither;
  // the result
  long long nfev, redraws;
  int nit;
  bool success;
  double fun, x[NV];

  KPDI_HD DifferentialEvolution(E &e, Storage &s, Team t = Team()) : ev(e), st(s), team(t) {}

  struct EnergyAt {
    const double *e;
    KPDI_HD double operator()(int i) const { return e[i]; }
  };
  struct SquaredDeviationAt {
    const double *e;
    double mean;
    KPDI_HD double operator()(int i) const {
      const double d = e[i] - mean;
      return d * d;
    }
  };

  // _scale_parameters
  KPDI_HD void scale_parameters(const double *t, double *out) const {
    for (int j = 0; j < n; ++j) out[j] = arg1[j] + (t[j] - 0.5) * arg2[j];
  }

  // ---- what only the leader runs (it writes the storage)
  // _ensure_constraint over `count` values in order: only the entries outside [0, 1] are drawn again
  KPDI_HD void ensure_constraint(double *t, int count) {
    for (int i = 0; i < count; ++i) {
      if (t[i] > 1.0 || t[i] < 0.0) {
        KPDI_DE_HIT(oob_redraw);
        ++redraws;
        t[i] = mt_double(st.mt);
      } else {
        KPDI_DE_HIT(oob_inside);
      }
    }
  }

  // _select_samples(candidate, 5), of which best1 uses the first two
  KPDI_HD void select_samples(int candidate, int *r0, int *r1) {
#if KPDI_DE_WRONG == 4
    for (int i = 0; i < S; ++i) st.index[i] = i;  // wrong on purpose: a fresh index array per call
#endif
    mt_shuffle(st.mt, st.index, S);
    int got = 0, r[2] = {0, 0};
    const int head = S < 6 ? S : 6;
    for (int i = 0; i < head && got < 2; ++i) {
      if (st.index[i] == candidate) {
        KPDI_DE_HIT(sample_candidate_skipped);
        continue;
      }
      KPDI_DE_HIT(sample_taken);
      r[got++] = st.index[i];
    }
    *r0 = r[0];
    *r1 = r[1];
  }

  // _best1: population[0] + scale * (population[r0] - population[r1])
  KPDI_HD void best1(int r0, int r1, double *bprime) const {
    for (int j = 0; j < n; ++j) bprime[j] = st.population[0][j] + scale * (st.population[r0][j] - st.population[r1][j]);
  }

  // the binomial crossover of one trial: `out` holds bprime on entry
  KPDI_HD void crossover(int candidate, int fill_point, double *out) {
    for (int j = 0; j < n; ++j) {
      const double u = mt_double(st.mt);
      bool take = u < cr;
      if (j == fill_point) {
        KPDI_DE_HIT(cross_fill);
        take = true;
      } else if (take) {
        KPDI_DE_HIT(cross_drawn);
      } else {
        KPDI_DE_HIT(cross_kept);
      }
      if (!take) out[j] = st.population[candidate][j];
    }
  }

  // _mutate: the fill point, the samples, then the crossover draws
  KPDI_HD void mutate(int candidate, double *out) {
    const int fill_point = (int)mt_interval(st.mt, (uint32_t)(n - 1));
    int r0, r1;
    select_samples(candidate, &r0, &r1);
    best1(r0, r1, out);
    crossover(candidate, fill_point, out);
  }

  // _mutate_many in ITS order: every _select_samples, then every fill point, then every crossover draw
  KPDI_HD void mutate_many() {
#if KPDI_DE_WRONG == 1
    for (int c = 0; c < S; ++c) mutate(c, st.trial[c]);  // wrong on purpose: the draw order of _mutate
#else
    for (int c = 0; c < S; ++c) {
      int r0, r1;
      select_samples(c, &r0, &r1);
      best1(r0, r1, st.trial[c]);
    }
    for (int c = 0; c < S; ++c) st.fill[c] = (int)mt_interval(st.mt, (uint32_t)(n - 1));
    for (int c = 0; c < S; ++c) crossover(c, st.fill[c], st.trial[c]);
#endif
  }

  // np.argmin: the first NaN, else the first of the smallest
  KPDI_HD int argmin_energy() const {
    int l = 0;
    double m = st.energies[0];
    if (de_isnan(m)) {
      KPDI_DE_HIT(argmin_nan);
      return 0;
    }
    for (int i = 1; i < S; ++i) {
      const double e = st.energies[i];
      if (de_isnan(e)) {
        KPDI_DE_HIT(argmin_nan);
        return i;
      }
      if (e < m) {
        KPDI_DE_HIT(argmin_lower);
        m = e;
        l = i;
      } else {
        KPDI_DE_HIT(argmin_not_lower);
      }
    }
    return l;
  }

  // _promote_lowest_energy
  KPDI_HD void promote() {
    const int l = argmin_energy();
    if (l == 0) {
      KPDI_DE_HIT(promote_stay);
      return;
    }
    KPDI_DE_HIT(promote_swap);
    const double e = st.energies[0];
    st.energies[0] = st.energies[l];
    st.energies[l] = e;
    for (int j = 0; j < n; ++j) {
      const double v = st.population[0][j];
      st.population[0][j] = st.population[l][j];
      st.population[l][j] = v;
    }
  }

  // _accept_trial without constraints
  KPDI_HD static bool accepts(double energy_trial, double energy_orig) {
#if KPDI_DE_WRONG == 3
    return energy_trial < energy_orig;  // wrong on purpose: SciPy accepts an equal energy
#else
    return energy_trial <= energy_orig;
#endif
  }

  KPDI_HD void init_lhs() {
    KPDI_DE_HIT(init_lhs);
    const double segsize = 1.0 / (double)S;
    // np.linspace(0., 1., S, endpoint=False)[i] = i * (1.0 / S) + 0.0
    const double step = 1.0 / (double)S;
    for (int i = 0; i < S; ++i) {
      const double offset = (double)i * step + 0.0;
      for (int j = 0; j < n; ++j) st.trial[i][j] = segsize * mt_double(st.mt) + offset;
    }
    for (int j = 0; j < n; ++j) {
      mt_permutation(st.mt, st.fill, S);
      for (int i = 0; i < S; ++i) st.population[i][j] = st.trial[st.fill[i]][j];
    }
  }

  KPDI_HD void init_random() {
    KPDI_DE_HIT(init_random);
    for (int i = 0; i < S; ++i)
      for (int j = 0; j < n; ++j) st.population[i][j] = mt_double(st.mt);
  }

  // ---- what every thread runs
  // _calculate_population_energies of `rows` into `out`, in order
  KPDI_HD void evaluate(const double (*rows)[NV], double *out) {
    team.sync();  // the rows are written
    for (int i = 0; i < S; ++i) {
      double p[NV];
      scale_parameters(rows[i], p);
      const double f = ev.eval(p);
      ++nfev;
      if (team.leader()) out[i] = f;  // nobody reads `out` before the next barrier
    }
    team.sync();
  }

  KPDI_HD bool all_infinite() const {
    for (int i = 0; i < S; ++i)
      if (!de_isinf(st.energies[i])) return false;
    return true;
  }

  // converged(): no infinite energy and np.std(E) <= atol + tol * |np.mean(E)|
  KPDI_HD bool converged() const {
    for (int i = 0; i < S; ++i)
      if (de_isinf(st.energies[i])) {
        KPDI_DE_HIT(conv_infinite);
        return false;
      }
    const double count = (double)S;
    const double mean = (0.0 + de_pairwise<3>(EnergyAt{st.energies}, 0, S)) / count;
    const double var = (0.0 + de_pairwise<3>(SquaredDeviationAt{st.energies, mean}, 0, S)) / count;
    const double std_dev = std::sqrt(var);
    if (std_dev <= atol + tol * std::fabs(mean)) {
      KPDI_DE_HIT(conv_yes);
      return true;
    }
    KPDI_DE_HIT(conv_no);
    return false;
  }

  // __next__: one generation.  The storage is read by every thread only between two barriers with no leader write
  // in between.
  KPDI_HD void next(int deferred) {
    if (all_infinite()) {  // "the population may have just been initialized": evaluated again
      KPDI_DE_HIT(recalc_all_inf);
      evaluate(st.population, st.energies);
      if (team.leader()) promote();
    } else {
      KPDI_DE_HIT(recalc_not);
    }
    if (team.leader()) {
      if (dither) {
        KPDI_DE_HIT(dither_draw);
        scale = mt_uniform(st.mt, dither_lo, dither_hi);
      } else {
        KPDI_DE_HIT(dither_none);
      }
    }
    if (!deferred) {
      KPDI_DE_HIT(gen_immediate);
      for (int candidate = 0; candidate < S; ++candidate) {
        team.sync();  // every thread has read what the leader writes next
        if (team.leader()) {
          mutate(candidate, st.trial[0]);
          ensure_constraint(st.trial[0], n);
          scale_parameters(st.trial[0], st.xeval);
        }
        team.sync();
        double p[NV];
        for (int j = 0; j < n; ++j) p[j] = st.xeval[j];
        const double energy = ev.eval(p);
        ++nfev;
        team.sync();
        if (team.leader()) {
          if (accepts(energy, st.energies[candidate])) {
            KPDI_DE_HIT(trial_accepted);
            for (int j = 0; j < n; ++j) st.population[candidate][j] = st.trial[0][j];
            st.energies[candidate] = energy;
            if (accepts(energy, st.energies[0])) {
              KPDI_DE_HIT(imm_promote);
              promote();
            } else {
              KPDI_DE_HIT(imm_no_promote);
            }
          } else {
            KPDI_DE_HIT(trial_rejected);
          }
        }
      }
      team.sync();
    } else {
      KPDI_DE_HIT(gen_deferred);
      team.sync();
      if (team.leader()) {
        mutate_many();
        for (int c = 0; c < S; ++c) ensure_constraint(st.trial[c], n);  // row by row = the order of the 2-D mask
      }
      evaluate(st.trial, st.trial_energies);
      if (team.leader()) {
        for (int i = 0; i < S; ++i) {  // the np.where update
          if (accepts(st.trial_energies[i], st.energies[i])) {
            KPDI_DE_HIT(trial_accepted);
            for (int j = 0; j < n; ++j) st.population[i][j] = st.trial[i][j];
            st.energies[i] = st.trial_energies[i];
          } else {
            KPDI_DE_HIT(trial_rejected);
          }
        }
        promote();
      }
      team.sync();
    }
  }

  // differential_evolution(func, bounds, strategy="best1bin", maxiter, popsize -> members, tol, mutation, recombination,
  // seed, polish=False, init, atol, updating).  members = max(5, popsize * max(1, n - (lower == upper).sum())), which
  // the caller works out; mutation_hi = NaN: `mutation` is a float, else the sorted pair.  Leaves fun, x, nfev, nit,
  // success (and `redraws`, the values _ensure_constraint drew again).
  KPDI_HD void solve(int nvar, const double *lower, const double *upper, int members, int maxiter, double tol_, double atol_,
                     double mutation_lo, double mutation_hi, double recombination, int init, int deferred, uint32_t seed) {
    n = nvar;
    S = members;
    tol = tol_;
    atol = atol_;
    cr = recombination;
    dither = !de_isnan(mutation_hi);
    dither_lo = mutation_lo;
    dither_hi = mutation_hi;
    scale = mutation_lo;
    nfev = 0;
    redraws = 0;
    for (int j = 0; j < n; ++j) {
      arg1[j] = 0.5 * (lower[j] + upper[j]);
      arg2[j] = std::fabs(lower[j] - upper[j]);
    }
    if (team.leader()) {
      mt_seed(st.mt, seed);
      if (init == DE_INIT_RANDOM) init_random(); else init_lhs();
      for (int i = 0; i < S; ++i) {
        st.index[i] = i;
        st.energies[i] = HUGE_VAL;
      }
    }
    // solve(): the initial energies
    evaluate(st.population, st.energies);
    if (team.leader()) promote();
    team.sync();
    nit = 0;
    bool warning_flag = false;
    int generation = 1;
    for (; generation <= maxiter; ++generation) {
      nit = generation;
      next(deferred);
      if (converged()) {
        KPDI_DE_HIT(exit_converged);
        break;
      }
    }
    if (generation > maxiter) {  // the `else` of the for loop
      KPDI_DE_HIT(exit_maxiter);
      warning_flag = true;
    }
    success = !warning_flag;
    fun = st.energies[0];
    scale_parameters(st.population[0], x);
    team.sync();  // the storage may be reused once every thread has its result
  }
};

}  // namespace kpdi
