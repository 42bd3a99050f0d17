// match16_device.h - what the kernels on the match16 skeleton share (match16.hip: the float16 forms and the bounded
// float32 passes; match32.hip: the unbounded float32 form): the geometry of a variant, the MFMA statements, the LDS-DMA
// piece, the lists' and candidate buffers' scratch homes, the direct list build and the developer probe.
#pragma once
#include "match_device.h"
#include <stdlib.h>

namespace kpdi {

// Geometry of a variant.  Both share the operand layout (tiles of 256 patterns, steps of 48 pixels = 3 k-steps,
// a (tile, step) block of 24 KB) and the 256 x 256 workgroup tile over a ring of three 48 KB stages:
//   WAVES = 8: two waves per SIMD, wave tile 128 x 64  = 8 accumulators (128 architectural VGPRs), 6 fragment
//              reads per 8 MFMAs, 6 LDS-DMA pieces per wave and step;
//   WAVES = 4: one wave per SIMD, wave tile 128 x 128 = 16 accumulators (256 AGPRs), 8 fragment reads per 16
//              MFMAs (0.5 instead of 0.75 per MFMA: the LDS is what bounds the 8-wave form), 12 pieces per wave.
template <int WAVES>
struct Geo {
  static constexpr int DT = F16_TILE;                  // dictionary patterns per tile
  static constexpr int BK = F16_STEP;                  // pixels per step
  static constexpr int KS = BK / 16;                   // MFMA k-steps per step
  static constexpr int DBLOCK = DT * BK * 2;           // dictionary (tile, step) block, bytes
  static constexpr int EBLOCK = F16_TILE * BK * 2;     // experimental (tile, step) block, bytes
  static constexpr int STAGE = DBLOCK + EBLOCK;
  static constexpr int NSTAGE = 3;
  static constexpr int LDS = NSTAGE * STAGE;           // 144 KB (+ 32 B control words)
  static constexpr int NCG = WAVES == 8 ? 2 : 4;       // column groups (32 experimental patterns) of a wave tile
  static constexpr int WCOLS = 32 * NCG;               // experimental patterns of a wave tile
  static constexpr int WC = F16_TILE / WCOLS;          // waves side by side
  static constexpr int PIECES = STAGE / 1024 / WAVES;  // LDS-DMA pieces per wave and step: 6 / 12
  static constexpr int DPIECES = DBLOCK / 1024 / WAVES;  // ... of which dictionary: 3 / 6
  static constexpr bool ACC_A = WAVES == 4;            // accumulators in AGPRs
};

// acc += A x B for 16 pixels, A and B = 8 f16 per lane (one 16-byte LDS read).  The operands come from
// ds_read (lgkmcnt), never from a VALU write: no hazard padding needed inside the asm statement.
// 8-wave form: accumulators in architectural VGPRs (bare MFMA loop 1.41 vs 1.74 ms in AGPRs, and the
// epilogue reads them without v_accvgpr_read); 4-wave form: 256 accumulation registers = the AGPR file.
//
// The asm statement hides the MFMA from the compiler's hazard recogniser: whatever the compiler places behind it
// that touches the accumulator (a register copy, a spill) would read it before the matrix pipe has written it
// (8 passes: 11 wait states).  KPDI16_MFMA_NOPS puts those wait states into the statement itself; the shipped
// build instead keeps every accumulator in its registers throughout the loop, which tools/check_mfma_loops.py
// (run by the test suite) verifies on the generated code of every instantiation.
#ifdef KPDI16_MFMA_NOPS
#define KPDI16_MFMA_TAIL "\n\ts_nop 11"
#else
#define KPDI16_MFMA_TAIL
#endif
template <bool ACC_A>
__device__ __forceinline__ void mfma16(f32x16 &c, const f32x4 &a, const f32x4 &b) {
  if (ACC_A)
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" KPDI16_MFMA_TAIL : "+a"(c) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" KPDI16_MFMA_TAIL : "+v"(c) : "v"(a), "v"(b));
}

// float32 form: one v_mfma_f32_32x32x2_f32 per element j of the two 16-byte fragments (pixels j of lanes 0-31 and
// 4 + j of lanes 32-63 of an 8-pixel plane) - exact f32 products, the arithmetic of match.hip
__device__ __forceinline__ void mfma32(f32x16 &c, float a, float b) {
  asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

// One of a wave's 1 KB LDS-DMA pieces of a stage (i < DPIECES: dictionary block, else experimental
// block); piece q = wv + WAVES * i' of its block.  `gd` / `ge`: wave-uniform block addresses.
template <int WAVES>
__device__ __forceinline__ void issue_piece16(const char *gd, const char *ge, char *stage_base, int wv, int i,
                                              unsigned goff) {
  typedef Geo<WAVES> G;
  const bool is_exp = i >= G::DPIECES;
  const int q = wv + WAVES * (is_exp ? i - G::DPIECES : i);
  __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void *)(is_exp ? ge : gd), 0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(
      rsrc, (__attribute__((address_space(3))) void *)(stage_base + (is_exp ? G::DBLOCK : 0) + q * 1024), 16,
      (int)goff, q * 1024, 0, 0);
}

// Entry j of a list in its scratch home: `base` is wave-uniform; accesses are grouped in chunks of 16
// entries (4 KB = the immediate-offset range of a global access with a scalar base) whose base pointer is
// made opaque to the optimiser: otherwise it materialises one 64-bit address register PER ENTRY, hoists
// them out of the tile loop and spills them (1.2 KB of scratch per lane, a third of the kernel's time).
template <typename T>
__device__ __forceinline__ T *chunk_base(T *base, int chunk) {
  T *p = base + chunk * 16 * 64;
  asm volatile("" : "+s"(p));
  return p;
}

// One column group's 4 accumulators (128 dictionary rows x 32 patterns; 64 candidates per lane by
// increasing dictionary index) into the lane's list: first a screen with plain compares (bit r of
// `hot` = some lane of register r reaches the threshold), then only those registers go through the
// loop with the scalar register index (match.hip: scan_tile, FORM = 2).
// LEX: candidates may arrive in any order of dictionary index (the permuted tile order): thresholds are non-strict
// against a list's last entry and the insertion decides by (score, index).  !LEX (the 32-entry lists of the 8-wave
// form, which have no register to spare for it - tools/check_mfma_loops.py): natural tile order, strict thresholds,
// list_insert's arrival-order tie rule.
template <int KMAX, bool BOUNDED, bool F32 = false, bool LEX = true>
__device__ __forceinline__ void scan16(f32x16 (&acc)[4], float (&best)[KMAX], int (&best_idx)[KMAX], float gthr,
                                       float ub, int ub_idx, int row0, int n_valid, int idx_base, int rt_n = 4) {
  constexpr float unscale = F32 ? 1.f : 0x1p-24f;  // float16 operands are stored scaled by 2^12 each
  // (non-strict against the list's last entry: tiles arrive in a permuted order, so an equal score with a LOWER index
  // may still come - the insertion decides by (score, index))
  float thr = fmaxf(gthr, LEX ? best[KMAX - 1] : next_up(best[KMAX - 1]));
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    if (F32 && rt >= rt_n) continue;  // a partial unit of the float32 form's tail
    unsigned hot = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      hot |= __builtin_amdgcn_ballot_w64(acc[rt][r] * unscale + 0.f >= thr) != 0 ? (1u << r) : 0u;
#pragma unroll 1
    while (hot != 0) {
      const int r = __builtin_ctz(hot);
      hot &= hot - 1;
      const float v = acc[rt][r] * unscale + 0.f;  // -0 -> +0 so that ties compare as the merge does
      const int lrow = row0 + rt * 32 + (r & 3) + 8 * (r >> 2);
      const int idx = idx_base + lrow;
      bool ok = lrow < n_valid && v >= thr && (!LEX || ranks_before(v, idx, best[KMAX - 1], best_idx[KMAX - 1]));
      if (BOUNDED) ok = ok && (v < ub || (v == ub && idx > ub_idx));
      if (ok) {
        if (LEX) {
          list_insert_lex<KMAX>(best, best_idx, v, idx);
          thr = fmaxf(gthr, best[KMAX - 1]);
        } else {
          list_insert<KMAX>(best, best_idx, v, idx);
          thr = fmaxf(gthr, next_up(best[KMAX - 1]));
        }
      }
    }
  }
}

// Candidate buffers (per lane and column group, in the scratch behind the lists).  Grouped form of the shared
// bound (>= 32 lists per pattern, every list publishes its BEST entry - which needs no sorted list): the
// buffer takes everything that passes the bound, including all 64 candidates of the first tile, and the sorted
// list is built ONCE, at the end, from the buffered candidates that pass the FINAL bound (a handful): no list is
// loaded, updated or stored inside the tile loop unless a buffer overflows (adversarial data: long runs of
// equal scores).  After the first tile the bound sits near the 3 % quantile (the minimum over 32 slots of the
// best of 128 candidates), then rises like 1 / tiles: ~7 further candidates per lane over a whole launch.
// Plain form (few lists; a list publishes its j-th best, j > 1): the list is needed, the buffer holds 8.
#ifndef KPDI16_CAP
#define KPDI16_CAP 96
#endif
constexpr int CAND_CAP = KPDI16_CAP;  // a multiple of 16
constexpr int CAND_CAP_PLAIN = 8;

// ---- a list in its scratch home (`hs` / `hi`: wave-uniform, entry j at [j * 64 + lane]), N entries in chunks of 16
// (chunk_base above)
template <int N>
__device__ __forceinline__ void list_load(float *hs, int *hi, unsigned ulane, float (&best)[N], int (&bidx)[N]) {
#pragma unroll
  for (int q = 0; q < (N + 15) / 16; ++q) {
    const float *ps = chunk_base(hs, q);
    const int *pi = chunk_base(hi, q);
#pragma unroll
    for (int j = 16 * q; j < N && j < 16 * q + 16; ++j) {
      best[j] = ps[(j - 16 * q) * 64 + ulane];
      bidx[j] = pi[(j - 16 * q) * 64 + ulane];
    }
  }
}
template <int N>
__device__ __forceinline__ void list_store(float *hs, int *hi, unsigned ulane, const float (&best)[N], const int (&bidx)[N]) {
#pragma unroll
  for (int q = 0; q < (N + 15) / 16; ++q) {
    float *ps = chunk_base(hs, q);
    int *pi = chunk_base(hi, q);
#pragma unroll
    for (int j = 16 * q; j < N && j < 16 * q + 16; ++j) {
      ps[(j - 16 * q) * 64 + ulane] = best[j];
      pi[(j - 16 * q) * 64 + ulane] = bidx[j];
    }
  }
}
// N entries of "no entry" into a home (all lists of a lane at once)
template <int N>
__device__ __forceinline__ void list_clear(float *hs, int *hi, unsigned ulane) {
#pragma unroll
  for (int c = 0; c < (N + 15) / 16; ++c) {
    float *ps = chunk_base(hs, c);
    int *pi = chunk_base(hi, c);
#pragma unroll
    for (int j = 16 * c; j < N && j < 16 * c + 16; ++j) {
      ps[(j - 16 * c) * 64 + ulane] = -INFINITY;
      pi[(j - 16 * c) * 64 + ulane] = INT_MAX;
    }
  }
}
// ---- developer builds (tools/build_variant.sh): cycle counters and statistics of ONE kernel, printed from it.  The
// kernel and its stages call the probe's methods at fixed points; in the shipped build the four flags are false and every method folds to nothing.
//   KPDI16_TIME_PHASES  cycles of a launch's phases (tools/probes/share_step.py; profiles/r06_launch_phases.txt)
//   KPDI16_TIME_EPI     where the cycles between tiles go (tools/probes/one_step.py)
//   KPDI16_EPI_STATS    per tile, what the epilogue of ONE wave did (tools/probes/one_step.py; profiles/r05_f32_tile_time.txt)
//   KPDI16_EPI_FINE     cycles of the three parts of a block's epilogue (same tools, same record)
#ifdef KPDI16_TIME_PHASES
constexpr bool PROBE_PHASES = true;
#else
constexpr bool PROBE_PHASES = false;
#endif
#ifdef KPDI16_TIME_EPI
constexpr bool PROBE_EPI = true;
#else
constexpr bool PROBE_EPI = false;
#endif
#ifdef KPDI16_EPI_STATS
constexpr bool PROBE_STATS = true;
#else
constexpr bool PROBE_STATS = false;
#endif
#ifdef KPDI16_EPI_FINE
constexpr bool PROBE_FINE = true;
#else
constexpr bool PROBE_FINE = false;
#endif
struct Probe16 {
  typedef unsigned long long u64;
  u64 ph_t0, ph_prologue = 0, ph_first_loop = 0, ph_first_epi = 0, ph_loop_end = 0, ph_epi_t0 = 0;
  u64 ph_fs_bound = 0, ph_fs_loop = 0, fs0 = 0, fs2 = 0;
  int ph_fs_iters = 0, ph_fs_inserts = 0;
  int st_hot = 0, st_iter = 0, st_cand = 0;
  u64 st_t0 = 0;
  u64 fine_screen = 0, fine_pm = 0, fine_loop = 0, f0 = 0, f1 = 0, f2 = 0;
  int fine_blocks = 0;
  u64 epi_cycles = 0, epi_drain = 0, epi_t0 = 0, kern_t0 = 0;
  static __device__ __forceinline__ u64 now() { return __builtin_readcyclecounter(); }
  __device__ __forceinline__ Probe16() : ph_t0(PROBE_PHASES ? now() : 0) {}
  __device__ __forceinline__ void mark_prologue() {
    if (PROBE_PHASES) ph_prologue = now() - ph_t0;
  }
  __device__ __forceinline__ void loop_begin() {
    if (PROBE_EPI) kern_t0 = now();
  }
  // behind a tile's last step
  __device__ __forceinline__ void tile_begin(int tiles_done) {
    if (PROBE_EPI) epi_t0 = now();
    if (PROBE_PHASES) {
      ph_epi_t0 = now();
      if (tiles_done == 0) ph_first_loop = ph_epi_t0 - ph_t0 - ph_prologue;
    }
  }
  __device__ __forceinline__ void drain_done() {
    if (PROBE_EPI) epi_drain += now() - epi_t0;
    if (PROBE_STATS) {
      st_hot = st_iter = st_cand = 0;
      st_t0 = now();
    }
  }
  // a block of 16 accumulator registers: its screen, the mask of a hot block, the append loop
  __device__ __forceinline__ void block_begin() {
    if (PROBE_FINE) f0 = now();
  }
  __device__ __forceinline__ void hot_block() {
    if (PROBE_FINE) f1 = now();
    if (PROBE_STATS) ++st_hot;
  }
  __device__ __forceinline__ void mask_done(unsigned &pm) {
    if (PROBE_FINE) {
      asm volatile("" : "+v"(pm));
      f2 = now();
    }
  }
  __device__ __forceinline__ void append_iteration(unsigned pm) {
    if (PROBE_STATS) {
      ++st_iter;
      st_cand += __builtin_popcountll(__builtin_amdgcn_ballot_w64(pm != 0));
    }
  }
  __device__ __forceinline__ void hot_block_end() {
    if (PROBE_FINE) {
      const u64 f3 = now();
      fine_screen += f1 - f0;
      fine_pm += f2 - f1;
      fine_loop += f3 - f2;
      ++fine_blocks;
    }
  }
  __device__ __forceinline__ void tile_end(int tiles_done, bool first_fast, int wv, int lane) {
    if (PROBE_EPI) epi_cycles += now() - epi_t0;
    if (PROBE_STATS) {
      const u64 dt = now() - st_t0;
      if (blockIdx.x == 100 && lane == 0 && wv == 0)
        printf("tile %d: %llu cycles, %d hot blocks of 16, %d loop iterations, %d candidates of the wave, first_fast %d\n", tiles_done, dt,
               st_hot, st_iter, st_cand, (int)first_fast);
    }
    if (PROBE_PHASES) {
      if (tiles_done == 0) ph_first_epi = now() - ph_epi_t0;
      ph_loop_end = now() - ph_t0;
    }
  }
  __device__ __forceinline__ void loop_report(int tiles_done, int wv, int lane) {
    if (PROBE_FINE && blockIdx.x == 100 && lane == 0)
      printf("wave %d: %d hot blocks: screen %llu, mask %llu, loop %llu cycles per hot block\n", wv, fine_blocks, fine_screen / fine_blocks,
             fine_pm / fine_blocks, fine_loop / fine_blocks);
    if (PROBE_EPI && (blockIdx.x == 0 || blockIdx.x == 100) && lane == 0)
      printf("block %d wave %d: %d tiles, %llu cycles between tiles (%llu of them waiting for the last MFMAs) of %llu in the tile loop "
             "(%.2f %%)\n", (int)blockIdx.x, wv, tiles_done, epi_cycles, epi_drain, now() - kern_t0,
             100.0 * epi_cycles / (double)(now() - kern_t0));
  }
  // the final stage: its bound, a batch of 16 buffered candidates (direct path: stores; sorted path: insertions)
  __device__ __forceinline__ void final_begin() {
    if (PROBE_PHASES) fs0 = now();
  }
  __device__ __forceinline__ void final_bound(float &tf) {
    if (PROBE_PHASES) {
      asm volatile("" : "+v"(tf));
      ph_fs_bound += now() - fs0;
    }
  }
  __device__ __forceinline__ void final_direct_begin() {
    if (PROBE_PHASES) fs2 = now();
  }
  __device__ __forceinline__ void final_batch_begin(unsigned &pm) {
    if (PROBE_PHASES) {
      asm volatile("" : "+v"(pm));
      fs2 = now();
    }
  }
  __device__ __forceinline__ void final_insert() {
    if (PROBE_PHASES) ++ph_fs_inserts;
  }
  __device__ __forceinline__ void final_batch_end() {
    if (PROBE_PHASES) {
      ph_fs_loop += now() - fs2;
      ++ph_fs_iters;
    }
  }
  __device__ __forceinline__ void report(int wv, int lane) {
    if (PROBE_PHASES) {
      const u64 end = now() - ph_t0;
      if ((blockIdx.x == 0 || blockIdx.x == 100 || blockIdx.x == 255) && lane == 0 && wv == 0)
        printf("block %d: prologue %llu, first tile's steps %llu, first epilogue %llu, tile loop ends at %llu, final stage %llu, kernel %llu cycles "
               "(shader cycles); final stage: bound loads %llu, insert loops %llu (%d batches, %d insertions)\n", (int)blockIdx.x, ph_prologue,
               ph_first_loop, ph_first_epi, ph_loop_end, end - ph_loop_end, end, ph_fs_bound, ph_fs_loop, ph_fs_iters, ph_fs_inserts);
    }
  }
};

// ---- a candidate that passed the screen into the lane's candidate buffer (`c` entries so far, `cap` at most; `mx`:
// the best score appended from this tile; a full buffer: `overflow`) - shared by the two append forms of the epilogue
__device__ __forceinline__ void append16(float *bs, int *bi, unsigned ulane, int cap, int &c, float &mx, bool &overflow, float v,
                                         int idx) {
  if (c < cap) {
    bs[c * 64 + ulane] = v;
    bi[c * 64 + ulane] = idx;
    ++c;
    mx = fmaxf(mx, v);
  } else {
    overflow = true;
  }
}

// floats (and as many ints) a kernel of this skeleton keeps per launch: the lists and the candidate buffers behind them
inline size_t scratch16_entries(int grid, int waves, int list_len) {
  (void)waves;  // waves x column groups per wave = 16 lists per lane position in both forms
  return (size_t)grid * 16 * (list_len + CAND_CAP) * 64;
}

// match32.hip: the unbounded float32 form (operand_form 3) - same operands, scratch and MatchArgs as match16_kernel<.., 4, true>
hipError_t launch_match32(const MatchArgs &g, int list_len, int grid, void *scratch, hipStream_t s);

}  // namespace kpdi
