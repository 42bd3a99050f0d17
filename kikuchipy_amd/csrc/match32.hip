// match32.hip - the unbounded pass of the float32 form (operand_form 3): match16_kernel<KMAX, false, 4, true> of
// match16.hip with the MFMA step instantiated twice inside one persistent kernel.  Operands, MatchArgs, scratch, lists,
// candidate buffers, the bound line, the tile order, the first-tile fast path, the epilogue and the final stage are those
// of match16.hip (the shared pieces: match16_device.h); the MFMA sequence of every accumulator is the same, so the
// scores are bit for bit the same.
//
// What differs is the step loop:
//  * WHOLE tiles (units below a.tail_first - every unit of a launch but those of its last round) run a step without
//    `rt_n`: the `rt < rt_n` guard of the shared template is a VALU -> SGPR -> branch chain in front of every group of
//    four MFMAs (48 per step, 7200 per tile) that is only ever taken by the partial units of the tail.  Those keep the
//    guarded step, the second instance.
//  * No result of a global load is live into either step loop: the bound refresh sits between a tile's last step and
//    its accumulator drain (it was at the head of the last step, inside the loop, where the registers its loads
//    clobber made the compiler drain the load counter at the head of EVERY step - with the LDS-DMA pieces of the
//    step before in flight).  The bound is read later than before, never earlier: it is a filter, any value that ever
//    stood is valid.
//  * The load cursor's scalar arithmetic (which tile, which addresses, the advance) is spread over MFMA groups inside
//    the step instead of standing at its head and tail, where the in-order wave ran it with the matrix pipe empty.
// tests/test_build_match32.py checks the generated code of every instantiation: between the first and the last MFMA of
// the whole-tile step there is no branch, no scratch access and one load-counter wait - the source's, in front of the
// step's barrier - and nothing goes through scratch inside either step.  (tools/check_mfma_loops.py takes a kernel's
// first to last MFMA as ONE loop; here the tile loop's own code lies between the two steps, so that test looks at each.)
#include "match16_device.h"
#include <type_traits>

namespace kpdi {

// (markers in the assembly for tests/test_build_match32.py: comments, no instructions)
#define KPDI32_MARK(text) asm volatile("; kpdi32 " text)

template <int KMAX>
__global__ __launch_bounds__(256, 1) void match32_kernel(MatchArgs a, float *ls_scores, int *ls_idx) {
  constexpr int WAVES = 4;
  typedef Geo<WAVES> G;
  constexpr int NCG = G::NCG;
  constexpr int BLOCK16 = G::DBLOCK, STAGE16 = G::STAGE, NSTAGE16 = G::NSTAGE, KSTEPS16 = G::KS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Probe16 probe;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0 .. 3
  const int wr = wv / G::WC, wc = wv % G::WC;
  int sp, rb;
  block_rb_sp(a, blockIdx.x, &rb, &sp);
  if (rb >= a.rows) return;  // (a workgroup of the padding of the XCD grid: whole workgroup, before any barrier)
  rb += a.row_first;
  const int n_tiles = a.n_tiles, n_valid = a.n_valid, idx_base = a.idx_base;
  const int nsteps = (2 * a.kpad) / G::BK;
  const size_t tile_bytes = (size_t)nsteps * G::DBLOCK;   // one dictionary tile, all steps
  const size_t etile_bytes = (size_t)nsteps * G::EBLOCK;  // one 256-pattern experimental tile
  const unsigned goff = (unsigned)lane * 16u;
  const char *exp_base = (const char *)a.exp + (size_t)rb * etile_bytes;
  const char *dict_base = (const char *)a.dict;

  // LDS -> MFMA fragments (match16.hip): lane l reads row (l & 31) of a 32-row group in plane ks, the 16-byte half
  // (l >> 5) of the row's 32 bytes, halves swapped for rows with bit 3 set; the rows of this wave within the tile
  // change with the unit - fa_base below
  const unsigned half_off = (unsigned)((((lane >> 5) ^ (lane >> 3)) & 1) * 16);
  const unsigned fa_lane = (unsigned)((lane & 31) * 32) + half_off;
  unsigned fa_off = (unsigned)(wr * 128 * 32) + fa_lane;
  const unsigned fb_off = (unsigned)(BLOCK16 + (wc * G::WCOLS + (lane & 31)) * 32) + half_off;
#define KPDI_FA(base, rt, ks) (*(const f32x4 *)((base) + fa_off + (rt) * 1024 + (ks) * (G::DT * 32)))
#define KPDI_FB(base, cg, ks) (*(const f32x4 *)((base) + fb_off + (cg) * 1024 + (ks) * (F16_TILE * 32)))

  // ==== STAGE: set-up - this lane's list and candidate-buffer homes, the bound line and slot (match16.hip)
  const int m_lane = rb * F16_TILE + wc * G::WCOLS + (lane & 31);
  float *home_s = ls_scores + (((size_t)blockIdx.x * WAVES + wv) * NCG) * KMAX * 64;
  int *home_i = ls_idx + (((size_t)blockIdx.x * WAVES + wv) * NCG) * KMAX * 64;
  const unsigned ulane = (unsigned)lane;
  unsigned built = 0u;  // bit cg: the list of column group cg has been built (its home holds nothing before)
  const size_t n_list_entries = (size_t)gridDim.x * WAVES * NCG * KMAX * 64;
  float *buf_s = ls_scores + n_list_entries + (((size_t)blockIdx.x * WAVES + wv) * NCG) * CAND_CAP * 64;
  int *buf_i = ls_idx + n_list_entries + (((size_t)blockIdx.x * WAVES + wv) * NCG) * CAND_CAP * 64;
  float last[NCG], pub[NCG], g[NCG];
  int cnt[NCG];
#pragma unroll
  for (int cg = 0; cg < NCG; ++cg) {
    last[cg] = pub[cg] = g[cg] = -INFINITY;
    cnt[cg] = 0;
  }
  const unsigned *line0 = a.gthr + (size_t)m_lane * BOUND_SLOTS;  // column group cg: + 32 cg BOUND_SLOTS
  const int list_id = sp * 4 + wr * 2 + (lane >> 5);
  const int my_slot = list_id & (BOUND_SLOTS - 1);
  const int bound_rank = a.bound_rank;
  const bool bound_grouped = a.bound_grouped != 0;
  const int cap = bound_rank == 1 ? CAND_CAP : CAND_CAP_PLAIN;

  // ==== STAGE: the unit and tile cursor (match16.hip: static hand-out, units of the tail, permuted order of the whole
  // rounds).  t0 / t1 / t2 stay plain locals.
  const int tail_first = a.tail_first, tail_shift = a.tail_shift;
  const int n_units = tail_first + ((n_tiles - tail_first) << tail_shift);
#define KPDI16_UNIT_TILE(u) ((u) < tail_first ? (u) : tail_first + (((u) - tail_first) >> tail_shift))
#define KPDI16_UNIT_ROW(u) ((u) < tail_first ? 0 : ((((u) - tail_first) & ((1 << tail_shift) - 1)) * (F16_TILE >> tail_shift)))
#define KPDI16_UNIT_RT(u) ((u) < tail_first ? 4 : (4 >> tail_shift))
  const int perm_rounds = a.perm_rounds, perm_stride = a.perm_stride;
  int seq_round = 0, seq_pos = 0;
  auto next_unit = [&]() {
    int u;
    if (seq_round < perm_rounds) {
      u = sp + a.nsplit * seq_pos;
      seq_pos += perm_stride;
      if (seq_pos >= perm_rounds) seq_pos -= perm_rounds;
    } else {
      u = sp + a.nsplit * seq_round;
    }
    ++seq_round;
    return u;
  };
  int t0 = next_unit(), t1 = next_unit(), t2 = next_unit();
  if (t0 < n_units) {
    const int last_tile = n_tiles - 1;
    int ld_pos = 0, ld_step = 0, ld_stage = 0;
    const char *gd = nullptr, *ge = nullptr;
#define KPDI16_CURSOR_SET()                                                          \
  {                                                                                  \
    int t_ = ld_pos == 0 ? t0 : (ld_pos == 1 ? t1 : t2);                             \
    t_ = KPDI16_UNIT_TILE(t_);                                                       \
    t_ = t_ < last_tile ? t_ : last_tile; /* past the end: harmless re-load */       \
    gd = dict_base + (size_t)t_ * tile_bytes + (size_t)ld_step * G::DBLOCK;          \
    ge = exp_base + (size_t)ld_step * G::EBLOCK;                                     \
  }
#define KPDI16_CURSOR_ADVANCE()                                \
  {                                                            \
    if (++ld_step == nsteps) {                                 \
      ld_step = 0;                                             \
      ++ld_pos;                                                \
    }                                                          \
    ld_stage = ld_stage == NSTAGE16 - 1 ? 0 : ld_stage + 1;    \
  }
    // ---- prologue: steps 0 and 1 in flight, then landed and visible
    KPDI16_CURSOR_SET();
#pragma unroll
    for (int i = 0; i < G::PIECES; ++i) issue_piece16<WAVES>(gd, ge, smem + ld_stage * STAGE16, wv, i, goff);
    KPDI16_CURSOR_ADVANCE();
    KPDI16_CURSOR_SET();
#pragma unroll
    for (int i = 0; i < G::PIECES; ++i) issue_piece16<WAVES>(gd, ge, smem + ld_stage * STAGE16, wv, i, goff);
    KPDI16_CURSOR_ADVANCE();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    probe.mark_prologue();

    // rows of this wave in a unit: 32 * rt_n consecutive rows from unit row + wr * 32 * rt_n
    auto fa_base = [&](int u) { return (unsigned)((KPDI16_UNIT_ROW(u) + wr * 32 * KPDI16_UNIT_RT(u)) * 32) + fa_lane; };
    fa_off = fa_base(t0);
    // fragments of the three k-steps of a step, each in its own registers (static indices)
    f32x4 fa[KSTEPS16][4], fb[KSTEPS16][NCG];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) fa[0][rt] = KPDI_FA(smem, rt, 0);
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) fb[0][cg] = KPDI_FB(smem, cg, 0);

    int stage = 0;
    int tiles_done = 0, refresh_at = 0;
    probe.loop_begin();
#pragma clang loop unroll(disable)
    for (;;) {  // dictionary tiles (units)
      const int rt_n = KPDI16_UNIT_RT(t0);  // row groups of this wave in this unit
      f32x16 acc[NCG][4];                   // [column group][32-row group]
#pragma unroll
      for (int cg = 0; cg < NCG; ++cg)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[cg][rt][r] = 0.f;
      // ==== STAGE: the MFMA loop - per step: fragment reads, MFMAs, DMA issue, one barrier.  64 MFMAs of 64 pipe cycles
      // per k-step; behind every four of them one of the 8 fragment reads of the next k-step, then (after the barrier)
      // this wave's 6 LDS-DMA pieces.  WHOLE: all four row groups, nothing to test between the MFMAs; !WHOLE: a partial
      // unit of the tail runs 2 or 1 of its row groups (the schedule stays).
      auto steps = [&](auto whole) __attribute__((always_inline)) {
        constexpr bool WHOLE = decltype(whole)::value;
        // (the load cursor spread over the step, below: whole tiles only, and not in the 8-entry instantiation - with
        // it, in either instance of the step, that one reloads two fragments from scratch inside the partial units'
        // loop, tests/test_build_match32.py)
        constexpr bool SPREAD = WHOLE && KMAX != 8;
        // (nothing a load from memory has written is read inside the loop before this point: the scratch reloads of
        // addresses and lane offsets in front of the loop are complete here, once, not at the head of every step)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma clang loop unroll(disable)
        for (int step = 0; step < nsteps; ++step) {
          if (WHOLE) KPDI32_MARK("whole step begin");
          const char *ls = smem + stage * STAGE16;
          const int nstage = stage == NSTAGE16 - 1 ? 0 : stage + 1;
          const char *ls_next = smem + nstage * STAGE16;
          if (!SPREAD) KPDI16_CURSOR_SET();
          char *ld_base = smem + ld_stage * STAGE16;
          int cur_t = 0;  // SPREAD: the load cursor's tile, worked out in four pieces during k-step 0 (below)
#pragma unroll
          for (int ks = 0; ks < KSTEPS16; ++ks) {
            if (ks == 1) {
              // ---- the step's only synchronisation point: this wave's pieces of step + 1 (issued during
              // the previous step) have landed; after the barrier step + 1 is complete in LDS and every
              // wave is past the previous step, whose stage is refilled below
#ifndef KPDI16_NO_BARRIER
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              __syncthreads();
#endif
            }
            const int nk = ks == KSTEPS16 - 1 ? 0 : ks + 1;       // fragments read during this k-step
            const char *src = ks == KSTEPS16 - 1 ? ls_next : ls;  // ... of the next step for the last one
            if (ks == KSTEPS16 - 1 && step == nsteps - 1) fa_off = fa_base(t1);  // those are the next unit's rows
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int rt = 0; rt < 4; ++rt) {
                if (WHOLE || rt < rt_n) {
#pragma unroll
                  for (int cg = 0; cg < NCG; ++cg) mfma32(acc[cg][rt], fa[ks][rt][j], fb[ks][cg][j]);
                }
                const int slot = 4 * j + rt;
                // ---- the load cursor (KPDI16_CURSOR_SET / _ADVANCE, a piece at a time): one wave per SIMD issues in
                // order, so scalar work is hidden only in the 64 pipe cycles behind an MFMA - about a dozen
                // instructions.  At the head and the tail of the step the cursor's ~55 ran in one gap, the matrix pipe
                // empty for most of them (3 % of a step).  Its pieces sit behind MFMA groups of k-step 0 that carry no
                // fragment read (gd / ge are first used by the DMA issues of k-step 1), the advance behind the last
                // DMA issue of the step.  The select is written with masks: as `?:` it became branches.
                if (SPREAD && ks == 0 && slot == 8) {
                  const int p0 = -(int)(ld_pos == 0), p1 = -(int)(ld_pos == 1);
                  cur_t = (t0 & p0) | (t1 & p1) | (t2 & ~(p0 | p1));
                }
                if (SPREAD && ks == 0 && slot == 9) {
                  cur_t = KPDI16_UNIT_TILE(cur_t);
                  cur_t = cur_t < last_tile ? cur_t : last_tile;  // past the end: harmless re-load
                }
                if (SPREAD && ks == 0 && slot == 10) gd = dict_base + (size_t)cur_t * tile_bytes + (size_t)ld_step * G::DBLOCK;
                if (SPREAD && ks == 0 && slot == 11) ge = exp_base + (size_t)ld_step * G::EBLOCK;
                if (SPREAD && ks == KSTEPS16 - 1 && slot == 14) KPDI16_CURSOR_ADVANCE();
#ifndef KPDI16_NO_READS  // (timing-only ablation builds, tools/f32_loop_ab.sh: as in match16.hip)
                if (slot < 4) fa[nk][slot] = KPDI_FA(src, slot, nk);
                else if (slot < 8) fb[nk][slot - 4] = KPDI_FB(src, slot - 4, nk);
#endif
#ifndef KPDI16_NO_DMA
                if (ks >= 1 && slot >= 8 && slot < 8 + 6) issue_piece16<WAVES>(gd, ge, ld_base, wv, (ks - 1) * 6 + slot - 8, goff);
#endif
                __builtin_amdgcn_sched_barrier(0);
              }
          }
          if (!SPREAD) KPDI16_CURSOR_ADVANCE();
          stage = nstage;
          if (WHOLE) KPDI32_MARK("whole step end");
        }  // steps
      };
      if (t0 < tail_first)
        steps(std::true_type());
      else
        steps(std::false_type());
      // ---- the shared bound of this wave's patterns, for the epilogue: all lines in flight, then reduced (a wait of
      // one memory latency under the tile's last MFMAs); refreshed after the tiles 0, 1, 2, 4, 7, 11, 17, 26 ... of a
      // workgroup: the bound rises like the logarithm of the candidates seen, and a bound that is a few tiles old lets
      // 1.5 x as many of the ~0.1 candidates per lane pass
      if (tiles_done >= refresh_at) {
        BoundHalf raw[NCG];
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg) bound_load_half(raw[cg], line0 + 32 * cg * BOUND_SLOTS, lane >> 5);
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg) g[cg] = bound_reduce_half<KMAX>(raw[cg], bound_grouped, lane >> 5);
        refresh_at = tiles_done + 1 + (tiles_done >> 1);
      }
      probe.tile_begin(tiles_done);
      // ==== STAGE: the accumulator drain: the last MFMAs (8 passes) must have written the accumulators before they are
      // read (the pipe retires MFMAs in order: ONE wait covers all of them; the empty statements only tie every
      // accumulator to this point)
#pragma unroll
      for (int cg = 0; cg < NCG; ++cg)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
          if (cg == 0 && rt == 0)
            asm volatile("s_nop 15\n\ts_nop 7" : "+a"(acc[cg][rt]));
          else
            asm volatile("" : "+a"(acc[cg][rt]));
        }
      probe.drain_done();
      {
        // ---- epilogue of the tile (match16.hip): the accumulators are screened against the bound, the few candidates
        // that pass are appended to the lane's candidate buffer; the sorted list is only built when a buffer is full
        const int row0 = KPDI16_UNIT_TILE(t0) * G::DT + KPDI16_UNIT_ROW(t0) + wr * 32 * rt_n + 4 * (lane >> 5);
        // ==== STAGE: first-tile fast path - publish the maxima, poll the bound -> first_fast
        bool first_fast = false;
        if (tiles_done == 0 && bound_rank == 1 && bound_grouped && KPDI16_UNIT_TILE(t0) * G::DT + G::DT <= n_valid) {
#pragma unroll
          for (int cg = 0; cg < NCG; ++cg) {
            float m = -INFINITY;
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
              if (rt >= rt_n) continue;
#pragma unroll
              for (int r = 0; r < 16; ++r) m = fmaxf(m, acc[cg][rt][r]);
            }
            m = m + 0.f;
            if (m > pub[cg]) {
              pub[cg] = m;
              __hip_atomic_fetch_max(const_cast<unsigned *>(line0) + 32 * cg * BOUND_SLOTS + my_slot, score_key(m),
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
#pragma unroll 1
          for (int it = 0; it < 48 && !first_fast; ++it) {
            BoundHalf raw[NCG];
#pragma unroll
            for (int cg = 0; cg < NCG; ++cg) bound_load_half(raw[cg], line0 + 32 * cg * BOUND_SLOTS, lane >> 5);
            bool ready = true;
#pragma unroll
            for (int cg = 0; cg < NCG; ++cg) {
              g[cg] = bound_reduce_half<KMAX>(raw[cg], bound_grouped, lane >> 5);
              ready = ready && g[cg] > -INFINITY;
            }
            first_fast = __builtin_amdgcn_ballot_w64(!ready) == 0;
            if (!first_fast) __builtin_amdgcn_s_sleep(24);
          }
        }
        // ==== STAGE: screen-and-append, per column group
        // index of a built list's last entry (a candidate that TIES with it passes only with a lower index: tiles
        // arrive in a permuted order); lists are rarely built before the end - then nothing is loaded
        int lidx[NCG];
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg) {
          lidx[cg] = INT_MAX;
          if ((built >> cg) & 1) lidx[cg] = chunk_base(home_i + cg * KMAX * 64, (KMAX - 1) / 16)[((KMAX - 1) % 16) * 64 + ulane];
        }
#pragma unroll
        for (int cg = 0; cg < NCG; ++cg) {
#ifdef KPDI16_NO_EPILOGUE  // (the MFMAs are asm volatile: they stay)
          continue;
#endif
          const float thr = fmaxf(g[cg], last[cg]);
          float *bs = buf_s + cg * CAND_CAP * 64;
          int *bi = buf_i + cg * CAND_CAP * 64;
          unsigned *line = const_cast<unsigned *>(line0) + 32 * cg * BOUND_SLOTS;
          int c = cnt[cg];
          // (the FIRST tile of a launch without the fast path goes the way of a full buffer: the list is built from the
          // accumulators directly)
          const bool first_tile = tiles_done == 0 && !first_fast;
          bool overflow = first_tile;
          float mx = -INFINITY;
#pragma unroll
          for (int rt = 0; rt < 4; ++rt) {
            if (first_tile) continue;
            if (rt >= rt_n) continue;
            probe.block_begin();
            float m = acc[cg][rt][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) m = fmaxf(m, acc[cg][rt][r]);
            if (__builtin_amdgcn_ballot_w64(m >= thr) == 0) continue;  // wave-uniform
            // ---- some lane of this block of 16 registers holds a candidate: a per-lane bit mask with vector
            // instructions only, then ONE loop, as long as any lane has a bit left (lowest bit = ascending dictionary index)
            probe.hot_block();
            unsigned pm = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) pm |= acc[cg][rt][r] >= thr ? (1u << r) : 0u;
            probe.mask_done(pm);
#pragma unroll 1
            while (__builtin_amdgcn_ballot_w64(pm != 0) != 0) {
              probe.append_iteration(pm);
              if (pm != 0) {
                const int r = __builtin_ctz(pm);
                pm &= pm - 1;
                float raw = acc[cg][rt][0];
#pragma unroll
                for (int q = 1; q < 16; ++q) raw = r == q ? acc[cg][rt][q] : raw;
                const int lrow = row0 + rt * 32 + (r & 3) + 8 * (r >> 2);
                const float v = raw + 0.f;  // -0 -> +0 so that ties compare as the merge does
                const int idx = idx_base + lrow;
                const bool ok = lrow < n_valid && (v > last[cg] || idx < lidx[cg]);
                if (ok) append16(bs, bi, ulane, cap, c, mx, overflow, v, idx);
              }
            }
            probe.hot_block_end();
          }
          if (__builtin_amdgcn_ballot_w64(overflow) == 0) {
            cnt[cg] = c;
            // grouped form of the shared bound (every list publishes its best entry): the best buffered
            // candidate counts as well
            if (bound_rank == 1 && mx > pub[cg]) {
              pub[cg] = mx;
              __hip_atomic_fetch_max(line + my_slot, score_key(mx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          } else {
            // ==== STAGE: the overflow rebuild - load or empty the list, replay the buffer, scan16, store, publish
            float best[KMAX];
            int bidx[KMAX];
            float *hs = home_s + cg * KMAX * 64;
            int *hi = home_i + cg * KMAX * 64;
            if ((built >> cg) & 1) {
              list_load<KMAX>(hs, hi, ulane, best, bidx);
            } else {  // (never built: the empty list)
#pragma unroll
              for (int j = 0; j < KMAX; ++j) {
                best[j] = -INFINITY;
                bidx[j] = INT_MAX;
              }
              built |= 1u << cg;
            }
#pragma unroll 1
            for (int i = 0; __builtin_amdgcn_ballot_w64(i < cnt[cg]) != 0; ++i) {
              if (i < cnt[cg]) {
                const float v = bs[i * 64 + ulane];
                const int id = bi[i * 64 + ulane];
                if (ranks_before(v, id, best[KMAX - 1], bidx[KMAX - 1])) list_insert_lex<KMAX>(best, bidx, v, id);
              }
            }
            if (a.epi_stats) {  // (developer counters, profiling level 3: what was appended before this list was built)
              const unsigned app = wave_sum_u32((unsigned)cnt[cg]);
              if (lane == 0) {
                atomicAdd(a.epi_stats + 1, (unsigned long long)app);
                atomicAdd(a.epi_stats + (first_tile ? 3 : 2), 1ull);
              }
            }
            cnt[cg] = 0;
            scan16<KMAX, false, true, true>(acc[cg], best, bidx, g[cg], INFINITY, -1, row0, n_valid, idx_base, rt_n);
            list_store<KMAX>(hs, hi, ulane, best, bidx);
            last[cg] = best[KMAX - 1];
            float now = best[0];  // the entry the shared bound is built from
#pragma unroll
            for (int j = 1; j < KMAX; ++j) now = j == bound_rank - 1 ? best[j] : now;
            if (now > pub[cg]) {
              pub[cg] = now;
              __hip_atomic_fetch_max(line + my_slot, score_key(now), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
        }
        probe.tile_end(tiles_done, first_fast, wv, lane);
        ++tiles_done;
        t0 = t1;
        t1 = t2;
        t2 = next_unit();
        --ld_pos;
        if (t0 >= n_units) break;
      }
    }
    probe.loop_report(tiles_done, wv, lane);
  }

  // ==== STAGE: the final stage (match16.hip): the buffered candidates that pass the FINAL shared bound join their lists
  // (in arrival order), then lists -> [m_pad][lists][KMAX] for the merge kernel
  {
    const int lists = 4 * a.nsplit;
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      const size_t ol = (size_t)(m_lane + 32 * cg) * lists + (size_t)list_id, o = ol * KMAX;
      probe.final_begin();
      // (any bound that ever stood is valid; the one this wave refreshed last is nearly the final one and costs nothing)
      float tf = g[cg];
      if (__builtin_amdgcn_ballot_w64(!(tf > -INFINITY)) != 0) tf = shared_bound<KMAX>(line0 + 32 * cg * BOUND_SLOTS, bound_grouped);
      probe.final_bound(tf);
      if (!((built >> cg) & 1)) {
        // ---- the usual case: this list was never built.  The merge kernel takes a partial list as a SET of candidates,
        // so the buffered candidates that reach the final bound go straight to the lane's partial list, unsorted.  A lane
        // with more than KMAX survivors (adversarial data): the sorted path below.
        probe.final_direct_begin();
        int n = 0;
#pragma unroll 1
        for (int base = 0; __builtin_amdgcn_ballot_w64(base < cnt[cg]) != 0; base += 16) {
          const float *ps = chunk_base(buf_s + (cg * CAND_CAP + base) * 64, 0);
          const int *pi = chunk_base(buf_i + (cg * CAND_CAP + base) * 64, 0);
          f32x16 vs;
          int ids[16];
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const bool in = base + e < cnt[cg];
            vs[e] = in ? ps[e * 64 + ulane] : -INFINITY;
            ids[e] = in ? pi[e * 64 + ulane] : INT_MAX;
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            if (vs[e] >= tf && ids[e] != INT_MAX) {
              if (n < KMAX) {
                a.part_scores[o + n] = vs[e];
                a.part_idx[o + n] = ids[e];
              }
              ++n;
            }
          }
        }
        probe.final_batch_end();
        if (__builtin_amdgcn_ballot_w64(n > KMAX) == 0) {
          a.part_cnt[ol] = n;  // (the merge takes the first n entries of this list: nothing is stored behind them)
          if (a.epi_stats) {
            const unsigned app = wave_sum_u32((unsigned)cnt[cg]);
            if (lane == 0) {
              atomicAdd(a.epi_stats, 64ull);
              atomicAdd(a.epi_stats + 1, (unsigned long long)app);
            }
          }
          continue;
        }
      }
      float best[KMAX];
      int bidx[KMAX];
      if ((built >> cg) & 1) {
#pragma unroll
        for (int q = 0; q < (KMAX + 15) / 16; ++q) {
          const float *ps = chunk_base(home_s + cg * KMAX * 64, q);
          const int *pi = chunk_base(home_i + cg * KMAX * 64, q);
#pragma unroll
          for (int j = 16 * q; j < KMAX && j < 16 * q + 16; ++j) {
            best[j] = ps[(j - 16 * q) * 64 + ulane];
            bidx[j] = pi[(j - 16 * q) * 64 + ulane];
          }
        }
      } else {  // (never built: the empty list + the buffered candidates below)
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
          best[j] = -INFINITY;
          bidx[j] = INT_MAX;
        }
      }
#pragma unroll 1
      for (int base = 0; __builtin_amdgcn_ballot_w64(base < cnt[cg]) != 0; base += 16) {
        const float *ps = chunk_base(buf_s + (cg * CAND_CAP + base) * 64, 0);  // 16 entries in flight, not one
        const int *pi = chunk_base(buf_i + (cg * CAND_CAP + base) * 64, 0);
        f32x16 vs;
        int ids[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const bool in = base + e < cnt[cg];
          vs[e] = in ? ps[e * 64 + ulane] : -INFINITY;
          ids[e] = in ? pi[e * 64 + ulane] : INT_MAX;
        }
        // which of a lane's 16 candidates may still enter its list: a bit mask per lane; then ONE loop in which every
        // lane inserts ITS next candidate (lowest bit = arrival order)
        unsigned pm = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e)
          pm |= (vs[e] >= tf && ranks_before(vs[e], ids[e], best[KMAX - 1], bidx[KMAX - 1])) ? (1u << e) : 0u;
        probe.final_batch_begin(pm);
#pragma unroll 1
        while (__builtin_amdgcn_ballot_w64(pm != 0) != 0) {
          probe.final_insert();
          if (pm != 0) {
            const int e = __builtin_ctz(pm);
            pm &= pm - 1;
            float v = vs[0];
            int id = ids[0];
#pragma unroll
            for (int q = 1; q < 16; ++q) {
              v = e == q ? vs[q] : v;
              id = e == q ? ids[q] : id;
            }
            if (ranks_before(v, id, best[KMAX - 1], bidx[KMAX - 1])) list_insert_lex<KMAX>(best, bidx, v, id);
          }
        }
        probe.final_batch_end();
      }
      if (a.epi_stats) {
        const unsigned app = wave_sum_u32((unsigned)cnt[cg]);
        if (lane == 0) {
          atomicAdd(a.epi_stats, 64ull);
          atomicAdd(a.epi_stats + 1, (unsigned long long)app);
        }
      }
      a.part_cnt[ol] = KMAX;  // (the sorted path writes the whole list, "no entry" tail included)
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        a.part_scores[o + j] = best[j];
        a.part_idx[o + j] = bidx[j];
      }
    }
  }
  probe.report(wv, lane);
}

template <int KMAX>
static hipError_t launch32_t(const MatchArgs &args, int grid, void *scratch, hipStream_t s) {
  // (the attribute belongs to the function ON A DEVICE: remembered per device, not per process)
  static unsigned long long attr_set = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (!((attr_set >> (dev & 63)) & 1ull)) {
    hipError_t e = hipFuncSetAttribute((const void *)match32_kernel<KMAX>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       Geo<4>::LDS + 32);
    if (e != hipSuccess) return e;
    attr_set |= 1ull << (dev & 63);
  }
  // scratch: scores of all lists, then their indices
  float *ls = (float *)scratch;
  int *li = (int *)(ls + scratch16_entries(grid, 4, KMAX));
  hipLaunchKernelGGL((match32_kernel<KMAX>), dim3(grid), dim3(256), Geo<4>::LDS + 32, s, args, ls, li);
  return hipGetLastError();
}

hipError_t launch_match32(const MatchArgs &g, int list_len, int grid, void *scratch, hipStream_t s) {
  switch (list_len) {
    case 1: return launch32_t<1>(g, grid, scratch, s);
    case 8: return launch32_t<8>(g, grid, scratch, s);
    case 20: return launch32_t<20>(g, grid, scratch, s);
    case 32: return launch32_t<32>(g, grid, scratch, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kpdi
