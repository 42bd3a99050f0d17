// merge_plan.h - which kernel of merge.hip takes a merge: a pure function of the number of candidates per pattern (all
// sources laid end to end, real or not).  No HIP call: launch_merge calls merge_plan and switches on the result;
// tests/test_host_merge_cases.py compiles this header with the host compiler, checks the boundaries and that the case
// table of tests/_merge_cases.py reaches every fork behind them.
//
//   candidates <= 64 * NK, NK = 4 | 12 | 24 | 48    MERGE_CACHED: one WAVE per pattern, four patterns per workgroup, NK
//                                                   keys per lane in registers; the real ones are packed into LDS when
//                                                   at most 64 * min(NK, 8) are (merge_packed_capacity)
//   candidates <= 256 * NK, NK = 24 | 64            MERGE_BLOCK: one WORKGROUP per pattern, NK keys per thread
//   more                                            MERGE_GENERIC: re-reads every candidate from L2 in every round
#pragma once

#if defined(__HIPCC__)
#define KPDI_PLAN_HD __host__ __device__ __forceinline__
#else
#define KPDI_PLAN_HD inline
#endif

namespace kpdi {

enum MergeFamily { MERGE_CACHED = 0, MERGE_BLOCK = 1, MERGE_GENERIC = 2 };

// the seven kernels, in the order of their capacity; MERGE_PLAN_AUTO = let the candidate count choose
enum MergePlanId {
  MERGE_PLAN_AUTO = -1,
  MERGE_PLAN_CACHED4 = 0,
  MERGE_PLAN_CACHED12,
  MERGE_PLAN_CACHED24,
  MERGE_PLAN_CACHED48,
  MERGE_PLAN_BLOCK24,
  MERGE_PLAN_BLOCK64,
  MERGE_PLAN_GENERIC,
  MERGE_PLANS
};

constexpr int MERGE_WAVE = 64;        // candidates per register slot of a wave-per-pattern kernel
constexpr int MERGE_BLOCK_THREADS = 256;
constexpr int MERGE_PACK_SLOTS = 8;   // packed keys per lane (CK = min(NK, MERGE_PACK_SLOTS))
constexpr int MERGE_UNBOUNDED = 0x7fffffff;

struct MergePlan {
  int id;        // MergePlanId
  int family;    // MergeFamily
  int nk;        // keys per lane (cached) / per thread (block); 0: generic
  int capacity;  // candidates the kernel holds
};

inline MergePlan merge_plan_of(int id) {
  switch (id) {
    case MERGE_PLAN_CACHED4: return {id, MERGE_CACHED, 4, 4 * MERGE_WAVE};
    case MERGE_PLAN_CACHED12: return {id, MERGE_CACHED, 12, 12 * MERGE_WAVE};
    case MERGE_PLAN_CACHED24: return {id, MERGE_CACHED, 24, 24 * MERGE_WAVE};
    case MERGE_PLAN_CACHED48: return {id, MERGE_CACHED, 48, 48 * MERGE_WAVE};
    case MERGE_PLAN_BLOCK24: return {id, MERGE_BLOCK, 24, 24 * MERGE_BLOCK_THREADS};
    case MERGE_PLAN_BLOCK64: return {id, MERGE_BLOCK, 64, 64 * MERGE_BLOCK_THREADS};
    case MERGE_PLAN_GENERIC: return {id, MERGE_GENERIC, 0, MERGE_UNBOUNDED};
  }
  return {MERGE_PLAN_AUTO, -1, 0, -1};
}

// the smallest kernel that holds `candidates`
inline MergePlan merge_plan(int candidates) {
  for (int id = MERGE_PLAN_CACHED4; id < MERGE_PLAN_GENERIC; ++id)
    if (candidates <= merge_plan_of(id).capacity) return merge_plan_of(id);
  return merge_plan_of(MERGE_PLAN_GENERIC);
}

// real candidates a wave-per-pattern kernel packs into LDS; with more, its rounds run over the registers
inline int merge_packed_capacity(int nk) { return MERGE_WAVE * (nk < MERGE_PACK_SLOTS ? nk : MERGE_PACK_SLOTS); }

// local / len without an integer division: the float quotient of local + 0.5 lies at least 1 / (2 len) away from an
// integer and float holds it to 2^-24 of its value, (local / len) 2^-24 < 1 / (2 len) for local < 2^23 - exact for
// every local < 16384 and len <= 1024 (tests/test_host_merge_cases.py tries them all)
KPDI_PLAN_HD int merge_list_index(int local, int len) { return (int)(((float)local + 0.5f) / (float)len); }

}  // namespace kpdi
