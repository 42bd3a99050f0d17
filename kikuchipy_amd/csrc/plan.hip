// plan.hip - kpdi_plan_describe (include/kpdi.h): the plan::SweepPlan that sweep.hip would launch for a sweep, as plain
// data.  It builds the engine's request (plan.h: chunk_request; for keep_n > 32 the first pass of it) and copies what
// plan::sweep_plan answers - no planning of its own; the fields of the kernel form that is not in use read 0.  Host
// arithmetic only: callable without a GPU (tests/test_planner.py).
#include "../../include/kpdi.h"
#include "group_hooks.h"
#include "plan.h"

extern "C" int kpdi_plan_describe(int64_t m, int64_t n_chunk, int k_kept, int keep_n, int n_cu, int form, kpdi_plan *out) {
  using namespace kpdi;
  if (!out) return fail_msg(KPDI_EINVAL, "out is NULL");
  if (m < 1 || n_chunk < 1 || k_kept < 1 || keep_n < 1 || n_cu < 1 || m >= (1ll << 31) - TILE_EXP || n_chunk >= (1ll << 31) - F16_TILE)
    return fail_msg(KPDI_EINVAL, "kpdi_plan_describe: sizes must be positive (and fit 32 bits)");
  if (form != -1 && form != 0 && form != 3) return fail_msg(KPDI_EINVAL, "form must be -1 (automatic), 0 (match.hip) or 3 (match16.hip, f32)");
  plan::Env e;
  e.n_cu = n_cu;
  e.blocks_per_cu = match_blocks_per_cu();
  e.sw.read();
  const int row_blocks = round_up(m, TILE_EXP) / TILE_EXP;
  const bool wide = form < 0 ? plan::prefer_wide(e, row_blocks, k_kept, n_chunk) : form == 3;
  plan::SweepPlan p = plan::sweep_plan(e, plan::chunk_request(wide ? 3 : 0, wide ? F16_TILE : TILE_DICT, row_blocks, n_chunk, keep_n, false));
  if (!p.req.allow_tail) p = p.pass(match_list_len((int)std::min<int64_t>(KMAX_LIMIT, n_chunk)), false);  // (sweep.hip: the first local_pass)
  *out = kpdi_plan{};
  out->form = p.req.form;
  out->tile = p.req.tile;
  out->row_blocks = row_blocks;
  out->n_tiles = p.n_tiles;
  out->nsplit = p.nsplit;
  out->rows_per_launch = p.rows_per_launch;
  out->launches = p.launches;
  out->round_rows = plan::round_rows(e, row_blocks);
  out->n_main = p.n_main;
  if (!wide) {
    out->tail_tiles = p.tail_tiles;
    out->tail_units = p.tail_units;
    out->tail_nsplit = p.tail_nsplit;
    out->fixed_draws = p.fixed_draws;
  } else {
    out->tail_first = p.tail_first;
    out->tail_shift = p.tail_shift;
    out->tail_gemm_rows = p.gemm_rows;
    out->perm_rounds = p.perm_rounds;
    out->perm_stride = p.perm_stride;
  }
  out->n_launch_desc = std::min(p.launches, KPDI_PLAN_MAX_LAUNCHES);  // (`launches` says how many there are)
  for (int j = 0; j < out->n_launch_desc; ++j) {
    const plan::Launch l = p.launch(j);
    out->launch[j].row_first = l.row_first;
    out->launch[j].rows = l.rows;
    out->launch[j].xcd_rows = l.xcd_rows;
    out->launch[j].xcd_splits = l.xcd_splits;
    out->launch[j].rows_grid = l.rows_grid;
  }
  return KPDI_OK;
}
