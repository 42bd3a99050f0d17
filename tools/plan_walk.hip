// plan_walk.hip - plan::sweep_plan (csrc/plan.h) under the host sanitizers: a stand-alone program that plans every request
// of a grid (map sizes x chunk sizes x the four operand forms x tails allowed / bounded x list lengths x three chips),
// walks the launches of every plan and checks that they cover the row blocks exactly once.  Host arithmetic only - it
// opens no GPU and nothing of it is loaded into Python:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -Ikikuchipy_amd/csrc tools/plan_walk.hip -o build/plan_walk && build/plan_walk
#include <cstdio>

#include "plan.h"

using namespace kpdi;

int main() {
  const int ms[] = {1, 9, 255, 256, 257, 512, 1024, 4096, 7424, 10000, 40000, 300000};
  const int list_lens[] = {1, 8, 20, 32};
  long plans = 0, launches = 0;
  for (int n_cu : {8, 104, 256}) {
    plan::Env e;
    e.n_cu = n_cu;
    for (int m : ms) {
      const int row_blocks = (m + TILE_EXP - 1) / TILE_EXP;
      // every chunk size up to four tiles, then steps that are no multiple of a tile, up to 300 000
      for (int64_t n = 1; n <= 300000; n += n < 1024 ? 1 : 1021) {
        for (int form = 0; form < 4; ++form)
          for (int flags = 0; flags < 4; ++flags) {
            plan::SweepRequest r;
            r.form = form;
            r.tile = form >= 2 ? F16_TILE : TILE_DICT;
            r.row_blocks = row_blocks;
            r.n_chunk = n;
            r.list_len = list_lens[(n + flags) % 4];
            r.allow_tail = flags & 1;
            r.bounded = flags & 2;
            const plan::SweepPlan p = plan::sweep_plan(e, r);
            int next = 0, grid = 0;
            for (int j = 0; j < p.launches; ++j) {
              const plan::Launch l = p.launch(j);
              if (l.row_first != next || l.rows < 1 || l.rows_grid < l.rows) return printf("launch %d of m %d n %lld form %d\n", j, m, (long long)n, form), 1;
              next += l.rows;
              grid = std::max(grid, l.rows_grid);
              ++launches;
            }
            const bool tails_ok = p.n_main >= 1 && p.n_main + p.tail_tiles + (p.gemm_rows > 0 ? p.n_tiles - p.n_main : 0) == p.n_tiles;
            if (next != row_blocks || grid != p.grid_rows || !tails_ok || !(p == plan::sweep_plan(e, r)) || !(p.pass(r.list_len, r.bounded) == p))
              return printf("plan of m %d n %lld form %d flags %d\n", m, (long long)n, form, flags), 1;
            ++plans;
          }
      }
    }
  }
  printf("plan_walk: %ld plans, %ld launches walked\n", plans, launches);
  return 0;
}
