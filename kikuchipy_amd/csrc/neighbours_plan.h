// neighbours_plan.h - how neighbours.hip lays the two map-wide ops (neighbour pattern averaging, neighbour dot products)
// on the chip: pure functions of the detector shape, no HIP call.
//
// One workgroup of NB_THREADS lanes per map point.  A lane owns the items tid, tid + NB_THREADS, ... of the pattern, an
// item being 4 consecutive pixels when the pattern size is a multiple of 4 (every pattern then starts on a 4-element
// boundary and is read with vector loads) and one pixel otherwise.  Up to NB_KEEP values per lane stay in registers
// between the two halves of an op (the correlated values until the pattern's min / max are known; the centred centre
// pattern while the neighbours stream by); larger patterns are read again instead - mostly from L1 / L2.
#pragma once
#include "pattern_plan.h"

namespace kpdi {

constexpr int NB_THREADS = 256;
constexpr int NB_KEEP = 16;              // values a lane keeps in registers
constexpr int NB_MAX_WINDOW = 1 << 20;  // coefficients of a window

// one window coefficient in use: its offset from the window's origin, its flat index in the window, its weight
struct NbTap {
  double w;
  int dy, dx, j, pad;
};

struct NbPlan {
  int vec;    // pixels per item: 4 or 1
  int nitem;  // items per pattern
  int keep;   // 1: the per-lane values stay in registers
};

PLAN_HD inline NbPlan nb_plan(int sy, int sx) {
  NbPlan p;
  const int npix = sy * sx;
  p.vec = npix % 4 == 0 ? 4 : 1;
  p.nitem = npix / p.vec;
  p.keep = p.nitem <= NB_THREADS * (NB_KEEP / p.vec) ? 1 : 0;
  return p;
}

}  // namespace kpdi
