// decomp_plan.h - how decomp.hip lays the PCA decomposition of the resident patterns on the chip: pure functions of the
// pattern count M and the pixel count K = sy sx, no HIP call (tests/test_host_decomposition.py compiles this header with
// the host compiler and checks branch choice, tile counts, edges and the size limit).
//
// X is the M x K matrix of the patterns, row-major.  The Gram matrix is taken over the SHORTER side:
//   K <= M: Xc^T Xc, K x K (transposed = 0), the reduction runs down the M rows;
//   K >  M: Xc Xc^T, M x M (transposed = 1), the reduction runs along the K pixels.
// Every product of decomp.hip (Gram, apply, model) is one tile kernel: a workgroup of DEC_THREADS owns one DEC_TILE x
// DEC_TILE output tile and walks the WHOLE reduction in steps of DEC_KB, so an output's sum has one order whatever the
// launch looks like; tiles and steps that stick out are padded with zeros in LDS and their outputs are not stored.  A
// Gram launch is a square grid of tiles of which the upper triangle (tj >= ti) computes and stores both (i, j) and
// (j, i); on the diagonal tiles only j >= i is stored and mirrored, so the matrix is symmetric bit for bit.
//
// The size limit: side = min(M, K) <= DEC_MAX_SIDE.  side^2 doubles come back to the host (8192^2: 512 MiB) and go
// through a dense symmetric eigen-solve there (O(side^3), tens of seconds at 8192); beyond that the caller bins the
// patterns first (EBSD.downsample).
#pragma once
#include <cstddef>
#include <cstdint>

namespace kpdi {

constexpr int DEC_TILE = 64;        // outputs per tile side: 4 waves of 32 x 32, each 2 x 2 MFMAs of 16 x 16
constexpr int DEC_KB = 16;          // reduction steps staged in LDS at once: 4 MFMAs of depth 4 per 16 x 16 block
constexpr int DEC_THREADS = 256;
constexpr int DEC_LD = DEC_TILE + 16;  // doubles per LDS row: the 4 depth rows a wave reads at once start 128 B apart modulo 256 B
constexpr size_t DEC_LDS_BYTES = 2 * (size_t)DEC_KB * DEC_LD * sizeof(double);
constexpr int64_t DEC_MAX_SIDE = 8192;
constexpr int DEC_MEAN_ROWS = 256;  // "navigation" means: rows per partial sum (fixed: part of the summation order)
constexpr int DEC_CENTRE_NONE = 0, DEC_CENTRE_NAVIGATION = 1, DEC_CENTRE_SIGNAL = 2;

struct DecPlan {
  int ok;            // 0: refused (too_large tells why)
  int too_large;     // side > DEC_MAX_SIDE
  int transposed;    // 1: the M x M branch
  int64_t side;      // min(M, K)
  int64_t reduce;    // max(M, K): length of every sum
  int tiles;         // tiles per side of the Gram matrix
  int edge;          // outputs of the last tile per side (DEC_TILE when it is full)
  int64_t computed_tiles;  // tiles of the upper triangle, diagonal included
  int64_t steps;     // LDS stages per tile
  int tail;          // reduction steps of the last stage (DEC_KB when it is full)
};

inline int dec_tiles(int64_t n) { return (int)((n + DEC_TILE - 1) / DEC_TILE); }
inline int dec_edge(int64_t n) { return n % DEC_TILE ? (int)(n % DEC_TILE) : DEC_TILE; }
inline int64_t dec_steps(int64_t r) { return (r + DEC_KB - 1) / DEC_KB; }
inline int dec_tail(int64_t r) { return r % DEC_KB ? (int)(r % DEC_KB) : DEC_KB; }
// partial sums of the "navigation" means
inline int64_t dec_mean_chunks(int64_t m) { return (m + DEC_MEAN_ROWS - 1) / DEC_MEAN_ROWS; }

inline DecPlan dec_plan(int64_t m, int64_t k) {
  DecPlan p{};
  if (m < 1 || k < 1 || m >= ((int64_t)1 << 31) || k >= ((int64_t)1 << 30)) return p;
  p.transposed = k > m;
  p.side = p.transposed ? m : k;
  p.reduce = p.transposed ? k : m;
  if (p.side > DEC_MAX_SIDE) {
    p.too_large = 1;
    return p;
  }
  p.tiles = dec_tiles(p.side);
  p.edge = dec_edge(p.side);
  p.computed_tiles = (int64_t)p.tiles * (p.tiles + 1) / 2;
  p.steps = dec_steps(p.reduce);
  p.tail = dec_tail(p.reduce);
  p.ok = 1;
  return p;
}

}  // namespace kpdi
