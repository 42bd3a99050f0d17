// prep_plan.h - which preparation kernel of prep.hip takes a launch, and with what geometry: a pure function of the
// dtype, the pixel counts, the metric, the operand form, the mask's kind, the raw pointer's alignment, the number of rows
// and the KPDI_PREP_* switches.  No HIP call and no getenv: launch_prep reads the environment into PrepSwitches, calls
// prep_plan and switches on the result; tests/test_host_prep_cases.py compiles this header with the host compiler and
// checks that the case table of tests/_prep_cases.py reaches every kernel family.
//
//   span = columns a row's owner writes = max(k (+1: centred NDP), kpad; float16 form: 2 * kpad)
//   span <= 64 * WAVE_VALUES = 4096     one WAVE per pattern, four patterns per workgroup
//     no mask, k % 4 == 0, vector loads     PREP_WAVE4 (forms 0 / 1), PREP_WAVE_LINES (forms 2 / 3: whole lines via LDS)
//     mask, float32, run-structured         PREP_WAVE_GATHER (descriptors of gather_descriptors())
//     mask, float32, vector loads           PREP_WAVE_MASKED_DMA (row staged in LDS by LDS-DMA)
//     mask, vector loads, npix <= 4096      PREP_WAVE_MASKED (row staged in LDS)
//     otherwise                             PREP_WAVE1 (element-wise loads; pixel map read from global memory)
//   span <= PREP_THREADS * WAVE_VALUES = 16384   one WORKGROUP per pattern (or several patterns per workgroup)
//     form 3                                PREP32_BLOCK4 (four patterns per 1024 threads, whole lines)
//     form 2                                PREP16_BLOCK4 (NP = 2 or 4 patterns per workgroup; KPDI_PREP16=block: PREP_BLOCK*)
//     no mask, k % 4 == 0, vector loads     PREP_BLOCK
//     mask                                  PREP_BLOCK_MASKED
//   anything else                           PREP_GENERIC (re-reads the pattern from L2; any size)
// "vector loads" = npix % 4 == 0 and the raw pointer aligned to four elements (vec_ok).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/kpdi.h"

namespace kpdi {

constexpr int NORM_NDP_CENTRED = 2;  // internal value of the `metric` argument: `ndp` in its centred form (prep.hip)
constexpr int PREP_THREADS = 256;
constexpr int WAVE_VALUES = 64;  // values per lane of the wave-per-pattern kernels (K <= 4096)
constexpr int PREP16_THREADS = 1024;
constexpr size_t PREP_LDS_DEFAULT = 64 * 1024;  // more dynamic LDS than this has to be asked for (hipFuncSetAttribute)
constexpr size_t PREP_DMA_LDS_CAP = 160 * 1024;

inline size_t dtype_size(int dtype) {
  switch (dtype) {
    case KPDI_U8: case KPDI_I8: return 1;
    case KPDI_U16: case KPDI_I16: case KPDI_F16: return 2;
    case KPDI_F32: case KPDI_I32: case KPDI_U32: return 4;
    case KPDI_F64: return 8;
  }
  return 0;
}

// host: the signal mask's pixel map as one descriptor per 4 kept pixels for the gather kernels of prep.hip - the quad's
// pixels as (up to) two runs of consecutive detector pixels: bits 0-11 = detector pixel of element 0, bits 12-23 =
// detector pixel of element j MINUS j (so that element e >= j is the e-th float behind it), bits 24-26 = j (4: one run).
// Returns false when some quad needs more than two runs or npix > 4096 (descriptors unusable).
inline bool gather_descriptors(const int *pix_map, int k, int npix, std::vector<unsigned> *out) {
  out->clear();
  if (npix > 4096 || k <= 0) return false;
  for (int q = 0; 4 * q < k; ++q) {
    const int n = std::min(4, k - 4 * q);
    const int *p = pix_map + 4 * q;
    int j = n;  // first element that does not continue the run of element 0
    for (int e = 1; e < n; ++e)
      if (p[e] != p[0] + e) {
        j = e;
        break;
      }
    for (int e = j + 1; e < n; ++e)
      if (p[e] != p[j] + (e - j)) return false;  // a third run
    const int off2 = j < n ? p[j] - j : p[0];      // >= 0: pix_map ascends, so p[j] > p[j - 1] >= j - 1
    if (off2 < 0) return false;
    out->push_back((unsigned)p[0] | ((unsigned)off2 << 12) | ((unsigned)(j < n ? j : 4) << 24));
  }
  return true;
}

// the kernel template families of prep.hip
enum PrepKernel {
  PREP_NONE = -1,          // unknown dtype
  PREP_GENERIC = 0,        // prep_kernel<T>
  PREP_WAVE1,              // prep_wave_kernel<T, 1, H>
  PREP_WAVE4,              // prep_wave_kernel<T, 4, H>
  PREP_WAVE_LINES,         // prep_wave_lines_kernel<T>
  PREP_WAVE_MASKED,        // prep_wave_masked_kernel<T, H>
  PREP_WAVE_MASKED_DMA,    // prep_wave_masked_dma_kernel<H>
  PREP_WAVE_GATHER,        // prep_wave_gather_kernel<LINES>
  PREP_BLOCK,              // prep_block_kernel<T, false, H>
  PREP_BLOCK_MASKED,       // prep_block_kernel<T, true, H>
  PREP32_BLOCK4,           // prep32_block4_kernel<T, MASKED>
  PREP16_BLOCK4,           // prep16_block4_kernel<T, MASKED, NP>
  PREP_KERNEL_FAMILIES
};

// the environment switches of launch_prep
struct PrepSwitches {
  bool no_staged = false;  // KPDI_PREP_NO_STAGED
  bool no_lines = false;   // KPDI_PREP_NO_LINES
  bool no_dma = false;     // KPDI_PREP_NO_DMA
  bool no_gather = false;  // KPDI_PREP_NO_GATHER
  int prep16 = 0;          // KPDI_PREP16: 0 unset (two patterns per workgroup), 1 "block" (prep_block_kernel), 2 "block4"
};

struct PrepPlan {
  int kernel;         // PrepKernel
  bool h16;           // template flag H: the plane-major forms (2: float16, 3: wide float32)
  bool masked;        // template flag MASKED of the block4 kernels
  bool lines;         // template flag LINES of the gather kernel
  int np;             // PREP16_BLOCK4: patterns per workgroup
  bool pass_form;     // the kernel is told the operand form (else 0: plain float32 rows)
  unsigned grid, threads;
  size_t lds_bytes;   // dynamic LDS; above PREP_LDS_DEFAULT the launcher raises the kernel's limit first
  bool split_after;   // form 1: launch_split_f16 converts the rows in place afterwards
  // the decisions behind it
  int span;
  bool wave_path, block_path, vec_ok, vec4, staged, staged_dma, gather, block_vec, block_masked;
};

// `raw_addr`: the raw pointer as an integer (only its remainders modulo 4 and modulo four elements matter)
inline PrepPlan prep_plan(int dtype, int npix, int k, int kpad, int metric, int operand_form, bool have_pix_map,
                          bool have_quad_desc, uint64_t raw_addr, int n_out, const PrepSwitches &sw) {
  PrepPlan p{};
  p.kernel = PREP_NONE;
  const size_t es = dtype_size(dtype);
  if (!es) return p;
  const int cols = k + (metric == NORM_NDP_CENTRED ? 1 : 0);  // columns of a row that are not padding
  // columns a row-owning wave / workgroup has to write: everything up to the padded row length
  p.span = std::max(cols, operand_form == 2 ? 2 * kpad : kpad);
  p.wave_path = p.span <= 64 * WAVE_VALUES;
  p.vec_ok = (npix % 4) == 0 && (raw_addr % (4 * es)) == 0;
  p.vec4 = p.wave_path && !have_pix_map && (k % 4) == 0 && p.vec_ok;
  p.staged = p.wave_path && have_pix_map && p.vec_ok && npix <= 64 * WAVE_VALUES && !sw.no_staged;
  // larger detectors, still register-resident: one workgroup per pattern
  p.block_path = !p.wave_path && p.span <= PREP_THREADS * WAVE_VALUES;
  p.block_vec = p.block_path && !have_pix_map && (k % 4) == 0 && p.vec_ok;
  p.block_masked = p.block_path && have_pix_map;
  const size_t staged_lds = (size_t)(((k + 3) & ~3) + 4 * npix) * 4;
  const size_t lines_lds = (size_t)4 * kpad * 4 * (sw.no_lines ? 1000 : 1);  // prep_wave_lines_kernel
  // float32 rows (dictionaries): LDS-DMA, double-buffered (prep_wave_masked_dma_kernel)
  const size_t dma_lds = (size_t)(((k + 3) & ~3) + 8 * ((npix + 255) & ~255)) * 4;
  p.staged_dma = p.staged && dtype == KPDI_F32 && dma_lds <= PREP_DMA_LDS_CAP && !sw.no_dma;
  // float32 rows whose mask is a set of runs: gathered straight from global memory (prep_wave_gather_kernel); the
  // plane-major forms (2: float16, 3: wide float32) are written as whole lines through LDS, forms 0 / 1 as 16-byte slots
  p.gather = p.wave_path && have_pix_map && have_quad_desc && dtype == KPDI_F32 && (raw_addr % 4) == 0 &&
             (operand_form < 2 || lines_lds <= PREP_LDS_DEFAULT) && !sw.no_gather;
  p.h16 = operand_form >= 2;
  p.pass_form = true;
  p.threads = PREP_THREADS;
  const unsigned quads = (unsigned)((n_out + 3) / 4);
  p.grid = p.wave_path ? quads : (unsigned)n_out;
  if (p.staged && !p.gather) p.grid = std::min(quads, 2048u);
  const bool block_any = p.block_vec || p.block_masked;
  if (p.gather) {
    p.kernel = PREP_WAVE_GATHER;
    p.lines = operand_form >= 2;
    p.lds_bytes = p.lines ? lines_lds : 0;
  } else if (operand_form == 3 && block_any) {
    p.kernel = PREP32_BLOCK4;
    p.masked = p.block_masked;
    p.grid = quads;
    p.threads = PREP16_THREADS;
    p.lds_bytes = (size_t)4 * (8 * ((kpad / 8 + 1) / 2) + 4) * 4;
  } else if (operand_form == 2 && block_any && sw.prep16 != 1) {
    p.kernel = PREP16_BLOCK4;
    p.masked = p.block_masked;
    p.np = sw.prep16 == 2 ? 4 : 2;
    // NP = 2: the affine mapping walks row groups of 4 in blocks of 16 units
    p.grid = p.np == 2 ? (unsigned)(((n_out + 1) / 2 + 15) / 16 * 16) : quads;
    p.threads = 256u * p.np;
    p.lds_bytes = (size_t)p.np * (2 * kpad + 8) * 2;
  } else if (p.h16 && p.vec4 && lines_lds <= PREP_LDS_DEFAULT) {
    p.kernel = PREP_WAVE_LINES;
    p.lds_bytes = lines_lds;
  } else if (p.vec4) {
    p.kernel = PREP_WAVE4;
  } else if (p.staged_dma) {
    p.kernel = PREP_WAVE_MASKED_DMA;
    p.grid = std::min(quads, 1024u);
    p.lds_bytes = dma_lds;
  } else if (p.staged) {
    p.kernel = PREP_WAVE_MASKED;
    p.lds_bytes = staged_lds;
  } else if (p.wave_path) {
    p.kernel = PREP_WAVE1;
    p.pass_form = p.h16;
  } else if (block_any) {
    p.kernel = p.block_vec ? PREP_BLOCK : PREP_BLOCK_MASKED;
    if (p.h16) p.grid = (unsigned)(((int64_t)n_out + 31) / 32 * 32);
  } else {
    p.kernel = PREP_GENERIC;
    p.pass_form = p.h16;
  }
  // paths that store whole float4 slots write the split-f16 form themselves; the others are converted in place
  // afterwards (rows beyond n_out are zero in either form).  The float16 form is written directly by every path.
  p.split_after = operand_form == 1 && !(p.vec4 || p.staged || p.gather || block_any);
  return p;
}

}  // namespace kpdi
