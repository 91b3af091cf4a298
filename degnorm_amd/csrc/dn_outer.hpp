// dn_outer.hpp -- the kernels the C ABI (dn_api.hip) launches directly, behind one launcher per operation: the O(n p) outer
// DegNorm update and initial normalisation, the row maxima of an upload and the small gathers.  A launcher queues on `st` and
// returns; the caller checks hipGetLastError.  Which kernel instantiation a sample count p gets is decided in dn_outer.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dn {
namespace outer {

// The update runs one wave per gene in blocks_for(n) blocks of four waves; every block leaves one row of partial sums.  The
// block count is part of the results: it fixes the order in which the genes are added up (tests/_outer_restatement.py).
constexpr int BLOCK_CAP = 512;
constexpr size_t PART_DOUBLES = (size_t) BLOCK_CAP * (3 * 256 + 4);     // the block-partials buffer: the widest row x the cap
inline int blocks_for(int64_t n) { return (n + 3) / 4 < BLOCK_CAP ? (int) ((n + 3) / 4) : BLOCK_CAP; }

// block partials of n genes into part[PART_DOUBLES], then their sums in block order into out[0 .. 3p + 4)
void partials(hipStream_t st, const double *rho_raw, double *rho_c, const double *xw, const int32_t *trace, const int32_t *flags,
              double *part, double *out, int64_t n, int p);
void init_partials(hipStream_t st, const double *est, const double *cov, const int32_t *status, const double *x,
                   double *part, double *out, int64_t n, int p);
void apply(hipStream_t st, double *rho_c, double *xw, double *xadj, const int32_t *flags, uint8_t *ran, const double *avg_di,
           const double *norm, bool have_avg, int64_t n, int p, int iter, int n_iter);
void scale_reads(hipStream_t st, const double *x, const double *norm, double *xw, size_t np, int p);
void gather_rows(hipStream_t st, const double *rho_raw, const int32_t *flags, const int64_t *rows, double *out_rho,
                 int32_t *out_flags, int n_rows, int p);
void trace_head(hipStream_t st, const int32_t *trace, int32_t *head, size_t n_ints, int cols);
void row_max(hipStream_t st, const float *cov, const int64_t *goff, const int32_t *glen, float *rowmax, int32_t *x16,
             int64_t n, int p, int n_cus);

}  // namespace outer
}  // namespace dn
