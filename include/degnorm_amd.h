/*
 * degnorm_amd.h -- C ABI of the MI355X-native NMF over-approximation core of DegNorm.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json:
 * the reference is pure Python, so "the reference's FFI for this path" is the set of calls its
 * GeneNMFOA.run() / run_gene_nmfoa_mpi() bodies make per gene; each entry point below names the
 * reference lines (relative to the DegNorm checkout, v0.1.4) it replaces.  The only caller is
 * degnorm_amd/_lib.py (ctypes); INTEGRATION.md shows the binding a DegNorm maintainer would add.
 *
 * Conventions
 *   - plain C types only; the caller allocates every host output; nothing throws across the boundary.
 *   - every function returns DN_OK (0) or a negative DN_E_* code; dn_last_error() gives the text.  The library keeps ONE
 *     text per thread: dn_assemble_last_error(), dn_reads_last_error() and dn_gtf_last_error() return the same string and
 *     stay for the callers that name their family.  A call's text is valid until the thread's next call that fails or
 *     (the reads, BAM and inflate entry points) clears it on entry.
 *   - per-gene problems the reference would raise on (ArpackError, empty np.min, svds ValueError:
 *     SURVEY H8) are reported in the per-gene trace status instead of aborting the batch.
 *   - a handle owns one HIP device, one stream, the resident coverage and all scratch; it is not
 *     thread-safe (the reference is called once from the main thread, nmf.py:483).
 *   - genes keep the caller's order on the boundary; the library permutes internally
 *     (longest-first work queue) and un-permutes on output.
 */
#ifndef DEGNORM_AMD_H
#define DEGNORM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DN_OK                 0
#define DN_E_INVALID         -1   /* bad argument / shape (reference: ValueError, nmf.py:469-481)            */
#define DN_E_HIP             -2   /* HIP runtime error (text in dn_last_error)                               */
#define DN_E_STATE           -3   /* call out of order (e.g. iterate before upload)                          */
#define DN_E_UNSUPPORTED     -4   /* p outside the compiled range                                            */
#define DN_E_NO_DEVICE       -5   /* no usable gfx950 device                                                 */

#define DN_TRACE_LEN          48  /* int32 per gene; layout mirrors oracle/nmfoa_oracle.c                    */
/* trace[0] n_hi_cov  [1] #nmf() calls  [2] sum of active columns over calls  [3] exit code
 * [4] loop-exit reason  [5] #dropped bins  [6] status (0 ok; -1 ArpackError, -2 empty min, -3 ValueError,
 *     -4 an eigen-solve left through its step cap: ARPACK's ArpackNoConvergence; the gene's DI row is zeroed like
 *     the other failures, never filled from an unconverged vector)
 * [7] total power-iteration steps of the on-chip eigen-solver  [8..40) drop_idx sequence                    */

typedef struct dn_handle_s *dn_handle;

/* Algorithm parameters of one outer iteration: GeneNMFOA.__init__ (nmf.py:12-53) after its own
 * normalisation (abs/int, min_high_coverage = max(2,.), forced to 2 when downsample_rate > 1). */
typedef struct {
    int32_t nmf_iter;                /* nmf.py:31  T, inner NMF-OA iterations per nmf() call               */
    int32_t bins;                    /* nmf.py:33  B                                                        */
    int32_t min_high_coverage;       /* nmf.py:34,52-53                                                     */
    int32_t downsample_rate;         /* nmf.py:36  take-every rate, 1 = none                                */
    int32_t skip_baseline_selection; /* nmf.py:48                                                           */
    int32_t want_estimates;          /* keep what dn_fetch_estimates needs (last outer iteration, nmf.py:601) */
    int32_t reserved[2];
} dn_params;

/* Library / device ------------------------------------------------------------------------------- */
const char *dn_version(void);
const char *dn_last_error(void);
int  dn_device_count(void);
int  dn_p_supported(int p);                         /* 1 if kernels for p samples are compiled in: the count-path
                                                       families of 2 .. 64 samples (0 from 65 on, see dn_p_max) */
int  dn_p_max(void);                                /* 256: the widest cohort dn_upload_* takes.  65 .. dn_p_max()
                                                       samples run on the wide-cohort kernel family             */

int  dn_create(int device, dn_handle *out);
int  dn_destroy(dn_handle h);

/* Upload --------------------------------------------------------------------------------------------
 * Replaces: cov_mats = list(cov_dat.values()) held as float64 host arrays (nmf.py:499) and the
 * per-iteration re-scaled copies adjust_coverage_curves makes (nmf.py:142-146, nmf_mpi.py:745-760).
 * Coverage is packed once into HBM as float32 (sample-major p x L_g per gene, genes back to back) and
 * stays resident; scaling by 1/s_i is folded into the kernels' loads.
 *
 * dn_upload_ragged: genes[g] points at a C-contiguous p x lengths[g] matrix of float64 (is_f32 = 0)
 * or float32 (is_f32 = 1).  *inexact (nullable) receives the number of values that are not exactly
 * representable in float32 (DegNorm coverage is integer counts, reads.py:714,773, so normally 0).
 * dn_upload_packed: the same data already packed (offsets in elements, offsets[n] = total).
 * Both accept 2 <= p <= dn_p_max(); beyond that DN_E_UNSUPPORTED.  The float64 per-gene path (dn_nmf_f64,
 * dn_baseline_selection_f64) stays at 2 <= p <= 64.                                                   */
/* Optional, before an upload: the take-every rate the following dn_baseline_iteration calls will use (GeneNMFOA's
 * downsample_rate, nmf.py:36).  Only steers which kernel family serves the data (results do not depend on it): when no
 * gene can keep more than 12 active columns, the row-wise one-wave-per-gene kernels are chosen from p = 8 on.          */
int  dn_set_downsample_hint(dn_handle h, int32_t rate);
/* Step cap of one on-chip eigen-solve in power-step equivalents (default 4000; the reference's ARPACK call has
 * maxiter = 10 n, scipy eigsh via svds, nmf.py:63).  A gene whose solve hits the cap gets status -4.                    */
int  dn_set_solver_step_cap(dn_handle h, int32_t max_steps);
/* Leading columns of the per-gene trace that dn_baseline_iteration copies back (8 .. DN_TRACE_LEN, default all): the
 * counters [0..8) are what a production run reads; the dropped-bin sequence [8..40) is diagnostics (at 50 000 genes the whole
 * trace is 9.6 MB per iteration).  `trace` of dn_baseline_iteration then holds n x cols int32.                            */
int  dn_set_trace_columns(dn_handle h, int32_t cols);
int  dn_upload_ragged(dn_handle h, int64_t n_genes, int32_t p, const void *const *genes,
                      const int64_t *lengths, int32_t is_f32, int32_t n_threads, int64_t *inexact);
int  dn_upload_packed(dn_handle h, int64_t n_genes, int32_t p, const float *packed,
                      const int64_t *lengths);

/* Initialisation pass -------------------------------------------------------------------------------
 * Replaces: par_apply(run_ratio_svd_serial) + est_sums / cov_sums (nmf.py:522-525; nmf_mpi.py:681-703).
 * est_sums[g*p+i] = sum_j max(K_i E_j, x_ij), cov_sums[g*p+i] = sum_j x_ij on the raw coverage.
 * status[g] (nullable): 0 or the per-gene error code (a gene of fewer than 2 columns: the reference's
 * ValueError; for p >= 17 also a gene of more than 2^24 columns -- its rows are addressed by 32-bit offsets).      */
int  dn_ratio_svd_sums(dn_handle h, double *est_sums, double *cov_sums, int32_t *status);

/* One outer DegNorm iteration over all resident genes ------------------------------------------------
 * Replaces: adjust_coverage_curves + par_apply_baseline_selection's per-gene work
 * (nmf.py:563-566 -> :142-146, :189-372; nmf_mpi.py:745-785), without the rho clip (host, nmf.py:398-399).
 * scale[p]: current scale factors.  ds_start (nullable unless downsample_rate > 1): per-gene
 * systematic-sample start offset in [0, rate) (nmf.py:422).
 * rho[n*p] (unclipped), flags[n] (ran_baseline_selection) -- both NULL: kept on the device for the dn_outer_* calls;
 * trace[n*DN_TRACE_LEN] (nullable).                                                                  */
int  dn_baseline_iteration(dn_handle h, const double *scale, const dn_params *prm, const int64_t *ds_start,
                           double *rho, int32_t *flags, int32_t *trace);

/* The outer DegNorm update on the device ---------------------------------------------------------------
 * Replaces: the O(n p) host arithmetic between two baseline-selection sweeps -- the DI clip (nmf.py:398-399),
 * correct_di_scores (:148-158), x_adj (:575, :581), the normalisation of the weighted counts (:584-587) and the
 * ran_baseline_selection column (:403); nmf_mpi.py:821-838 on rank 0.  With it dn_baseline_iteration may be called with
 * rho = flags = NULL: the n x p DI matrix stays in HBM and the host sees 3p + 4 numbers per iteration.
 *   dn_outer_begin     x_weighted (n x p, after the initial normalisation, nmf.py:534) -> device; degnorm_iter columns of flags
 *   dn_outer_partials  after dn_baseline_iteration: partials[0:p] = sum over touched genes of x_w / (1 - rho),
 *                      [p:2p] = sum over untouched genes (rho.max() == 0) of x_w, [2p:3p] = sum of x_w,
 *                      [3p] = #untouched, [3p+1] = #genes with trace status != 0, [3p+2] = #genes with status -4,
 *                      [3p+3] = #genes sent through baseline selection (ran_baseline_selection[:, iter].sum(), nmf.py:571)
 *                      -- 3p + 4 doubles
 *                      (sums in a fixed order; the caller all-reduces them over the GPUs)
 *   dn_outer_apply     rho[untouched] = avg_di (NULL: none untouched); x_adj = x_w / (1 - rho); x_w /= norm; flags -> column iter
 *   dn_fetch_outer     final rho / x_adj / x_weighted (n x p each) and ran_baseline_selection (n x degnorm_iter bytes); any may be NULL
 *   dn_fetch_rows      raw (unclipped) DI rows and flags of a few genes of the last dn_baseline_iteration (diagnostics)          */
int  dn_outer_begin(dn_handle h, const double *x_weighted, int32_t degnorm_iter);
/* The initial normalisation on the device -------------------------------------------------------------
 * Replaces: rho0 = 1 - cov_sums / (est_sums + 1), the `low` genes (rho0.max() < 0.1) and the per-sample sums of their read
 * counts, nmf.py:524-531 (nmf_mpi.py:681-718 on rank 0) -- O(n p) host arithmetic on two n x p matrices that
 * dn_ratio_svd_sums would otherwise have to copy back -- and x_weighted = x / norm (:533).
 *   dn_init_begin          reads (n x p float64 read counts) -> device, once per upload
 *   dn_ratio_svd_sums      may then be called with est_sums = cov_sums = NULL (the sums stay in HBM)
 *   dn_init_partials       partials[0:p] = sum over the low genes of x, [p:2p] = sum over all genes of x, [3p] = #low genes,
 *                          [3p+1] = #genes whose initial SVD failed ([2p:3p], [3p+2], [3p+3] unused; 3p + 4 doubles); fixed order, for the all-reduce
 *   dn_outer_begin_scaled  dn_outer_begin with x_weighted = reads / norm formed on the device                        */
int  dn_init_begin(dn_handle h, const double *reads);
int  dn_init_partials(dn_handle h, double *partials);
int  dn_outer_begin_scaled(dn_handle h, const double *norm, int32_t degnorm_iter);
int  dn_outer_partials(dn_handle h, double *partials);
/* The same sums left ON THE DEVICE for a device-side collective (RCCL all-reduce over xGMI on the buffer itself, no host
 * hop; nmf_mpi.py:796-838 moves the whole DI matrix through rank 0 instead): *d_partials receives the device address of the
 * 3p + 4 doubles, valid until the next dn_outer_* call on this handle; the library's stream has been synchronised.          */
int  dn_outer_partials_device(dn_handle h, double **d_partials);
int  dn_outer_apply(dn_handle h, const double *avg_di, const double *norm, int32_t iter);
int  dn_fetch_outer(dn_handle h, double *rho, double *x_adj, double *x_weighted, uint8_t *ran);

/* The collective of the sharded run, inside the library ----------------------------------------------------
 * Replaces: the per-iteration traffic of run_gene_nmfoa_mpi -- rank 0 re-scales and re-sends every coverage chunk
 * (nmf_mpi.py:745-760), every worker returns its estimates and DI rows (:796-815) and rank 0 alone updates the scale
 * factors (:821-838).  Here every GPU keeps its genes, and ONE all-reduce of 3p + 4 float64 per outer iteration (RCCL
 * over xGMI, in place on the library's device buffer, on the library's stream) gives every rank what it needs to
 * compute the new scale factors itself.  A host written in any language shards a run with these calls alone:
 *   dn_comm_unique_id   rank 0: DN_COMM_ID_BYTES opaque bytes (ncclGetUniqueId); the host hands them to every rank by
 *                       whatever it has (MPI_Bcast, a file, a socket)
 *   dn_comm_create      every rank, collectively: joins the communicator with the handle's GPU (ncclCommInitRank)
 *   dn_init_allreduce   dn_init_partials summed over the ranks: totals[3p + 4], same layout
 *   dn_outer_allreduce  dn_outer_partials summed over the ranks: totals[3p + 4], same layout; dn_outer_apply follows
 *   dn_comm_allreduce   sums a small host vector (<= DN_COMM_MAX_DOUBLES: the 3p + 4 sums of the widest cohort) over the
 *                       ranks in place: a rank WITHOUT genes joins the
 *                       two collectives above with zeros through this call (same count 3p + 4), error counts, ...
 *   dn_comm_library     which librccl was bound ("" if none could be loaded).  RCCL is resolved at run time (a copy the
 *                       process already holds, e.g. PyTorch's, else DN_RCCL_PATH, else the system's): no link-time dependency. */
#define DN_COMM_ID_BYTES 128
#define DN_COMM_MAX_DOUBLES (3 * 256 + 4)
int  dn_comm_unique_id(uint8_t *id);
int  dn_comm_create(dn_handle h, const uint8_t *id, int32_t rank, int32_t size);
int  dn_comm_destroy(dn_handle h);
int32_t dn_comm_size(dn_handle h);
const char *dn_comm_library(void);
int  dn_comm_allreduce(dn_handle h, double *buf, int32_t count);
int  dn_init_allreduce(dn_handle h, double *totals);
int  dn_outer_allreduce(dn_handle h, double *totals);
int  dn_fetch_rows(dn_handle h, int64_t n_rows, const int64_t *rows, double *rho_raw, int32_t *flags);

/* TEST-ONLY seam -- not part of the product's path, no caller under degnorm_amd/ besides the ctypes binding ---------------
 * The O(n p) kernels around the NMF pass read state that only kernels write (the raw DI rows, the flags and the per-gene
 * status of dn_baseline_iteration; the two sums and the status of dn_ratio_svd_sums) and write two arrays that no entry point
 * returns (the row maxima and the 16-bit flag of an upload).  The suite plants the former and reads the latter to compare
 * each of those kernels with a restatement of its own operation on inputs that no data set produces.
 *   dn_debug_plant   overwrites one device array of an uploaded handle from host memory (copies on the handle's stream,
 *                    no kernel); src holds the WHOLE array:
 *                      DN_PLANT_RHO_RAW      n x p doubles   the unclipped DI rows
 *                      DN_PLANT_FLAGS        n int32         ran_baseline_selection of the last iteration
 *                      DN_PLANT_ITER_STATUS  n int32         column 6 of the per-gene counters (status of the last iteration)
 *                      DN_PLANT_EST_SUMS     n x p doubles   est_sums of the initial pass
 *                      DN_PLANT_COV_SUMS     n x p doubles   cov_sums of the initial pass
 *                      DN_PLANT_INIT_STATUS  n int32         status of the initial pass
 *   dn_debug_peek    copies out DN_PEEK_ROWMAX (n x p floats, max_j x_ij of the uploaded coverage) or DN_PEEK_X16 (n int32:
 *                    1 when every count of the gene is a whole number in [0, 65535])
 * DN_E_INVALID for a null handle, a null pointer or an unknown array, DN_E_STATE when nothing is uploaded.                    */
#define DN_PLANT_RHO_RAW 0
#define DN_PLANT_FLAGS 1
#define DN_PLANT_ITER_STATUS 2
#define DN_PLANT_EST_SUMS 3
#define DN_PLANT_COV_SUMS 4
#define DN_PLANT_INIT_STATUS 5
#define DN_PEEK_ROWMAX 0
#define DN_PEEK_X16 1
int  dn_debug_plant(dn_handle h, int32_t which, const void *src);
int  dn_debug_peek(dn_handle h, int32_t which, void *dst);

/* Estimated coverage matrices of the last dn_baseline_iteration run with want_estimates = 1 ----------
 * Replaces: the `estimate` output of baseline_selection (nmf.py:355-369), returned by run() (nmf.py:601).
 * out: float64, gene g at element offset p * sum(lengths[:g]), p x L_g row-major.                     */
int  dn_fetch_estimates(dn_handle h, double *out);
/* The same for a chosen subset (plots and reports only read a handful of genes, report.py:97-113,
 * __main__.py:291-316): gene_ids[n_sel] in upload order; out holds the selected genes back to back, in that order. */
int  dn_fetch_estimates_subset(dn_handle h, int64_t n_sel, const int64_t *gene_ids, double *out);

/* The float64-input path: per-gene calls on matrices as given ------------------------------------------------
 * Replaces: GeneNMFOA.rank_one_approx / nmf / ratio_svd / run_ratio_svd_serial / baseline_selection /
 * run_baseline_selection_serial (nmf.py:55-121, :189-375) and their module twins (nmf_mpi.py:10-78, :174-378) called on
 * arbitrary float64 matrices -- e.g. coverage already scaled by 1/s_i (nmf.py:196, :563), which the float32 count storage
 * of dn_upload_* cannot hold exactly.  Each call is one kernel launch over the whole batch (longest-first work queue) in
 * device buffers of its own: the handle's resident coverage, scratch slots and outer-iteration state are not touched, so
 * dn_fetch_estimates* and the dn_outer_* calls see what they saw before.  x[m] / F[m]: C-contiguous p x lengths[m] float64.
 * Outputs are packed back to back in caller order (K: n x p; E and est at the running column offset, est p x L each).
 * 2 <= p <= 64, else DN_E_UNSUPPORTED (dn_p_supported is about the count path and unchanged).
 *
 * dn_nmf_f64  mode DN_NMF_RANK_ONE: svds(x, k=1) -> K = u sigma, E = v (nmf.py:55-64)
 *             mode DN_NMF:          nmf(x) with nmf_iter (>= 0) Lagrangian iterations, factors K, E (nmf.py:78-107)
 *             mode DN_NMF_RATIO:    rank one, est = max(K E, x) (nmf.py:109-121)
 *             est (nullable) receives K E (or the clamped estimate); status[n]: 0, or -3 for min(p, n_k) < 2 (svds'
 *             ValueError), -1 for an all-zero matrix (ArpackError), -4 for an eigen-solve left through its step cap.
 * dn_baseline_selection_f64  baseline_selection (nmf.py:189-372) on F as given (scale 1): rho[n*p] unclipped, flags[n]
 *             (ran_baseline_selection), trace[n*DN_TRACE_LEN] (nullable; [6] is the status), est (nullable; the
 *             estimate of every gene).  prm->want_estimates is ignored (est decides).  ds_start: as dn_baseline_iteration. */
#define DN_NMF_RANK_ONE       0
#define DN_NMF                1
#define DN_NMF_RATIO          2
int  dn_nmf_f64(dn_handle h, int64_t n, int32_t p, const double *const *x, const int64_t *lengths, int32_t mode,
                int32_t nmf_iter, double *K, double *E, double *est, int32_t *status);
int  dn_baseline_selection_f64(dn_handle h, int64_t n, int32_t p, const double *const *F, const int64_t *lengths,
                               const dn_params *prm, const int64_t *ds_start, double *rho, int32_t *flags,
                               int32_t *trace, double *est);
/* Device time in ms of the kernel(s) of the most recent dn_nmf_f64 / dn_baseline_selection_f64 call.                  */
double dn_last_f64_ms(dn_handle h);

/* Coverage-matrix assembly -------------------------------------------------------------
 * Replaces: the densify-and-slice loop of merge_chrom_coverage (reads_coverage_merge.py:283-353).
 * Per sample i the chromosome coverage is the CSR row written by reads.py:785-786: nnz[i] positions indices[i][]
 * (0-based) with values[i][] (nnz[i] = 0: file missing, imputed as zeros, :309-316).  Each gene's union of exons is
 * given as chunks (<= any length): chunk c copies chunk_len[c] positions starting at chromosome position chunk_src[c]
 * to column chunk_dst_in_gene[c] of gene chunk_gene[c].  out_packed: float32, gene g at p * sum(lengths[:g]),
 * p rows of lengths[g] -- the layout dn_upload_packed takes.  device_ms (nullable): device time of the assembly. */
int  dn_assemble_coverage(int device, int64_t chrom_len, int32_t p, const int64_t *nnz,
                          const int32_t *const *indices, const float *const *values,
                          int64_t n_genes, const int64_t *lengths,
                          int64_t n_chunks, const int32_t *chunk_gene, const int64_t *chunk_src,
                          const int64_t *chunk_dst_in_gene, const int32_t *chunk_len,
                          float *out_packed, double *device_ms);
const char *dn_assemble_last_error(void);          /* = dn_last_error() */

/* Reads -> coverage and read counts (one sample, one chromosome) -------------------------------------
 * Replaces: the per-read loop of BamReadsProcessor.chromosome_coverage_read_counts (reads.py:397-774): CIGAR parsing
 * (cigar_segment_bounds, :9-66; end_pos :404-405), the position pre-filter (:410-413), the pair filter (:417-420), the
 * mate clipping (:459-470), the exon-union filter (:423-516), the overlap-group stage (:545-644) and the isolated-gene
 * stage (:669-786).  Positions are the reference's 0-based read positions; every interval below is closed [lo, hi],
 * given as flat (lo, hi) pairs sorted by lo.
 *   reads     n_rows rows in the caller's order: pos, CIGAR bytes cigar[cigar_off[r] .. cigar_off[r+1]) (ASCII), and when
 *             paired the pair id of every row (0 .. n_pair_ids-1, the qname without its mate suffix); pairs are the
 *             consecutive rows left after the pre-filter keep_lo <= pos, end_pos <= keep_hi and the two-rows-per-id rule.
 *   exon_iv   the merged union of all exons (0-based [start-1, end-1]; touching exons merged).
 *   groups    n_groups overlap groups, disjoint spans group_iv ([min gene_start-1, max gene_end-1]); the genes of group g are
 *             entries group_gene_off[g] .. group_gene_off[g+1] of the ol_* arrays: ol_gene (index into counts),
 *             ol_gene_start0 (gene_start-1), their exon bounds ol_exon_bounds[ol_exon_off[q] ..] as (start-1, end) pairs of
 *             separately sorted starts and ends (:575), and their span vectors at ol_cov_off[q] .. ol_cov_off[q+1]-1 of
 *             ol_cov (gene_end - gene_start + 1 values, then one pad slot).
 *   isolated  n_iso disjoint gene spans iso_iv ([gene_start-1, gene_end-1]) with their count indices iso_gene, and the
 *             merged union of those spans iso_union.
 * Outputs: counts[n_genes] (read counts), ol_cov (the span vectors, before the projection onto exon positions of :644),
 * the chromosome coverage as CSR nonzeros (*nnz positions csr_idx ascending, values csr_val; at most csr_cap: the length
 * of the exon union bounds it), *n_isolated_reads (0: the reference writes no chrom_coverage file, :711) and device_ms
 * (nullable).  A kept row whose CIGAR has no M op returns DN_E_INVALID (the reference's ValueError, :63-64); one with more
 * than DN_READS_MAX_SEG M ops returns DN_E_UNSUPPORTED (both are ValueError in the Python layer, with the CIGAR in the
 * text).  A read or pair with a segment bound below position 0 is dropped (the reference indexes from the vector's end
 * there).  Such a bound arises in two ways: a zero-length M op at position 0 (`0M10M` at 0 has the bounds 0, -1, -1, 8),
 * single-end or paired, and a mate 2 clipped to the left of a mate 1 that starts at position 0.  Results are bit-identical
 * from run to run.  Text of the last error: dn_reads_last_error(). */
#define DN_READS_MAX_SEG      32  /* match segments (M ops) per row                                                   */
int  dn_read_coverage(int device, int32_t paired, int64_t n_rows, const int64_t *pos, const int64_t *cigar_off,
                      const uint8_t *cigar, const int32_t *pair_id, int64_t n_pair_ids,
                      int64_t chrom_len, int64_t keep_lo, int64_t keep_hi,
                      int64_t n_exon, const int64_t *exon_iv,
                      int64_t n_groups, const int64_t *group_iv, const int32_t *group_gene_off,
                      const int32_t *ol_gene, const int64_t *ol_gene_start0, const int64_t *ol_cov_off,
                      const int32_t *ol_exon_off, const int64_t *ol_exon_bounds,
                      int64_t n_iso, const int64_t *iso_iv, const int32_t *iso_gene,
                      int64_t n_iso_union, const int64_t *iso_union,
                      int64_t n_genes, int64_t *counts, int64_t *ol_cov,
                      int64_t csr_cap, int64_t *nnz, int32_t *csr_idx, int64_t *csr_val,
                      int64_t *n_isolated_reads, double *device_ms);
/* Debug view of the device CIGAR parser (cigar_segment_bounds, :9-66): per row nseg[r] match segments (0: no M op, -1: more
 * than max_seg) as bounds[r * 2 * max_seg ..] (start, end inclusive), and end_pos[r] = pos + sum of all op lengths (:404). */
int  dn_reads_cigar_bounds(int device, int64_t n, const int64_t *pos, const int64_t *cigar_off, const uint8_t *cigar,
                           int32_t max_seg, int32_t *nseg, int64_t *bounds, int64_t *end_pos);
const char *dn_reads_last_error(void);             /* = dn_last_error() */

/* BAM records -> coverage and read counts (NativeBamReadsProcessor, degnorm_amd/bam.py) ------------------------------
 * The host inflates a chromosome's BGZF blocks window by window; the device decodes the records and keeps the rows the
 * reference's load_chromosome_reads keeps (reads.py): refID == tid, no NH > 1 when unique_alignment (NH of any integer type;
 * another type is DN_E_INVALID), and when paired next_refID != -1.  Kept rows go, in file order, into a device-resident
 * row store; the coverage stages of dn_read_coverage then read their binary CIGARs in place.
 *   dn_bam_frame          host only: the start offsets of the complete records of buf (a walk over block_size), at most
 *                         cap of them; *consumed = the bytes they span (the rest is a record cut by the window end).  With
 *                         tid >= 0 every record must have refID tid and a pos no smaller than the one before it (*last_pos,
 *                         carried between windows; start at INT32_MIN), else DN_E_INVALID (unsorted file or stale index).
 *   dn_bam_rows_create    an empty row store on `device` for reference tid.
 *   dn_bam_rows_append    decode the n_rec records of one window (offsets from dn_bam_frame) and append its kept rows.  An op
 *                         code above 8 or a CIGAR moved to the CG tag in a kept row: DN_E_UNSUPPORTED.
 *   dn_bam_rows_info      rows, CIGAR ops and name bytes stored, and the longest qname_unpaired key (nullable outputs).
 *   dn_bam_rows_keys      every row's qname_unpaired (the name up to its last '.'; empty without one) as width bytes,
 *                         NUL padded: n_rows x width.
 *   dn_bam_rows_fetch     the rows (nullable outputs): pos, their ops at op_beg[r] .. op_beg[r] + n_op[r] of ops (len << 4 |
 *                         op), their names at name_beg[r] .. name_beg[r] + name_len[r] of names (without NUL).
 *   dn_bam_rows_coverage  dn_read_coverage on the stored rows, taken in `order` (row indices; required when paired, NULL for
 *                         file order) with pair_id[k] the pair id of the k-th row taken.  A kept row without CIGAR ops gives
 *                         DN_E_INVALID naming the read (the reference's regex fails on cigarstring None).
 *                         A paired store that dn_bam_rows_pair has paired also takes order == NULL and pair_id == NULL: the
 *                         call then reads the store's own two arrays where they lie, and n_pair_ids is ignored.
 *   dn_bam_rows_pair      pair the mates of a paired store on its device (csrc/dn_pair.hip) and keep the result there:
 *                         `order`, the rows in ascending qname_unpaired order, and `pair_id`, for every position of that
 *                         order the number of distinct keys before it; *n_pair_ids = the last id + 1 (0 for no rows).
 *                         Keys compare as unsigned bytes, zero-padded to the longest key (a key that is a prefix of
 *                         another comes first), and rows of equal key stay in ascending row order, which is file order:
 *                         order is np.argsort(keys, kind='stable') on the keys of dn_bam_rows_keys.  This is not the
 *                         reference's order for equal keys -- there pandas' quicksort leaves the two mates of a pair in
 *                         an order of its own making -- and the clipping of a pair's second mate against its first is
 *                         not symmetric; the results can differ only for pairs whose mates overlap on the reference.
 *                         order_out / pair_id_out (n_rows each, nullable) receive copies, for tests.  An unpaired store
 *                         is DN_E_INVALID.  Rows appended later end the pairing.
 *   dn_bam_pair_host      host only: the same order and ids for n keys names[name_beg[r] .. name_beg[r] + key_len[r]),
 *                         by the same passes with std::stable_sort; n below 2^31.
 *   dn_bam_cigar_bounds   dn_reads_cigar_bounds on binary CIGARs: row r's ops are ops[op_off[r] .. op_off[r+1]).
 *
 * Read filters and pairing by FLAG (dn_bam_rows_create_with; with every option 0 it is dn_bam_rows_create).
 * Read filters, of a single-end and a paired store alike.  A well-formed record of refID tid is dropped
 *   - when flag & exclude_flags != 0, or flag & require_flags != require_flags (counted as dropped by flags), else
 *   - when its MAPQ byte, 0 .. 255 taken as that number, is below min_mapq (counted as dropped by MAPQ).
 * The filters come before the NH rule, the mate rule and the CIGAR checks: a record they drop raises none of the errors of
 * a kept row (NH of a non-integer type, no CIGAR, an unsupported op, a CIGAR in CG); a malformed record is an error
 * whatever the filters say.
 * Pairing by FLAG (pairing = DN_PAIR_BY_FLAG on a paired store; aligners that give both mates of a template one QNAME).
 *   - Candidate rows are the records that pass the read filters and the NH rule and have 0x1 set, 0x4 and 0x8 clear,
 *     next_refID == tid and exactly one of 0x40 and 0x80 set.  No other record is stored (counted as not a candidate);
 *     this stands in for the rule next_refID != -1.
 *   - The mate key of a row is (QNAME bytes, pos_first, pos_last): a 0x40 row has pos_first = pos and pos_last = next_pos,
 *     a 0x80 row pos_first = next_pos and pos_last = pos.  Two alignments of one multi-mapping template at different loci
 *     have different keys.
 *   - dn_bam_rows_pair orders the rows by name -- unsigned bytes, zero-padded, as above, the whole name being the key --
 *     then by (uint32) (pos_first + 1), then by (uint32) (pos_last + 1); rows of equal key stay in file order, and pair_id
 *     is the number of distinct keys before a position.
 *   - A pair is a key whose rows, among those that pass the position pre-filter of the coverage stages (keep_lo, keep_hi),
 *     are exactly two, one with 0x40 and one with 0x80.  Any other composition contributes nothing.  Mate 1 of the
 *     asymmetric clipping is the row that comes first in the file.
 *   dn_bam_rows_coverage of such a store takes the pairing of dn_bam_rows_pair only (order == NULL, pair_id == NULL), and
 *   at most 2^30 rows.
 *   dn_bam_rows_dropped      what each rule dropped in the windows appended so far (nullable outputs).
 *   dn_bam_rows_fetch_mates  FLAG, MAPQ and next_pos of the rows of a store that pairs by FLAG (nullable outputs; any other
 *                            store is DN_E_INVALID: it does not keep them).
 *   dn_bam_mate_host         host only: order and ids of the FLAG rule for n rows with names names[name_beg[r] .. name_beg[r] +
 *                            name_len[r]), by the passes of dn_bam_rows_pair with std::stable_sort.  A row with 0x40 set counts
 *                            as a first mate, any other as a last one.
 * Errors: dn_reads_last_error(). */
typedef struct dn_bam_rows_s *dn_bam_rows;
enum { DN_PAIR_BY_NAME = 0, DN_PAIR_BY_FLAG = 1 };
typedef struct {
    int32_t  pairing;                   /* DN_PAIR_BY_NAME or DN_PAIR_BY_FLAG (which matters to a paired store only) */
    uint32_t exclude_flags;             /* up to 0xffff */
    uint32_t require_flags;             /* up to 0xffff */
    int32_t  min_mapq;                  /* 0 .. 255 */
} dn_bam_rows_options;
int  dn_bam_rows_create_with(int device, int32_t tid, int32_t unique_alignment, int32_t paired, const dn_bam_rows_options *opt,
                             dn_bam_rows *out);
int  dn_bam_rows_dropped(dn_bam_rows h, int64_t *by_flags, int64_t *by_mapq, int64_t *not_candidate);
int  dn_bam_rows_fetch_mates(dn_bam_rows h, uint16_t *flag, uint8_t *mapq, int32_t *next_pos);
int  dn_bam_mate_host(int64_t n, const int64_t *name_beg, const int32_t *name_len, const uint8_t *names, const int64_t *pos,
                      const int32_t *next_pos, const uint16_t *flag, int32_t *order, int32_t *pair_id, int64_t *n_pair_ids);
int  dn_bam_frame(const uint8_t *buf, int64_t n_bytes, int32_t tid, int32_t *last_pos, int64_t *rec_off, int64_t cap,
                  int64_t *n_rec, int64_t *consumed);
int  dn_bam_rows_create(int device, int32_t tid, int32_t unique_alignment, int32_t paired, dn_bam_rows *out);
void dn_bam_rows_destroy(dn_bam_rows h);
int  dn_bam_rows_append(dn_bam_rows h, const uint8_t *window, int64_t n_bytes, const int64_t *rec_off, int64_t n_rec);
int  dn_bam_rows_info(dn_bam_rows h, int64_t *n_rows, int64_t *n_ops, int64_t *n_name_bytes, int32_t *max_key_len);
int  dn_bam_rows_keys(dn_bam_rows h, int32_t width, uint8_t *keys);
int  dn_bam_rows_fetch(dn_bam_rows h, int64_t *pos, int64_t *op_beg, int32_t *n_op, uint32_t *ops, int64_t *name_beg,
                       int32_t *name_len, uint8_t *names);
int  dn_bam_rows_coverage(dn_bam_rows h, const int32_t *order, const int32_t *pair_id, int64_t n_pair_ids,
                          int64_t chrom_len, int64_t keep_lo, int64_t keep_hi,
                          int64_t n_exon, const int64_t *exon_iv,
                          int64_t n_groups, const int64_t *group_iv, const int32_t *group_gene_off,
                          const int32_t *ol_gene, const int64_t *ol_gene_start0, const int64_t *ol_cov_off,
                          const int32_t *ol_exon_off, const int64_t *ol_exon_bounds,
                          int64_t n_iso, const int64_t *iso_iv, const int32_t *iso_gene,
                          int64_t n_iso_union, const int64_t *iso_union,
                          int64_t n_genes, int64_t *counts, int64_t *ol_cov,
                          int64_t csr_cap, int64_t *nnz, int32_t *csr_idx, int64_t *csr_val,
                          int64_t *n_isolated_reads, double *device_ms);
int  dn_bam_rows_pair(dn_bam_rows h, int32_t *order_out, int32_t *pair_id_out, int64_t *n_pair_ids, double *device_ms);
int  dn_bam_pair_host(int64_t n, const int64_t *name_beg, const int32_t *key_len, const uint8_t *names, int32_t *order,
                      int32_t *pair_id, int64_t *n_pair_ids);
int  dn_bam_cigar_bounds(int device, int64_t n, const int64_t *pos, const int64_t *op_off, const uint32_t *ops,
                         int32_t max_seg, int32_t *nseg, int64_t *bounds, int64_t *end_pos);

/* Strand-specific counting -------------------------------------------------------------------------------------------
 * For stranded libraries (Illumina TruSeq Stranded / dUTP and the like), where a read's orientation tells the strand its
 * fragment came from.  The reference has no such mode; the rule is this library's, and it is stated so that the unstranded
 * path above, which is held to the reference, is its oracle.  `stranded` is 'no' (0, the default: everything above, as it
 * is), 'forward' (1) or 'reverse' (2).
 * Sense of a row (dn::row_sense, csrc/dn_bam_record.hpp; a function of one record):
 *   - a row is a last mate when FLAG 0x1 and 0x80 are both set; in a store paired by the name rule also when the last
 *     byte of its name is '2'.  Every other row counts as a first mate or a single read;
 *   - sense is '-' when FLAG 0x10 is set, else '+'; it is flipped for a last mate, and once more when stranded is
 *     'reverse' (dUTP: htseq-count -s reverse, featureCounts -s 2; 'forward' is -s yes / -s 1).
 * Strand of a gene: '+' or '-' when every exon row of the gene says so in field 7 of the annotation; a gene with '.', '?'
 * or both strands among its rows is unstranded and is left out of a stranded run.
 * A stranded chromosome is two chromosomes.  For each strand s, '+' then '-': the genes of strand s and their exons, their
 * own overlap structure (overlap groups and isolated genes among the genes of that strand only), their own keep_lo,
 * keep_hi, exon union, groups and isolated spans, and the rows whose sense is s, handed to the coverage stages above
 * unchanged: the position pre-filter additionally asks for sense == s.  A strand without genes is skipped.
 * Paired files: a stranded run pairs on the device, equal keys in file order (dn_bam_rows_pair).  The strand test is part
 * of the position pre-filter and is applied per row, so a pair whose two mates disagree about the fragment's sense leaves
 * one row on each strand, fails the "exactly two rows" rule in both passes and contributes nothing.
 * Guarantee: a stranded run over annotation A and file B gives, gene for gene -- read counts, overlap coverage vectors and
 * chromosome coverage -- what the unstranded code gives on (A+, B+) and on (A-, B-), where As is the exon lines of the
 * genes on strand s and Bs the records of sense s, in file order.
 *   dn_read_coverage_strand      dn_read_coverage with sense[r] ('+' or '-') of every row and the strand counted ('+' or '-').
 *   dn_read_sense_host           host only: dn::row_sense of n rows with these FLAGs and last name bytes (0: empty name);
 *                                by_name != 0: the rows of a store paired by the name rule; stranded 1 or 2.
 *   dn_bam_rows_set_stranded     make an empty store keep the sense of its rows under protocol `stranded` (1 or 2; 0 ends
 *                                it).  A store with rows is DN_E_STATE.  The sense is computed where the window is decoded,
 *                                which also covers a store paired by the name rule, which does not keep FLAG.
 *   dn_bam_rows_fetch_sense      the sense of every row of a stranded store (any other store: DN_E_INVALID).
 *   dn_bam_rows_coverage_strand  dn_bam_rows_coverage on the rows of one sense of a stranded store.  One store, and one
 *                                dn_bam_rows_pair, serve the calls of both strands. */
int  dn_read_coverage_strand(int device, int32_t paired, int64_t n_rows, const int64_t *pos, const int64_t *cigar_off,
                             const uint8_t *cigar, const int32_t *pair_id, int64_t n_pair_ids, const uint8_t *sense, int32_t strand,
                             int64_t chrom_len, int64_t keep_lo, int64_t keep_hi,
                             int64_t n_exon, const int64_t *exon_iv,
                             int64_t n_groups, const int64_t *group_iv, const int32_t *group_gene_off,
                             const int32_t *ol_gene, const int64_t *ol_gene_start0, const int64_t *ol_cov_off,
                             const int32_t *ol_exon_off, const int64_t *ol_exon_bounds,
                             int64_t n_iso, const int64_t *iso_iv, const int32_t *iso_gene,
                             int64_t n_iso_union, const int64_t *iso_union,
                             int64_t n_genes, int64_t *counts, int64_t *ol_cov,
                             int64_t csr_cap, int64_t *nnz, int32_t *csr_idx, int64_t *csr_val,
                             int64_t *n_isolated_reads, double *device_ms);
int  dn_read_sense_host(int64_t n, const uint16_t *flag, const uint8_t *name_last, int32_t by_name, int32_t stranded, uint8_t *sense);
int  dn_bam_rows_set_stranded(dn_bam_rows h, int32_t stranded);
int  dn_bam_rows_fetch_sense(dn_bam_rows h, uint8_t *sense);
int  dn_bam_rows_coverage_strand(dn_bam_rows h, int32_t strand, const int32_t *order, const int32_t *pair_id, int64_t n_pair_ids,
                                 int64_t chrom_len, int64_t keep_lo, int64_t keep_hi,
                                 int64_t n_exon, const int64_t *exon_iv,
                                 int64_t n_groups, const int64_t *group_iv, const int32_t *group_gene_off,
                                 const int32_t *ol_gene, const int64_t *ol_gene_start0, const int64_t *ol_cov_off,
                                 const int32_t *ol_exon_off, const int64_t *ol_exon_bounds,
                                 int64_t n_iso, const int64_t *iso_iv, const int32_t *iso_gene,
                                 int64_t n_iso_union, const int64_t *iso_union,
                                 int64_t n_genes, int64_t *counts, int64_t *ol_cov,
                                 int64_t csr_cap, int64_t *nnz, int32_t *csr_idx, int64_t *csr_val,
                                 int64_t *n_isolated_reads, double *device_ms);

/* BGZF inflate on the device (csrc/dn_inflate.hip) ----------------------------------------------------------------------
 * A raw-DEFLATE (RFC 1951) decoder of the library's own: one BGZF block per wavefront, no zlib.  Block b's payload (the
 * bytes between its gzip header and its CRC32 / ISIZE trailer) is comp[pay_off[b] .. pay_off[b] + pay_len[b]) and must
 * inflate to exactly out_off[b+1] - out_off[b] bytes (its ISIZE, 0 .. 65536), which go to out + out_off[b]; out_off has
 * n_blocks + 1 entries and starts at 0.  The input is untrusted: a block that does not decode sets status[b] to one of the
 * DN_INFLATE_E_* below, leaves its output bytes unspecified and does not fail the call (DN_OK); status[b] = 0 otherwise.
 * Arrays that contradict each other (a payload outside comp, a size outside 0 .. 65536, out_off not monotone): DN_E_INVALID.
 *   dn_bgzf_inflate_host  the same decoder source compiled for the host, one block after the other; no device is touched.
 *   dn_bgzf_inflate       copy comp to `device`, inflate, copy back to out (host memory).  copy_ms / device_ms (nullable):
 *                         the copy in and the kernel, by HIP events.
 *   dn_bam_rows_inflate   build the next window of a row store on its device: n_carry bytes of `carry` (the record cut by the
 *                         end of the window before), then the inflated blocks; the first block loses its first head_skip
 *                         bytes, the last one is cut to tail_keep bytes first (tail_keep < 0: kept whole).  *host_window
 *                         points at a pinned host copy of the *n_bytes of the window (owned by the store, valid until its
 *                         next dn_bam_rows_inflate or its destruction) for dn_bam_frame; the window stays resident unless a
 *                         block failed.  isize[b] may exceed 65536 here (the decoder keeps 32 KiB of history, not the
 *                         block, and zlib-based readers accept such files).  device_ms (nullable): the inflate kernel.
 *   dn_bam_rows_append_resident   dn_bam_rows_append on the resident window, without uploading it again; DN_E_STATE when
 *                         there is none.
 * The CRC32 of a block's trailer (RFC 1952: reflected polynomial 0xEDB88320, register 0xFFFFFFFF at the start, inverted at
 * the end) is compared with the inflated bytes only where the caller asks for it; a block that decodes and differs gets
 * status[b] = DN_INFLATE_E_CRC, and a block that does not decode keeps its decode error.  The CRC covers the whole block,
 * also the bytes a head_skip or tail_keep leaves out of the window.  On the device every lane of the block's wavefront takes
 * one slice of the bytes the LDS ring is about to flush and the wave combines the slices ("BGZF inflate").
 *   dn_bgzf_inflate_check_host / dn_bgzf_inflate_check   dn_bgzf_inflate_host / dn_bgzf_inflate with crc32[b], the CRC32 of
 *                         block b's trailer; crc32 == NULL: no check.  out == NULL: the blocks are decoded and checked and
 *                         their bytes dropped (on the device nothing is written or copied back but the statuses).
 *   dn_bgzf_crc32_host    *crc = the CRC32 of data[0 .. n) by the routines the kernel uses: the data cut into spans of
 *                         flush_bytes (at least 1) as the ring's flushes cut a block, every span into `lanes` slices
 *                         (1 .. 64; else DN_E_INVALID).  No device is touched.
 *   dn_bam_rows_expect_crc   arm the store's next dn_bam_rows_inflate or dn_bam_rows_inflate_framed with the trailer CRC32 of
 *                         each of its n_blocks blocks.  That call consumes the arming whatever it returns; when its block
 *                         count is another, it returns DN_E_INVALID before it touches the store.
 *   dn_bai_expect_crc     the same for a device builder's next dn_bai_window; DN_E_STATE on a host builder, whose caller
 *                         holds the inflated bytes and checks them itself.
 * Errors: dn_reads_last_error(). */
#define DN_INFLATE_E_HEADER    1   /* block type 3, a stored block whose LEN / NLEN disagree, too many code lengths         */
#define DN_INFLATE_E_LENGTHS   2   /* over-subscribed or incomplete code lengths, a bad repeat, no end-of-block code        */
#define DN_INFLATE_E_CODE      3   /* a code that is not in the table, or a length / distance symbol that does not exist    */
#define DN_INFLATE_E_DISTANCE  4   /* a distance beyond the output so far                                                   */
#define DN_INFLATE_E_INPUT     5   /* the payload ends before the final block does                                          */
#define DN_INFLATE_E_SIZE      6   /* the output is not ISIZE bytes long                                                    */
#define DN_INFLATE_E_TRAILING  7   /* bytes left in the payload after the final block                                       */
#define DN_INFLATE_E_CRC       8   /* decoded, but the CRC32 of the bytes is not the trailer's (only where it is checked)   */
int  dn_bgzf_inflate_host(const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                          const int64_t *out_off, uint8_t *out, int32_t *status);
int  dn_bgzf_inflate(int device, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                     const int32_t *pay_len, const int64_t *out_off, uint8_t *out, int32_t *status, double *copy_ms,
                     double *device_ms);
int  dn_bam_rows_inflate(dn_bam_rows h, const uint8_t *carry, int64_t n_carry, const uint8_t *comp, int64_t n_comp,
                         int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len, const int32_t *isize,
                         int32_t head_skip, int32_t tail_keep, const uint8_t **host_window, int64_t *n_bytes,
                         int32_t *status, double *device_ms);
int  dn_bam_rows_append_resident(dn_bam_rows h, const int64_t *rec_off, int64_t n_rec);
int  dn_bgzf_inflate_check_host(const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                                const int64_t *out_off, uint8_t *out, int32_t *status, const uint32_t *crc32);
int  dn_bgzf_inflate_check(int device, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                           const int32_t *pay_len, const int64_t *out_off, uint8_t *out, int32_t *status, double *copy_ms,
                           double *device_ms, const uint32_t *crc32);
int  dn_bgzf_crc32_host(const uint8_t *data, int64_t n, int32_t lanes, int32_t flush_bytes, uint32_t *crc);
int  dn_bam_rows_expect_crc(dn_bam_rows h, const uint32_t *crc32, int64_t n_blocks);

/* Record framing on the device (csrc/dn_frame.hip) ----------------------------------------------------------------------
 * dn_bam_frame's walk, block_size to block_size, is serial.  Here the window is cut into segments of segment_bytes (at
 * least 64; 0: the library's default, dn_bam_frame_segment_default()): every segment guesses where a record starts in it
 * and walks the chain from there, the host stitches the per-segment results from offset 0 and has a segment whose guess
 * was not the true entry walked again (a fix-up), and a last pass writes the offsets and checks refID and order.  Offsets,
 * *n_rec, *consumed, *last_pos and every error -- code, text, and which one wins when a window holds several -- equal
 * dn_bam_frame's for every input, whatever the guesses were; *n_fixups (nullable) counts the segments walked again.
 *   dn_bam_frame_segments_host  the same source compiled for the host, one segment after the other; no device is touched.
 *   dn_bam_frame_device   copy buf to `device`, frame it there, copy the offsets back to rec_off (host memory).  device_ms
 *                         (nullable): first framing kernel to the last, by HIP events.  For tests and tools.
 *   dn_bam_rows_append_framed   dn_bam_rows_append without offsets: upload the window, frame it on the device, decode it
 *                         and append its kept rows.  *consumed = the bytes the complete records span; the caller carries
 *                         the rest to its next window.  The store remembers the last pos between calls.
 *   dn_bam_rows_inflate_framed  dn_bam_rows_inflate, then framing, decoding and appending on the device: no host copy of
 *                         the window.  The record cut by the window end stays on the device and starts the next window;
 *                         *n_carry = its bytes, *n_bytes = the bytes of this window.  When a block failed (status[b] != 0)
 *                         the call returns DN_OK before framing, as dn_bam_rows_inflate does.  inflate_ms / frame_ms
 *                         (nullable): the inflate kernel and the framing of this window.
 *   dn_bam_rows_frame_segment   the segment size of a store's framing from now on (0: the default).
 *   dn_bam_rows_frame_info      sums over every window a store framed on the device (nullable outputs): segments, fix-ups,
 *                         the device ms of framing, and the host's ms in decoding and appending those windows.
 * Errors: dn_reads_last_error(). */
int64_t dn_bam_frame_segment_default(void);
int  dn_bam_frame_segments_host(const uint8_t *buf, int64_t n_bytes, int32_t tid, int32_t *last_pos, int64_t segment_bytes,
                                int64_t *rec_off, int64_t cap, int64_t *n_rec, int64_t *consumed, int64_t *n_fixups);
int  dn_bam_frame_device(int device, const uint8_t *buf, int64_t n_bytes, int32_t tid, int32_t *last_pos, int64_t segment_bytes,
                         int64_t *rec_off, int64_t cap, int64_t *n_rec, int64_t *consumed, int64_t *n_fixups, double *device_ms);
int  dn_bam_rows_append_framed(dn_bam_rows h, const uint8_t *window, int64_t n_bytes, int64_t *consumed);
int  dn_bam_rows_inflate_framed(dn_bam_rows h, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off,
                                const int32_t *pay_len, const int32_t *isize, int32_t head_skip, int32_t tail_keep,
                                int32_t *status, int64_t *n_bytes, int64_t *n_carry, double *inflate_ms, double *frame_ms);
int  dn_bam_rows_frame_segment(dn_bam_rows h, int64_t segment_bytes);
int  dn_bam_rows_frame_info(dn_bam_rows h, int64_t *n_segments, int64_t *n_fixups, double *device_ms, double *decode_ms);

/* .bai index of a BAM file (csrc/dn_bai.hip; degnorm_amd.bam.build_index) -------------------------------------------------
 * One pass over every record of a coordinate-sorted file, window by window, all references: per record [beg, end) on its
 * reference (end - beg from the CIGAR ops M D N = X; 1 when flag & 4, without CIGAR or when that sum is 0; beg below 0
 * becomes 0 and end below 1 becomes 1 on a reference), bin = reg2bin(beg, end) of the SAM specification 5.3, and the
 * virtual offset of its first byte.  The index holds, per reference with records, its bins in ascending order -- per bin
 * the chunks of its maximal runs of consecutive records in file order, two joined when the later begins in the BGZF block
 * the earlier ends in, nothing else merged and no bin folded into its parent --, the pseudo-bin's four values and the
 * linear index (per 16 kb window the smallest offset of a record that overlaps it, mapped or not; an empty window takes
 * the next one's value).  A CIGAR kept in the CG tag (more than 65 535 ops) is read as stored in the record.
 *   dn_bai_create         a builder for a file of n_ref references on `device`, or (device < 0) the host build, which
 *                         touches no device.  segment_bytes: of the framing (0: the default).
 *   dn_bai_window         device builder: the next window.  comp holds n_blocks whole BGZF blocks, described as for
 *                         dn_bam_rows_inflate_framed, coffset[b] the file offset of block b; head_skip bytes of the first
 *                         block are left out (the first window starts where the BAM header ends).  The blocks are inflated
 *                         behind the record the window before cut, which waited on the device; the window is framed and
 *                         indexed where it lies, and only the tables of run heads and linear-index claims come back.  When
 *                         a block failed (status[b] != 0) the call returns DN_OK and the builder is spent.  *n_rec: the
 *                         records of this window; inflate_ms / frame_ms / index_ms (nullable): by HIP events.
 *                         dn_bai_expect_crc (BGZF inflate, above) has the next window's blocks checked against their CRC32s.
 *   dn_bai_window_host    host builder: the same on the n_data inflated bytes of the n_blocks blocks.
 *   dn_bai_finish         no more windows; end_voffset is the virtual offset of the end of the stream (the block behind the
 *                         last one that holds a byte, offset 0).  sizes[0 .. 6] = bins (without pseudo-bins), chunks,
 *                         linear-index entries, records, records with refID < 0, windows, framing fix-ups.
 *   dn_bai_fetch          ref_n_bin[n_ref] (without the pseudo-bin), ref_n_intv[n_ref], ref_pseudo[4 n_ref] (offset of the
 *                         first record, end of the last, mapped, unmapped), then per bin in (reference, bin) order bin_id
 *                         and bin_n_chunk, the chunks as (begin, end) pairs, and the linear indexes one after the other.
 * DN_E_INVALID with a text naming the record's ordinal in the file: refID not below n_ref, refID decreasing (a negative
 * one counts as behind every reference), pos decreasing within a reference, beg or end above 2^29, a record whose name
 * and CIGAR do not fit in it, a record that starts beyond byte 65535 of its block (no virtual offset can name it), a record
 * cut by the end of the file, and the errors of the framing.  Host and device builders
 * give the same texts.  After an error a builder only accepts dn_bai_destroy.  Errors: dn_last_error(). */
typedef struct dn_bai_s *dn_bai;
int  dn_bai_create(int device, int32_t n_ref, int64_t segment_bytes, dn_bai *out);
void dn_bai_destroy(dn_bai h);
int  dn_bai_window(dn_bai h, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                   const int32_t *isize, const int64_t *coffset, int32_t head_skip, int32_t *status, int64_t *n_rec,
                   double *inflate_ms, double *frame_ms, double *index_ms);
int  dn_bai_window_host(dn_bai h, const uint8_t *data, int64_t n_data, int64_t n_blocks, const int32_t *isize, const int64_t *coffset,
                        int32_t head_skip, int64_t *n_rec);
int  dn_bai_expect_crc(dn_bai h, const uint32_t *crc32, int64_t n_blocks);
int  dn_bai_finish(dn_bai h, int64_t end_voffset, int64_t *sizes);
int  dn_bai_fetch(dn_bai h, int32_t *ref_n_bin, int32_t *ref_n_intv, uint64_t *ref_pseudo, int32_t *bin_id, int32_t *bin_n_chunk,
                  uint64_t *chunks, uint64_t *ioffset);

/* .csi index of a BAM file (the same builder, csrc/dn_bai.hip; degnorm_amd.bam.build_index(fmt='csi')) ---------------------
 * The binning index of the .bai with two parameters: min_shift, the bits of the smallest bins' span (a "granule" of
 * 2^min_shift bases), and depth, the number of levels below the root bin 0.  It holds one offset per bin in place of the
 * linear index, reaches positions up to 2^(min_shift + 3 depth), and its file is BGZF-compressed.  (14, 5) is the
 * binning of the .bai, whose cap of 2^29 bases is why this index exists.
 *   File.   A BGZF stream that ends with the end-of-file block.  Its inflated bytes, little-endian:
 *             magic "CSI\1", int32 min_shift, int32 depth, int32 l_aux, uint8 aux[l_aux], int32 n_ref;
 *             per reference  int32 n_bin;
 *             per bin        uint32 bin, uint64 loffset, int32 n_chunk, then n_chunk pairs uint64 beg, end;
 *             optionally     uint64 n_no_coor.
 *   Bins.   reg2bin(beg, end):
 *               l = depth; s = min_shift; t = ((1 << 3*depth) - 1) / 7; --end
 *               while l > 0:
 *                   if beg >> s == end >> s: return t + (beg >> s)
 *                   --l; s += 3; t -= 1 << 3*l
 *               return 0
 *           Level l (0 is the root) has 8^l bins from t_l = (8^l - 1) / 7 on, each of 2^s_l bases, s_l = min_shift + 3 (depth - l);
 *           a bin of level l starts at (bin - t_l) << s_l.  The bins that may hold records overlapping [beg, end) are
 *           t_l + (beg >> s_l) .. t_l + ((end - 1) >> s_l) at every level l.  The pseudo-bin is ((1 << 3 (depth + 1)) - 1) / 7 + 1
 *           (37450 at depth 5) with two "chunks", (offset of the first record, end of the last) and (mapped, unmapped);
 *           its loffset is 0.  The largest end an index can hold is 2^(min_shift + 3 depth).
 *   What the builder writes.  Per record [beg, end), the chunks of a bin and the rule that joins them, bins in ascending
 *           order, the pseudo-bin last and n_no_coor always: all as the .bai section above defines them.  l_aux = 0.
 *           loffset(bin) is the virtual offset of the first record of the reference, in file order, whose end lies beyond
 *           the start of the bin's interval: the back-filled linear index of granule 2^min_shift at the bin's first granule.
 *           The builder keeps no such table.  Record r claims the granules max(beg >> min_shift, E(r) + 1) .. (end - 1) >>
 *           min_shift (E(r): the largest last granule of the reference's earlier records), as for the .bai; the claims of a
 *           reference are disjoint and ascending, and loffset(bin) is the offset of the first whose last granule is at or
 *           beyond the bin's first -- a binary search, whatever min_shift is.
 *   Parameters.  min_shift 1 .. 30, depth 0 .. 8, min_shift + 3 depth <= 54.  Where the caller leaves depth open
 *           (bam.build_index(depth=None)) this library takes the smallest depth with 2^(min_shift + 3 depth) >= the longest
 *           reference of the header + 256; this is the library's own rule.  Byte equality with the .csi files of other
 *           programs is not claimed, as it is not for the .bai.
 *   Query (bam.index_chunks).  The chunks of the bins above, without those that end at or below `low`, sorted and coalesced.
 *           low is the largest loffset over the stored bins of the reference whose interval begins at or before beg (0
 *           without one): a record that overlaps the region ends beyond beg, hence beyond such a bin's start.
 *   dn_csi_create         dn_bai_create for a .csi index of (min_shift, depth).  The handle is a dn_bai: dn_bai_window,
 *                         dn_bai_window_host, dn_bai_expect_crc, dn_bai_finish and dn_bai_destroy take it.  dn_bai_finish gives
 *                         sizes[2] = 0 and dn_bai_fetch ref_n_intv = 0 and no ioffset entry (ioffset may be null).
 *   dn_csi_loffset        after dn_bai_finish: loffset[sizes[0]], one per bin in the order of dn_bai_fetch's bin_id.
 *                         DN_E_STATE on a dn_bai_create builder.
 * Errors as for the .bai, but for the range: "<record> reaches beyond position 2^<min_shift + 3 depth>: a .csi index of
 * min_shift <m> and depth <d> cannot hold it". */
int  dn_csi_create(int device, int32_t n_ref, int64_t segment_bytes, int32_t min_shift, int32_t depth, dn_bai *out);
int  dn_csi_loffset(dn_bai h, uint64_t *loffset);

/* Coordinate sort of a BAM file (csrc/dn_sort.hip; degnorm_amd.bam.sort_bam) ----------------------------------------------
 * The order: records ascend by key = ref_key << 32 | (uint32) (pos + 1), where ref_key is refID, or the largest 32-bit
 * value for refID -1 -- unplaced records go last, and pos -1 sorts first within its reference -- and records of equal key
 * keep the order they have in the input (a stable sort; flag, strand and read name play no part).  The whole inflated
 * record stream of the file (what follows the BAM header; n_inflated bytes) is held twice: as read and sorted.
 *   dn_bam_sort_device_memory   free and total bytes of `device` (hipMemGetInfo), for the caller's check before a sort.
 *   dn_bam_sort_create    a sort of a file of n_ref references and n_inflated bytes of records on `device`, or (device < 0)
 *                         the host build, which touches no device.  segment_bytes: of the framing (0: the default);
 *                         piece_bytes: the stream is framed this many bytes at a time (0: 256 MiB; a piece grows when a
 *                         record is longer than it).
 *   dn_bam_sort_window    device sort: the next blocks of the file, described as for dn_bai_window, inflated to their place in
 *                         the stream; head_skip bytes of the first block are left out (the first window starts where the BAM
 *                         header ends).  When a block failed (status[b] != 0) the call returns DN_OK and the sort is spent.
 *                         dn_bam_sort_expect_crc has the next window's blocks checked against the CRC32s of their trailers
 *                         (DN_E_STATE on a host sort, whose caller holds the inflated bytes and checks them itself).
 *   dn_bam_sort_window_host   host sort: the next n_data inflated bytes, without their first head_skip.
 *   dn_bam_sort_finish    no more windows: frame the stream, compute key and length of every record and check it, sort
 *                         (key, ordinal) stably, sum the lengths in sorted order and copy every record to its place.
 *                         *n_records and *n_bytes: of the sorted stream; nullable: the framing's fix-ups, and the device ms
 *                         of framing, of keys + sort + sum, and of the copy (0 on the host).
 *   dn_bam_sort_ends      ends[k] = the byte of the sorted stream at which record first + k ends, for n records.
 *   dn_bam_sort_read      n bytes of the sorted stream from byte off on, to dst (host memory).
 * DN_E_INVALID with a text naming the record's ordinal in the input, the first such record winning: a block_size below 32,
 * a record whose name and CIGAR do not fit in it, refID outside -1 .. n_ref - 1, pos below -1, a record cut by the end of
 * the file.  Host and device sorts give the same texts and the same stream.  After an error a sort only accepts
 * dn_bam_sort_destroy.  Errors: dn_last_error(). */
typedef struct dn_bam_sort_s *dn_bam_sort;
int  dn_bam_sort_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes);
int  dn_bam_sort_create(int device, int32_t n_ref, int64_t n_inflated, int64_t segment_bytes, int64_t piece_bytes, dn_bam_sort *out);
void dn_bam_sort_destroy(dn_bam_sort h);
int  dn_bam_sort_window(dn_bam_sort h, const uint8_t *comp, int64_t n_comp, int64_t n_blocks, const int64_t *pay_off, const int32_t *pay_len,
                        const int32_t *isize, int32_t head_skip, int32_t *status, double *inflate_ms);
int  dn_bam_sort_window_host(dn_bam_sort h, const uint8_t *data, int64_t n_data, int32_t head_skip);
int  dn_bam_sort_expect_crc(dn_bam_sort h, const uint32_t *crc32, int64_t n_blocks);
int  dn_bam_sort_finish(dn_bam_sort h, int64_t *n_records, int64_t *n_bytes, int64_t *n_fixups, double *frame_ms, double *sort_ms,
                        double *gather_ms);
int  dn_bam_sort_ends(dn_bam_sort h, int64_t first, int64_t n, int64_t *ends);
int  dn_bam_sort_read(dn_bam_sort h, int64_t off, int64_t n, uint8_t *dst);

/* BGZF deflate (csrc/dn_deflate.hip; degnorm_amd.bam.bgzf_deflate, sort_bam(deflate='native')) -----------------------------
 * The library's own DEFLATE encoder, the counterpart of dn_bgzf_inflate: byte ranges of at most 0xff00 bytes become whole
 * BGZF blocks -- the 18-byte header with BSIZE, a raw-DEFLATE payload (RFC 1951), CRC32 and ISIZE.  One source, written
 * against a memory policy: the host build runs lane after lane, the device build one 64-lane workgroup per block, and both
 * write the same bytes for every input ("BGZF deflate", defines the parse).  Every byte string is a valid input,
 * so there is no per-block status.  Block b holds data[beg[b] .. beg[b] + len[b]); the blocks are written back to back into
 * out, block b at out_off[b], and out_off[n_blocks] is their size.  No DEFLATE block is larger than its stored form, so a
 * block of len bytes is at most len + 26 + 6 * max(1, ceil(len / 8192)) bytes, below 65536:
 *   dn_bgzf_deflate_bound       the sum of that bound over len[0 .. n_blocks): the out_cap that always suffices; -1 when a
 *                         length is outside 0 .. 0xff00.
 *   dn_bgzf_deflate_host  the host build; no device is touched.
 *   dn_bgzf_deflate       copy data to `device`, deflate there (one wave per block into a 64 KiB slot of its own, at most
 *                         1024 blocks in flight; the slots are compacted on the device) and copy only the blocks back.
 *                         device_ms (nullable): the kernels, by HIP events.
 *   dn_deflate_code_lengths_host   the code-length builder the encoder uses, for tests: lens[0 .. n) of a prefix code for
 *                         the symbols with freq != 0, no length above `limit` (n is 1 .. 288, limit 1 .. 15, 2^limit at
 *                         least n).  Huffman's lengths where they fit the limit; always a complete code (Kraft sum 1) when
 *                         two or more symbols are used; one used symbol gets length 1; unused symbols get 0.
 *   dn_bam_sort_deflate   ranges of the sorted stream of a finished sort (dn_bam_sort_finish returned DN_OK; DN_E_STATE
 *                         otherwise, and for a sort that has failed) as BGZF blocks.  A device sort deflates the stream
 *                         where it lies; the unsorted copy, dead since the sort finished, lends the slots and the room for
 *                         the compacted blocks (a stream too small for one slot gets 128 KiB of its own), and the sort's
 *                         key and offset tables are released at the first call, so the device need stays below the
 *                         sort's.  A host sort (device < 0) runs the host build.  deflate_ms (nullable): the kernels.
 * DN_E_INVALID before any launch: a length outside 0 .. 0xff00, a range outside data (or the stream), an out_cap below
 * dn_bgzf_deflate_bound.  Errors: dn_last_error(). */
int64_t dn_bgzf_deflate_bound(int64_t n_blocks, const int32_t *len);
int  dn_bgzf_deflate_host(const uint8_t *data, int64_t n_data, int64_t n_blocks, const int64_t *beg, const int32_t *len, uint8_t *out,
                          int64_t out_cap, int64_t *out_off);
int  dn_bgzf_deflate(int device, const uint8_t *data, int64_t n_data, int64_t n_blocks, const int64_t *beg, const int32_t *len,
                     uint8_t *out, int64_t out_cap, int64_t *out_off, double *device_ms);
int  dn_deflate_code_lengths_host(const uint32_t *freq, int32_t n, int32_t limit, uint8_t *lens);
int  dn_bam_sort_deflate(dn_bam_sort h, int64_t n_blocks, const int64_t *beg, const int32_t *len, uint8_t *out, int64_t out_cap,
                         int64_t *out_off, double *deflate_ms);

/* GTF annotation scan (GeneAnnotationLoader, degnorm_amd/loaders.py) --------------------------------------------------
 * Replaces the reference's read_csv of the nine columns, its lower-case `apply` on the feature column and its regex
 * `apply` per exon row (loaders.py:128-152, _attribute_to_gene :102-112).  buf holds the n_bytes raw bytes of a GTF file,
 * or of a window of it that ends at a line end.  A line ends at '\n' (a '\r' before it belongs to the line end) or at the
 * end of the bytes.  Empty lines and lines whose first byte is '#' are skipped.  Every other line must hold eight tabs
 * (DN_GTF_E_FIELDS); it is kept when its third field is `exon` in any letter case.  A kept line's fourth and fifth fields
 * must be 1 .. 18 decimal digits (DN_GTF_E_INTEGER), and its ninth field (up to a further tab or the line end) must name a
 * gene (DN_GTF_E_GENE): of the pieces between ';', blanks stripped, the first that begins with `gene_name` gives the name
 * -- the rest of the piece without blanks and '"' at either end -- and when there is none, or its value is empty, the
 * first piece that begins with `gene_id` does.
 * Outputs, host arrays of row_cap entries (n_bytes / 20 + 1 always suffices: a kept line is longer than 20 bytes):
 * the kept lines in file order as line (1-based, within buf), the byte span of the chromosome name (chr_beg, chr_len)
 * and of the gene name (gene_beg, gene_len) with the 64-bit FNV-1a hash of each span, start and end; *n_rows of them;
 * *n_lines, the number of lines of buf.  On malformed input the call still returns DN_OK: *err_kind is the DN_GTF_E_*
 * of the first offending line, *err_line its number, and no rows come back.  copy_ms / device_ms (nullable): the copy of
 * buf to the device and the kernels, by HIP events.  Results are bit-identical from run to run.  Text of the last
 * error: dn_gtf_last_error(). */
#define DN_GTF_E_FIELDS   1   /* fewer than nine tab-separated fields                                                   */
#define DN_GTF_E_GENE     2   /* an exon line without a usable gene_name / gene_id                                      */
#define DN_GTF_E_INTEGER  3   /* an exon line whose start or end is not a decimal integer                               */
#define DN_GTF_E_STRAND   4   /* dn_gtf_scan_strand only: an exon line whose seventh field is not one of + - . ?         */
int  dn_gtf_scan(int device, const uint8_t *buf, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                 int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                 int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, int64_t *err_line, int32_t *err_kind,
                 double *copy_ms, double *device_ms);
/* The same with the strand column (strand-specific counting, above): strand[r] is field seven of the exon line of row r, one
 * of '+', '-', '.', '?', read from the line itself while the window is resident.  A kept line whose seventh field is anything
 * else is DN_GTF_E_STRAND, under the same first-error rule.  dn_gtf_scan checks nothing about field seven. */
int  dn_gtf_scan_strand(int device, const uint8_t *buf, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                        int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                        int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *strand, int64_t *err_line,
                        int32_t *err_kind, double *copy_ms, double *device_ms);
const char *dn_gtf_last_error(void);               /* = dn_last_error() */

/* SAM text to BAM records (csrc/dn_sam.hip; degnorm_amd.bam.sam_records, sam_to_bam) -----------------------------------------
 * What `samtools view -b` is run for: the alignment lines of a SAM file become BAM records, in input order.  text holds the
 * n_bytes (1 .. 2^30) of a window of alignment lines -- no '@' header lines -- that ends at a line end.  A line ends at
 * '\n' (a '\r' before it belongs to the line end) or at the end of the bytes; every line is one record, and an empty line
 * is an error.  The references are the @SQ names of the header, handed over sorted by the 64-bit FNV-1a hash of the name:
 * entry k has hash ref_hash[k] (ascending), refID ref_id[k] and the name names[ref_name_beg[k] .. + ref_name_len[k]).  The
 * encoder hashes RNAME / RNEXT, searches the table and compares the bytes of every entry of that hash.
 *
 * The encoding.  A line is 11 mandatory fields and any number of optional ones, separated by single tabs:
 *   QNAME   1 .. 254 bytes -> read_name with its NUL, l_read_name = length + 1.
 *   FLAG    0 .. 65535.     MAPQ  0 .. 255.
 *   RNAME   refID = the @SQ ordinal of the name; `*` is -1; a name the table does not have is an error.
 *   POS     0 .. 2^31 - 1; pos = POS - 1, so POS 0 gives -1.        PNEXT  the same -> next_pos.
 *   CIGAR   `*` is 0 ops; else <length><op> groups, op in MIDNSHP=X (codes 0 .. 8), length 0 .. 2^28 - 1, each stored as
 *           length << 4 | code.  More than 65 535 ops is an error (not supported: no CG tag is written).
 *   RNEXT   `=` is refID, `*` is -1, else as RNAME.                  TLEN   -2^31 .. 2^31 - 1.
 *   SEQ     `*` gives l_seq 0; else one base a byte, code = index in `=ACMGRSVTWYHKDBN` in either letter case, any other
 *           byte 15 (N); two codes a byte, the first in the high nibble, the spare low nibble of an odd length 0.  When
 *           the CIGAR has ops and SEQ is not `*`, the lengths of its M I S = X ops must add up to l_seq.
 *   QUAL    `*` gives l_seq bytes 0xFF; else l_seq bytes in '!' .. '~', each stored minus 33.
 *   bin     the low 16 bits of reg2bin(pos, pos + max(1, sum of the lengths of the M D N = X ops)) of the SAM specification
 *           5.3, with arithmetic shifts on signed values: pos = -1 without CIGAR gives 4680.
 *   Integers are decimal digits, at most 18 of them, with a leading '-' where the range has negative values (and a
 *   leading '+' in optional fields).  The fixed part is block_size, refID, pos, l_read_name, mapq, bin, n_cigar_op, flag,
 *   l_seq, next_refID, next_pos, tlen; then read_name, the ops, the packed bases, the qualities and the optional fields.
 *   Optional fields TAG:TYPE:VALUE -> the two tag bytes, a type byte and the value:
 *     A   one byte.
 *     i   the smallest type that holds the value, unsigned preferred: C up to 255, S up to 65 535, I up to 4 294 967 295;
 *         c down to -128, s down to -32 768, i down to -2 147 483 648; a value outside is an error.
 *     Z   the bytes (none is valid) and a NUL.          H   the same; an odd number of bytes is an error.
 *     B   VALUE is a subtype t of cCsSiIf and then `,value` any number of times -> B, t, the count as int32, the values in
 *         t's width; no value is valid; an integer outside t's range is an error.
 *     f   and the values of B:f: (float) strtod(text) of text that is [+-] followed by inf, infinity, nan in any letter
 *         case or by digits with at most one '.' and an optional exponent; other text is an error.
 *   The size of a float payload does not depend on its value, so the device does not read decimals: the record stream
 *   comes back with those four bytes zero and a patch table of (offset in the stream, offset in text) per payload, and the
 *   host code fills them with strtod before the call returns -- dn_sam_encode_host does the same -- so both builds write
 *   the same bytes.  patch[2 k], patch[2 k + 1] is entry k, in stream order, for callers who want to see it.
 *
 * Passes (device): line starts as in the GTF scan (newlines per 16 KiB tile, scan, scatter); measure, one lane per line
 * (every check above, the record's size and float payloads; the first faulty line in file order wins, by atomicMin);
 * exclusive sums of sizes and payload counts; emit, one lane per line, every record to its offset.  Device memory: the
 * window padded to 16 KiB, the record stream (at most 2 n_bytes + 36 n_lines), 40 bytes a line and 16 a float payload.
 * Outputs: out[0 .. *n_out) the record stream, rec_off[0 .. *n_rec] where every record starts (the last entry = *n_out),
 * *n_lines = *n_rec on success.  out_cap = 2 n_bytes + 36 lines always suffices, rec_cap = lines + 1, patch_cap = entries
 * the patch table can hold; a capacity that is too small is DN_E_INVALID, found after the measure pass and before anything
 * is written.  On a malformed line the call still returns DN_OK: *err_kind is the DN_SAM_E_* of the first faulty line,
 * *err_line its number within text (1-based), and no record comes back.  Within a line the fields are checked in their
 * order, each one whole before the next is looked for, so a line that ends early is DN_SAM_E_FIELDS only when the fields it
 * has are well-formed (a line without any tab is DN_SAM_E_FIELDS whatever it holds).  copy_ms / device_ms (nullable): the copy of text to the device, and the first kernel to the last,
 * by HIP events.
 *   dn_sam_encode_host    the host build of the same source, line after line; no device is touched.
 * Errors: dn_last_error(). */
#define DN_SAM_E_EMPTY      1   /* an empty line                                                                          */
#define DN_SAM_E_FIELDS     2   /* fewer than 11 tab-separated fields                                                     */
#define DN_SAM_E_NAME       3   /* a read name that is empty or longer than 254 bytes                                     */
#define DN_SAM_E_INTEGER    4   /* FLAG, POS, MAPQ, PNEXT or TLEN is not a decimal integer in its range                   */
#define DN_SAM_E_RNAME      5   /* RNAME or RNEXT names a reference the header does not have                              */
#define DN_SAM_E_CIGAR      6   /* a CIGAR that is not <length><op> groups over MIDNSHP=X, or a length above 2^28 - 1     */
#define DN_SAM_E_CIGAR_OPS  7   /* more than 65 535 CIGAR operations: not supported                                       */
#define DN_SAM_E_SEQ        8   /* an empty SEQ field                                                                     */
#define DN_SAM_E_SEQ_CIGAR  9   /* the CIGAR's query length is not the length of SEQ                                      */
#define DN_SAM_E_QUAL_LEN  10   /* QUAL is neither `*` nor as long as SEQ                                                 */
#define DN_SAM_E_QUAL      11   /* a QUAL byte outside '!' .. '~'                                                         */
#define DN_SAM_E_TAG       12   /* an optional field that is not TAG:TYPE:VALUE with a known type and a well-formed value */
#define DN_SAM_E_TAG_RANGE 13   /* an `i` value outside -2 147 483 648 .. 4 294 967 295                                   */
#define DN_SAM_E_TAG_ARRAY 14   /* a B value outside the range of its subtype                                             */
#define DN_SAM_E_TAG_HEX   15   /* an H value with an odd number of bytes                                                 */
#define DN_SAM_E_TAG_FLOAT 16   /* an `f` or B:f value that is not a decimal number                                       */
int  dn_sam_encode(int device, const uint8_t *text, int64_t n_bytes, int32_t n_ref, const uint64_t *ref_hash, const int32_t *ref_id,
                   const int64_t *ref_name_beg, const int32_t *ref_name_len, const uint8_t *names, int64_t n_names, uint8_t *out,
                   int64_t out_cap, int64_t *rec_off, int64_t rec_cap, int64_t *patch, int64_t patch_cap, int64_t *n_lines,
                   int64_t *n_rec, int64_t *n_out, int64_t *n_patch, int64_t *err_line, int32_t *err_kind, double *copy_ms,
                   double *device_ms);
int  dn_sam_encode_host(const uint8_t *text, int64_t n_bytes, int32_t n_ref, const uint64_t *ref_hash, const int32_t *ref_id,
                        const int64_t *ref_name_beg, const int32_t *ref_name_len, const uint8_t *names, int64_t n_names, uint8_t *out,
                        int64_t out_cap, int64_t *rec_off, int64_t rec_cap, int64_t *patch, int64_t patch_cap, int64_t *n_lines,
                        int64_t *n_rec, int64_t *n_out, int64_t *n_patch, int64_t *err_line, int32_t *err_kind);

/* GFF3 annotation scan (csrc/dn_gff3.hip, csrc/dn_gff3.hpp; Gff3AnnotationLoader and gff3_scan, degnorm_amd/loaders.py) ---------
 * The exon table of a GFF3 file: the GTF scan's output for the other annotation format.  In GFF3 an exon line may carry only
 * `Parent=transcript:...`, the transcript line `Parent=gene:...`, and only the gene line the name: the gene of an exon is the
 * result of a join over the whole file, with parents and children any distance apart and in either order.
 *
 * Lines, as in the GTF scan.  A line ends at '\n' or at the end of the bytes; a trailing '\r' is dropped.  Empty lines and
 * lines whose first byte is '#' are skipped (`##gff-version 3`, `###`).  A line that is exactly `##FASTA` ends the annotation:
 * that line and every line after it are ignored, with any error they would raise.  Every other line must hold at least eight
 * tabs (DN_GFF3_E_FIELDS).
 * Attributes: field nine, up to a further tab or the line's end.  It is split at ';', ASCII spaces are stripped from each
 * piece, each piece is split at its first '=' into tag and value (a piece without '=' is a tag with an empty value), and
 * spaces are stripped from both.  Tags compare exactly and case-sensitively (`gene` is not `gene_id`); the first piece with a
 * tag wins, whether its value is empty or not.  Values are the file's bytes: there is NO percent-decoding (`%3B` stays `%3B`).
 * `Parent` may be a comma-separated list: its first element, spaces stripped, is used, and an empty one counts as no Parent.
 * Kinds of line.  An exon line has `exon` as its third field in any letter case; its fourth and fifth fields must be 1 .. 18
 * decimal digits (DN_GFF3_E_INTEGER).  A node is any other line with a non-empty `ID`; it records its ID, its first parent or
 * none, gname = the first non-empty of `gene_name` and `gene`, and rname = the first non-empty of `Name`, `gene_id` and the
 * ID.  When several lines share an ID (legal for discontinuous features), the first in file order is the node.
 * The gene of an exon line:
 *   1  its own first non-empty of `gene_name` and `gene` (GENCODE and RefSeq files end here);
 *   2  otherwise, with a Parent, the node of that ID is looked up, and at each node: gname if it has one; otherwise rname
 *      if the node has no parent; otherwise on to the node's parent.  An ID no node has is DN_GFF3_E_PARENT; more than 8
 *      lookups are DN_GFF3_E_DEPTH (which also ends cycles); both are reported at the exon's line;
 *   3  otherwise, without a Parent, its own non-empty `gene_id`; failing that DN_GFF3_E_GENE.
 * Errors.  Errors of a line itself (FIELDS, INTEGER, GENE) win over link errors (PARENT, DEPTH); within each class the
 * smallest line number wins.  Neither the rows nor the error depend on how the file is cut into windows.
 *
 * One load.  dn_gff3_open checks the need (about 1.5 times the file and 64 MiB) against the free device memory before
 * anything is uploaded -- a file that does not fit is DN_E_INVALID with a message -- and allocates one zeroed buffer of
 * total_bytes padded to whole 16 KiB tiles, where the text stays until dn_gff3_close.  hash_bits (1 .. 64, normally 64) masks
 * the hashes of IDs and Parents to that many bits, in both builds: a way for tests to fill the runs of equal hashes.
 * dn_gff3_window takes the next n_bytes (1 .. 2^30) of the file, which end at a line end (only the last window may end without
 * one): upload to their place, line starts (the GTF scan's three passes over the tiles the window touches), one lane per
 * line (classify, parse, 64-bit FNV-1a hashes; first error and first `##FASTA` line by atomicMin), and two compactions in file
 * order.  The exon rows come back as in dn_gtf_scan, with `line` 1-based in the file and spans as offsets in the file:
 * pending[r] = 0, gene_* is the gene's name; pending[r] = 1, gene_* is the Parent to resolve and gene_hash its masked hash.
 * Node rows stay on the device.  *fasta_line: the line of `##FASTA` when the window held it (0: not), after which no further
 * window is taken.  On a malformed line the call returns DN_OK with *err_kind / *err_line (in the file) and no rows.
 * dn_gff3_resolve takes the pending rows of all windows (line, Parent span and hash as dn_gff3_window gave them; spans outside
 * the bytes uploaded are DN_E_INVALID): the node rows are sorted as (ID hash, ordinal) by a stable radix sort, and one lane
 * per row walks: per lookup a lower-bound search on the hash, then a scan of that hash's run for the first node whose ID has
 * the wanted length and bytes -- two IDs that share a hash stay apart, nothing is decided by a hash alone.  It returns the
 * span and the full hash of every row's gene name, *n_nodes, or the first link error.  Every byte read lies below its
 * line's end, the walk stops after 8 lookups and the run scan at the run's end: malformed input gives a status, nothing else.
 *   dn_gff3_scan_host    the host build of the same source on a whole buffer, line after line, names resolved (row_cap:
 *                        n_bytes / 20 + 1 suffices); *n_walked = the rows that named a Parent.  No device is touched.
 * copy_ms / device_ms / resolve_ms (nullable): by HIP events.  Results are bit-identical from run to run.  Errors: dn_last_error(). */
#define DN_GFF3_E_FIELDS   1   /* fewer than nine tab-separated fields                                                   */
#define DN_GFF3_E_GENE     2   /* an exon line without gene_name, gene, Parent or gene_id                                */
#define DN_GFF3_E_INTEGER  3   /* an exon line whose start or end is not a decimal integer                               */
#define DN_GFF3_E_PARENT   4   /* an exon line whose chain of parents names an ID that no line has                       */
#define DN_GFF3_E_DEPTH    5   /* an exon line whose chain of parents takes more than 8 lookups                          */
#define DN_GFF3_E_STRAND   6   /* the _strand entries only: an exon line whose seventh field is not one of + - . ?       */
typedef struct dn_gff3_ *dn_gff3;
int  dn_gff3_open(int device, int64_t total_bytes, int32_t hash_bits, dn_gff3 *out);
int  dn_gff3_window(dn_gff3 h, const uint8_t *bytes, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                    int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                    int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *pending, int64_t *fasta_line,
                    int64_t *err_line, int32_t *err_kind, double *copy_ms, double *device_ms);
int  dn_gff3_resolve(dn_gff3 h, int64_t n, const int64_t *line, const int64_t *par_beg, const int32_t *par_len, const uint64_t *par_hash,
                     int64_t *name_beg, int32_t *name_len, uint64_t *name_hash, int64_t *n_nodes, int64_t *err_line, int32_t *err_kind,
                     double *resolve_ms);
int  dn_gff3_close(dn_gff3 h);
int  dn_gff3_scan_host(const uint8_t *data, int64_t n_bytes, int32_t hash_bits, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                       int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                       int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, int64_t *n_nodes, int64_t *n_walked, int64_t *err_line,
                       int32_t *err_kind);
/* The same two with the strand column (strand-specific counting, above): strand[r] is field seven of the exon line of row r
 * -- of the exon line itself, not of its gene's line -- one of '+', '-', '.', '?'.  An exon line above ##FASTA whose seventh
 * field is anything else is DN_GFF3_E_STRAND, an error of the line itself.  The entries without it check nothing about it. */
int  dn_gff3_window_strand(dn_gff3 h, const uint8_t *bytes, int64_t n_bytes, int64_t row_cap, int64_t *n_lines, int64_t *n_rows,
                           int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start, int64_t *end,
                           int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *pending, uint8_t *strand,
                           int64_t *fasta_line, int64_t *err_line, int32_t *err_kind, double *copy_ms, double *device_ms);
int  dn_gff3_scan_host_strand(const uint8_t *data, int64_t n_bytes, int32_t hash_bits, int64_t row_cap, int64_t *n_lines,
                              int64_t *n_rows, int64_t *line, int64_t *chr_beg, int32_t *chr_len, uint64_t *chr_hash, int64_t *start,
                              int64_t *end, int64_t *gene_beg, int32_t *gene_len, uint64_t *gene_hash, uint8_t *strand,
                              int64_t *n_nodes, int64_t *n_walked, int64_t *err_line, int32_t *err_kind);

/* Coverage matrices to text (csrc/dn_text.hip, csrc/dn_text.hpp; degnorm_amd.data_access.get_coverage_data, cov_text) ----------
 * What `DataFrame(cov.T).to_csv(file, index=None, sep=' ', float_format='%.5f')` writes below its header line, for a batch of
 * genes.  x holds n_x doubles; gene g is the p x len[g] row-major (sample-major) matrix at x + beg[g], as it lies in the
 * pickles of an output directory.  Its piece of the text has len[g] lines, line j is x[0][j] x[1][j] ... x[p-1][j] -- so the
 * call also transposes -- every value as '%.5f', values separated by single spaces, every line ended by '\n'.
 *
 * The rule, exact for every finite double with |x| < 2^63:
 *   1  x is split into sign, 53-bit significand m and exponent e, |x| = m 2^e; a subnormal has e = -1074 and no hidden bit.
 *   2  |x| 10^5 = (m 3125) 2^(e + 5), and m 3125 < 2^65 fits two 64-bit words.
 *   3  For e + 5 >= 0 that integer, shifted left, is the result.
 *   4  Otherwise it is shifted right by -(e + 5) -- the quotient is 0 for shifts of 66 and more -- and the bits shifted out
 *      are compared with one half: round half to even.
 *   5  The result q is printed as q / 100000, a point, and q % 100000 on five digits, with '-' in front when the sign bit is
 *      set: -0.0 and -1e-9 both give -0.00000, as C does.
 *   6  The code splits off the integer part of |x| first and scales only the fraction, so that everything but the product
 *      stays in 64 bits (10^5 is even, so the fraction's q decides a tie, and a fraction that rounds up to 100000 carries
 *      into the integer part).  Decimal digits come from divisions by constants, 32-bit ones below 10^9.
 * A gene that holds a NaN, an infinity or a value with |x| >= 2^63 is not formatted: flag[g] = 1 and its piece is empty
 * (pandas prints NaN as an empty field with quoting of its own; get_coverage_data writes such genes through pandas).
 *
 * Passes (device): the matrices are uploaded once; measure, one lane per line (the line's width, its gene by a search in
 * the running sum of the lengths, the gene's flag); an exclusive sum over the n_lines + 1 widths, read as 0 for the lines
 * of flagged genes; emit, one wavefront per 64 consecutive lines, whose text is one contiguous run: the lanes write their
 * lines into an 8 KiB LDS chunk that stands for a 16-byte-aligned stretch of the output -- a run longer than that takes
 * several trips, a value across a chunk's end is formatted on both sides -- and the wavefront copies the chunk out in
 * 16-byte pieces, with byte stores only at the run's two ends.  Both walks are one routine with and without stores
 * (dn::text::walk_line), so the second writes what the first measured, and no store leaves the measured size.  The text
 * comes back into pinned memory of exactly the scanned size, owned by *text.
 * Outputs: text_off[0 .. n_genes] where every gene's piece starts in the text (the last entry = dn_text_size), flag[0 ..
 * n_genes), *text.  dn_text_bytes / dn_text_size give the text, dn_text_free releases it (null: nothing happens).
 * Refused with DN_E_INVALID before any work: a null pointer, p < 2 or p > 4096, n_x < 1, n_genes < 1, a negative length, a
 * gene that leaves x, two genes that overlap, more than 2^30 lines, and (dn_cov_text) a device index out of range.
 * ms (nullable, 5 doubles, by HIP events): upload, measure, scan, emit, copy back.
 *   dn_cov_text_host    the host build of the same source, line after line, into plain memory; no device is touched.
 * Results are the same bytes from run to run and in both builds.  Errors: dn_last_error(). */
typedef struct dn_text_ *dn_text;
int  dn_cov_text(int device, const double *x, int64_t n_x, int64_t n_genes, int32_t p, const int64_t *beg, const int64_t *len,
                 int64_t *text_off, uint8_t *flag, dn_text *text, double *ms);
int  dn_cov_text_host(const double *x, int64_t n_x, int64_t n_genes, int32_t p, const int64_t *beg, const int64_t *len,
                      int64_t *text_off, uint8_t *flag, dn_text *text);
const uint8_t *dn_text_bytes(dn_text text);
int64_t dn_text_size(dn_text text);
void dn_text_free(dn_text text);

/* gzip streams (csrc/dn_gz.hip, csrc/dn_gz.hpp; degnorm_amd/gz.py) ---------------------------------------------------------------
 * The inflated bytes of a .gz file (RFC 1952 around RFC 1951), chunk-parallel: what `*.gtf.gz`, `*.gff3.gz` and `*.sam.gz` need
 * before the scans can read them.  A gzip member is one DEFLATE stream whose 32 KiB history runs through the whole member, so it
 * does not inflate block by block as BGZF does.  It is inflated chunk by chunk, by guess, walk, stitch and fix-up (the scheme
 * of dn_frame.hip): an entry is guessed per chunk, every chunk is decoded from its guess without its history, the unknown
 * bytes tracked as 16-bit markers; the host stitches the chain from the true start and walks again only where a guess was
 * wrong; the windows are propagated in chain order; every segment is decoded for real with its window preloaded.
 *
 * Bits.  Byte p of the file holds bits 8 p .. 8 p + 7, least significant first, as RFC 1951 packs them.
 * Container.  A member starts with the magic 1f 8b, CM = 8 and a FLG byte whose bits 5 .. 7 are zero; MTIME, XFL and OS are
 * ignored.  FEXTRA, FNAME, FCOMMENT and FHCRC are skipped; the FHCRC value (the low 16 bits of the CRC32 of the header bytes
 * before it) is compared when `verify` is on.  The DEFLATE stream follows the header; the trailer (CRC32, ISIZE, little endian)
 * starts at the first byte boundary at or behind the final block's end.  ISIZE is always compared with the member's length mod
 * 2^32, the CRC32 when `verify` is on, the CRC32 first.  Any number of members follow each other, an empty one is legal, and
 * no bytes at all are no members.  Behind a member zero bytes are skipped; what follows them is the next member when it starts
 * with the magic and `trailing garbage` otherwise.  (A BGZF file -- the first member carries the BC extra subfield -- is a gzip
 * file too and inflates here, but degnorm_amd.gz sends it down the BGZF path, block by block.)
 * Chunks.  The compressed bytes are cut on an absolute grid of chunk_bytes = C (a power of two, 4 KiB .. 16 MiB; degnorm_amd.gz takes 16 KiB):
 * chunk c is bytes [c C, (c + 1) C), the last one ends with the file.  The guess of chunk c is the smallest bit offset b of
 * the chunk's bits [8 c C, min(8 (c + 1) C, 8 n)) that passes the guess rule, or none (-1).
 * The guess rule at bit b, all of:
 *   1  BFINAL = 0 and BTYPE = 2 (the three bits at b are 0, 0, 1), HLIT <= 29, HDIST <= 29;
 *   2  the HCLEN + 4 code-length code lengths are complete: the sum of 2^-len over the non-zero ones is exactly 1;
 *   3  the HLIT + 257 + HDIST + 1 code lengths decode: every code exists, a repeat of the previous length (16) is not the
 *      first symbol, no repeat leaves the count, nothing reads beyond the file; symbol 256 has a code.  (A 16 behind a run
 *      of zeros written by 17 or 18 repeats zero.)
 *   4  the literal/length code is complete (sum exactly 1); the distance code is complete, or has no code at all, or has one
 *      code of one bit;
 *   5  the block's symbols decode to the end-of-block symbol: every code exists, no length symbol 286 or 287, no distance
 *      symbol 30 or 31, nothing reads beyond the file.  Distances are not compared with anything: the history is unknown;
 *   6  the three bits behind the end-of-block code lie inside the file and are not BTYPE = 3.
 * Stored and fixed blocks are never guessed (the chain reaches them), and a guess may be wrong: a rule, not the truth.
 * Segments.  A true entry is the first bit of a block on the chain that starts at the first block of a member.  The stitch
 * is at a true entry e in chunk c = e / 8 C, at first that of the first member's first block:
 *   - if e is the guess of c, the chunk is confirmed: its segment runs along the block chain to the first block end at or
 *     beyond the chunk's end 8 (c + 1) C, or to the end of a final block if that comes first;
 *   - otherwise the segment is a fix-up: it is walked from e and ends at the first block end y that is the guess of the
 *     chunk y lies in (whichever chunk that is, c included), or at the end of a final block if that comes first.  A run of
 *     wrong or missing guesses is one walk.
 * The segment's exit is the next entry; behind a final block (exit kind DN_GZ_EXIT_MEMBER, else DN_GZ_EXIT_BLOCK) the trailer
 * is read, then padding and the next header, and the next entry is the first bit behind that header.  The chunks strictly
 * between an entry's chunk and its exit's chunk are jumped over: their guesses and walks contribute nothing.  The output is
 * the serial decoder's for every input, whatever the guesses were; guesses only decide the cost.
 * Markers.  A walk keeps the last 32 768 output symbols as uint16: a literal is 0 .. 255, 0x8000 | j is "byte j of the 32 768
 * that precede the entry" (j = 32 767 is the byte just before it).  The ring starts as the identity, ring[j] = 0x8000 | j, so a
 * back-reference is one read of the ring, and a segment shorter than 32 KiB passes the older window through.  A walk leaves
 * its exit bit, its output length (int64), its exit kind, its number of blocks and the ring in order (tail, 32 768 symbols).
 * Windows, in chain order: win[s + 1][j] = tail[s][j] < 256 ? tail[s][j] : win[s][tail[s][j] & 0x7fff]; at a member's first
 * segment the window is all zero.  have[s] = min(32 768, the member's output before s).
 * Emit.  Every segment is decoded again by the byte decoder with win[s] preloaded, from its entry to its exit, to its place
 * (the exclusive sum of the output lengths).  A distance beyond out_pos + have[s] is DN_INFLATE_E_DISTANCE; a length other
 * than the walk's is DN_INFLATE_E_SIZE; the other statuses are those of the BGZF decoder.  The segment's CRC register starts
 * from zero; the host joins the registers in order (reg = reg x^(8 len) + seg, dn_crc.hpp) and compares at the trailer.
 * Spans.  The file is taken in spans of about window_bytes compressed bytes (default 64 MiB, at least one chunk), each starting
 * at the chunk of the next entry.  A walk that the span's end cuts is dropped and its entry starts the next span; when no
 * segment of a span ends inside it the span is doubled (up to 1 GiB).  A guess whose trial decode the span's end cuts is none
 * in that span, so the counters and tables are those of the definition above when the file is one span.  Device memory per
 * span: the compressed bytes, 64 KiB + 32 KiB per chunk and fix-up, and the inflated bytes; the need is compared with the free
 * memory before the upload, and a span that does not fit is DN_E_INVALID with the sizes in the message.
 * Errors: DN_E_INVALID, dn_last_error() = `gzip member at byte <offset of the member's magic>: <what>`, where <what> is one
 * of: truncated header | bad magic | compression method <CM> | reserved flag bits set | header CRC mismatch |
 * invalid block header | invalid code lengths | invalid code | distance beyond the start of the member | truncated deflate
 * stream | inflated length disagrees with the walk | truncated trailer | CRC32 mismatch | ISIZE mismatch | trailing garbage
 * (there <offset> is that of the first such byte).  The first error in stream order wins; the text is the same from both
 * builds; neither the bytes nor the errors depend on chunk_bytes or window_bytes.
 *
 * dn_gz_open takes the whole compressed file (comp stays the caller's and must outlive the handle); device >= 0 is the device
 * build, device = -1 the host build of the same source, which touches no device.  emit = 0 decodes nothing for real: the tables
 * only.  dn_gz_next inflates the next span: *out / *n_out are its bytes (owned by the handle, valid until the next call; pinned
 * host memory in the device build), *done = 1 with *n_out = 0 behind the last one.  After an error the handle only closes.
 * Kernels (one wave per chunk or segment, 64 threads): k_gz_guess tests 64 bit offsets a step, one per lane (rules 1 and 2 in
 * registers), and sends the survivors in ascending order through rules 3 .. 6; k_gz_walk is the marker decoder with a 64 KiB
 * uint16 ring in LDS (about 70 KiB a workgroup, two per CU); k_gz_windows is one workgroup that walks the chain; k_gz_emit is
 * the byte decoder with the ring preloaded, CRC and 16-byte stores in its flush.
 * dn_gz_counters: DN_GZ_N_COUNTERS int64 (order below) and 6 doubles, ms by HIP events (0 in the host build): copy, guess,
 * walk (fix-ups included), windows, emit, copy back.  dn_gz_tables: after the last span, the guess of every chunk (absolute
 * bit or -1) and four int64 per segment: entry bit, exit bit, output length, exit kind.  The pointers are the handle's. */
#define DN_GZ_EXIT_BLOCK   0
#define DN_GZ_EXIT_MEMBER  1
#define DN_GZ_N_COUNTERS   10  /* members, chunks, guessed, confirmed, jumped, fixups, segments, blocks, bytes_in, bytes_out */
typedef struct dn_gz_ *dn_gz;
int  dn_gz_open(const uint8_t *comp, int64_t n_comp, int32_t device, int64_t chunk_bytes, int64_t window_bytes, int32_t verify,
                int32_t emit, dn_gz *out);
int  dn_gz_next(dn_gz h, const uint8_t **out, int64_t *n_out, int32_t *done);
int  dn_gz_counters(dn_gz h, int64_t *counters, double *ms);
int  dn_gz_tables(dn_gz h, int64_t *n_chunks, const int64_t **guess, int64_t *n_segments, const int64_t **segments);
void dn_gz_close(dn_gz h);

/* Measurement hooks (bench.py) -------------------------------------------------------------------- */
/* Device time in ms of the most recent dn_baseline_iteration's main kernel, measured with HIP events
 * on the library's own stream; kernel name via dn_main_kernel_name().                               */
double dn_last_kernel_ms(dn_handle h);
const char *dn_main_kernel_name(dn_handle h);
/* The same for the most recent dn_ratio_svd_sums (the initial pass over the whole transcripts).       */
double dn_last_init_ms(dn_handle h);
/* Device time in ms of the row-maxima kernel of the most recent upload (one read of the whole packed coverage).          */
double dn_last_rowmax_ms(dn_handle h);
const char *dn_init_kernel_name(dn_handle h);
/* Genes are run in up to three classes: class 0 = genes longer than dn_split_length() (256-thread workgroups, one per CU),
 * class 1 = the others (128-thread workgroups, two per CU), class 2 = genes of at most dn_tiny_length() bases (one wavefront
 * per gene, two genes per 128-thread workgroup; 0 when the class does not exist for this sample count); one kernel launch
 * per non-empty class and outer iteration, and a second one for a class that receives handed-down genes (dn_handdown). */
int32_t dn_split_length(dn_handle h);
/* The same two boundaries for ANY cohort of p samples before anything is uploaded (they depend on p and on the device's
 * register / LDS capacity, not on the data): what a host needs to deal genes to GPUs by predicted cost so that every GPU gets
 * the same share of every class (the reference deals contiguous equal-count chunks, nmf_mpi.py:605).  0 / 0: one class.   */
int  dn_class_lengths(dn_handle h, int32_t p, int32_t downsample_rate, int32_t *split_len, int32_t *tiny_len);
int32_t dn_tiny_length(dn_handle h);
double dn_class_kernel_ms(dn_handle h, int cls);
/* First launch to last end of the class kernels of the most recent dn_baseline_iteration (they overlap).          */
double dn_last_span_ms(dn_handle h);
const char *dn_class_kernel_name(dn_handle h, int cls);
/* On-chip capacity of a class after an upload, in columns of ONE gene: those held in registers (with the counts packed next to
 * the state; a gene with a count beyond 16 bits keeps more) and those of its LDS tile.  Active columns beyond their sum live in
 * the scratch slot (spill tier).  0 / 0 for an empty class. */
int  dn_class_tier_cols(dn_handle h, int cls, int32_t *reg_cols, int32_t *lds_cols);
/* Hand-down: a gene of class 0 or 1 whose drop loop has shrunk it to at most `cols` active columns -- what the next class keeps in
 * registers and LDS; DN_HANDDOWN_COLS=a,b overrides the two widths -- is parked between two nmf() calls and finished by a second
 * launch of the next class, queued behind the end of the donor's launch (one level per gene).  Off with DN_HANDDOWN=0 at the
 * upload, for a launch with want_estimates or down-sampling, beyond 32 bins, and outside the templated kernels (p > 64, the
 * run-time-p family): *cols is then the width it would use and *parked stays 0.  *parked: genes class `cls` parked in the most
 * recent dn_baseline_iteration.  A handed-down gene's Gram sums are added in another lane order, so its DI agrees with the run
 * without hand-down to rounding (1e-5 relative against the oracle), not to the bit; the trace counters are the same. */
int  dn_handdown(dn_handle h, int cls, int32_t *cols, int32_t *parked);
int  dn_synchronize(dn_handle h);
/* Stream-copy ceiling of this device (GB/s, float4 copy of `bytes` bytes, best of `reps`).          */
double dn_measure_copy_gbps(dn_handle h, int64_t bytes, int reps);
/* Stream-READ ceiling of this device (GB/s: `bytes` bytes read with four 16-byte loads per lane in flight and folded into
 * one number, best of `reps`): what a read-only streaming kernel -- the row maxima, the two passes of the initial DI pass --
 * is measured against, beside the 8 TB/s of the data sheet.                                              */
double dn_measure_read_gbps(dn_handle h, int64_t bytes, int reps);

#ifdef __cplusplus
}
#endif
#endif /* DEGNORM_AMD_H */
