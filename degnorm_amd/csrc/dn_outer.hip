// dn_outer.hip -- the kernels of dn_outer.hpp and their launchers.  Device code and grid shapes only: no handle, no error text.
#include "dn_outer.hpp"
#include "dn_kernels.hpp"       // TRACE_LEN, ST_NO_CONVERGENCE, P_MAX, P_WIDE_MAX

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace dn {
namespace outer {

// Row maxima of the raw coverage, once per upload: max_j fl(x_ij / s_i) = fl((max_j x_ij) / s_i) for s_i > 0, so the
// 0.1 * max(F) threshold of get_high_coverage_idx (nmf.py:66-76) needs these p numbers per gene instead of a scan of
// the whole scaled matrix in every outer iteration (SURVEY 8(d), config-4 regime note).  One workgroup per gene, one wave per
// row at a time.  Round 4: a pure max-reduce has to stream -- a wave keeps FOUR 16-byte loads per lane in flight (4 KiB per wave
// and trip; rows are only 4-byte aligned, so a scalar head brings the wave to a 16-byte boundary first) instead of one dword
// (round 3: 2.77 TB/s on config 4's 27.5 GB).
__device__ __forceinline__ void row_max_acc(float v, float &m, bool &ok)
{
    m = fmaxf(m, v);
    ok = ok && (v >= 0.0f) && (v <= 65535.0f) && (v == truncf(v));
}

__global__ __launch_bounds__(256) void k_row_max(const float *__restrict__ cov, const int64_t *__restrict__ goff,
                                                 const int32_t *__restrict__ glen, float *__restrict__ rowmax,
                                                 int32_t *__restrict__ x16, int n, int p)
{
    __shared__ int ok_w[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int g = blockIdx.x; g < n; g += gridDim.x) {
        const int L = glen[g];
        bool ok = true;                                    // every value a whole number in [0, 65535]: fits 16 bits exactly
        for (int i = w; i < p; i += 4) {
            const float *row = cov + goff[g] + (size_t) i * L;
            float m = row[0];
            const int head = (int) (((16u - (unsigned) ((size_t) row & 15u)) & 15u) >> 2);     // floats up to the next 16-byte boundary
            const int h = head < L ? head : L;
            if (lane < h) row_max_acc(row[lane], m, ok);
            const float4 *q = reinterpret_cast<const float4 *>(row + h);
            const int n4 = (L - h) >> 2;
            int j = lane;
            typedef float vf4 __attribute__((ext_vector_type(4)));
            const vf4 *qv = reinterpret_cast<const vf4 *>(q);
            for (; j + 448 < n4; j += 512) {               // eight independent 16-byte loads per lane in flight, read once: non-temporal
                vf4 v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = __builtin_nontemporal_load(qv + j + 64 * k);
#pragma unroll
                for (int k = 0; k < 8; k++) { row_max_acc(v[k].x, m, ok); row_max_acc(v[k].y, m, ok); row_max_acc(v[k].z, m, ok); row_max_acc(v[k].w, m, ok); }
            }
            for (; j + 192 < n4; j += 256) {               // four
                const float4 a = q[j], b = q[j + 64], c = q[j + 128], d = q[j + 192];
                row_max_acc(a.x, m, ok); row_max_acc(a.y, m, ok); row_max_acc(a.z, m, ok); row_max_acc(a.w, m, ok);
                row_max_acc(b.x, m, ok); row_max_acc(b.y, m, ok); row_max_acc(b.z, m, ok); row_max_acc(b.w, m, ok);
                row_max_acc(c.x, m, ok); row_max_acc(c.y, m, ok); row_max_acc(c.z, m, ok); row_max_acc(c.w, m, ok);
                row_max_acc(d.x, m, ok); row_max_acc(d.y, m, ok); row_max_acc(d.z, m, ok); row_max_acc(d.w, m, ok);
            }
            for (; j < n4; j += 64) {
                const float4 a = q[j];
                row_max_acc(a.x, m, ok); row_max_acc(a.y, m, ok); row_max_acc(a.z, m, ok); row_max_acc(a.w, m, ok);
            }
            const int t0 = h + 4 * n4;                     // scalar tail (< 4 floats)
            if (t0 + lane < L) row_max_acc(row[t0 + lane], m, ok);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if (lane == 0) rowmax[(size_t) g * p + i] = m;
        }
        const int all_ok = __all(ok);
        if (lane == 0) ok_w[w] = all_ok;
        __syncthreads();
        if (threadIdx.x == 0) x16[g] = (ok_w[0] && ok_w[1] && ok_w[2] && ok_w[3]) ? 1 : 0;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// The outer DegNorm update on the device (nmf.py:398-399, :148-158, :575-590; nmf_mpi.py:821-838).  Per outer iteration
// the host needs 3p + 4 numbers, not the n x p DI matrix: one wave per gene, sample 64 q + lane in slot q of the lane.
//   k_outer_partials  clip rho to [0, 0.9]; untouched = (max_i rho == 0); per-sample partial sums
//                     A = sum_touched x_w / (1 - rho), B = sum_untouched x_w, W = sum x_w; counts of untouched / failed /
//                     unconverged genes.  Block partials, then k_outer_reduce adds them in block order (deterministic).
//   k_outer_apply     rho[untouched] = avg_di; x_adj = x_w / (1 - rho); x_w /= norm; ran_baseline_selection[:, iter].
// One family, template <int WR> = samples per lane, instantiated twice: WR = 1 for cohorts of at most 64 samples, WR = 4 for
// wide cohorts (65 <= p <= 256).  The waves of a block, the blocks and the eight running sums of the reduction are combined in
// the same fixed orders in both: nothing depends on timing, and the summation order is part of the results.
// ---------------------------------------------------------------------------------------------------
template <int WR> constexpr int STRIDE = 3 * 64 * WR + 4;    // per block: A[64 WR] B[64 WR] W[64 WR] n_untouched n_failed n_noconv n_flagged
static_assert(64 * 4 == P_WIDE_MAX && PART_DOUBLES == (size_t) BLOCK_CAP * STRIDE<4>, "the partials buffer holds the widest family");

__device__ __forceinline__ double wave_max_d(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const double t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// the block's row of partials: its four waves added as ((w0 + w1) + w2) + w3
template <int WR> __device__ __forceinline__ void store_partials(double (&sm)[4][3][64 * WR], double (&cnt)[4][4], double *__restrict__ part)
{
    for (int t = threadIdx.x; t < 3 * 64 * WR; t += 256) {
        const int k = t / (64 * WR), i = t - k * (64 * WR);
        part[(size_t) blockIdx.x * STRIDE<WR> + t] = ((sm[0][k][i] + sm[1][k][i]) + sm[2][k][i]) + sm[3][k][i];
    }
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        part[(size_t) blockIdx.x * STRIDE<WR> + 3 * 64 * WR + k] = ((cnt[0][k] + cnt[1][k]) + cnt[2][k]) + cnt[3][k];
    }
}

template <int WR>
__global__ __launch_bounds__(256) void k_outer_partials(const double *__restrict__ rho_raw, double *__restrict__ rho_c,
                                                        const double *__restrict__ xw, const int32_t *__restrict__ trace,
                                                        const int32_t *__restrict__ flags, double *__restrict__ part, int n, int p)
{
    __shared__ double sm[4][3][64 * WR];
    __shared__ double cnt[4][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nw = gridDim.x * 4;
    double a[WR], b[WR], ws[WR], nu = 0.0, nf = 0.0, nc = 0.0, nr = 0.0;
#pragma unroll
    for (int q = 0; q < WR; q++) { a[q] = 0.0; b[q] = 0.0; ws[q] = 0.0; }
    for (int g = blockIdx.x * 4 + w; g < n; g += nw) {
        double r[WR], x[WR], rmax = 0.0;
#pragma unroll
        for (int q = 0; q < WR; q++) {
            const int i = 64 * q + lane;
            r[q] = 0.0; x[q] = 0.0;
            if (i < p) {
                double v = rho_raw[(size_t) g * p + i];
                v = v > 0.9 ? 0.9 : v;                                    // nmf.py:398
                v = v < 0.0 ? 0.0 : v;                                    // nmf.py:399
                rho_c[(size_t) g * p + i] = v;
                r[q] = v;
                x[q] = xw[(size_t) g * p + i];
            }
            rmax = r[q] > rmax ? r[q] : rmax;
        }
        const bool untouched = wave_max_d(rmax) == 0.0;                   // nmf.py:155
#pragma unroll
        for (int q = 0; q < WR; q++) {
            a[q] += untouched ? 0.0 : x[q] / (1.0 - r[q]);                // nmf.py:575
            b[q] += untouched ? x[q] : 0.0;
            ws[q] += x[q];
        }
        if (lane == 0) {
            const int st = trace[(size_t) g * dn::TRACE_LEN + 6];
            nu += untouched ? 1.0 : 0.0; nf += st != 0 ? 1.0 : 0.0; nc += st == dn::ST_NO_CONVERGENCE ? 1.0 : 0.0;
            nr += flags[g] != 0 ? 1.0 : 0.0;                              // ran_baseline_selection[:, i].sum() (nmf.py:571)
        }
    }
#pragma unroll
    for (int q = 0; q < WR; q++) { sm[w][0][64 * q + lane] = a[q]; sm[w][1][64 * q + lane] = b[q]; sm[w][2][64 * q + lane] = ws[q]; }
    if (lane == 0) { cnt[w][0] = nu; cnt[w][1] = nf; cnt[w][2] = nc; cnt[w][3] = nr; }
    __syncthreads();
    store_partials<WR>(sm, cnt, part);
}

// The initial normalisation on the device (nmf.py:524-531): rho0 = 1 - cov_sums / (est_sums + 1) per gene, `low` =
// (max_i rho0 < 0.1), per-sample sums of the read counts over the low genes and over all genes, the number of low genes and
// of genes whose initial SVD failed.  Same block-partial layout as k_outer_partials (A = low sums, B = all sums, W unused).
template <int WR>
__global__ __launch_bounds__(256) void k_init_partials(const double *__restrict__ est, const double *__restrict__ cov,
                                                       const int32_t *__restrict__ status, const double *__restrict__ x,
                                                       double *__restrict__ part, int n, int p)
{
    __shared__ double sm[4][3][64 * WR];
    __shared__ double cnt[4][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nw = gridDim.x * 4;
    double a[WR], b[WR], nl = 0.0, nb = 0.0;
#pragma unroll
    for (int q = 0; q < WR; q++) { a[q] = 0.0; b[q] = 0.0; }
    for (int g = blockIdx.x * 4 + w; g < n; g += nw) {
        double xv[WR], rmax = -INFINITY;
#pragma unroll
        for (int q = 0; q < WR; q++) {
            const int i = 64 * q + lane;
            xv[q] = 0.0;
            if (i < p) {
                const double r = 1.0 - cov[(size_t) g * p + i] / (est[(size_t) g * p + i] + 1.0);       // nmf.py:526
                rmax = r > rmax ? r : rmax;
                xv[q] = x[(size_t) g * p + i];
            }
        }
        const bool low = wave_max_d(rmax) < 0.1;                          // nmf.py:529
#pragma unroll
        for (int q = 0; q < WR; q++) { a[q] += low ? xv[q] : 0.0; b[q] += xv[q]; }
        if (lane == 0) { nl += low ? 1.0 : 0.0; nb += status[g] != 0 ? 1.0 : 0.0; }
    }
#pragma unroll
    for (int q = 0; q < WR; q++) { sm[w][0][64 * q + lane] = a[q]; sm[w][1][64 * q + lane] = b[q]; sm[w][2][64 * q + lane] = 0.0; }
    if (lane == 0) { cnt[w][0] = nl; cnt[w][1] = nb; cnt[w][2] = 0.0; cnt[w][3] = 0.0; }
    __syncthreads();
    store_partials<WR>(sm, cnt, part);
}

// x_weighted = x / norm (nmf.py:533)
__global__ __launch_bounds__(256) void k_scale_reads(const double *__restrict__ x, const double *__restrict__ norm,
                                                     double *__restrict__ xw, long long np, int p)
{
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < np; i += (long long) gridDim.x * 256)
        xw[i] = x[i] / norm[i % p];
}

// one thread per entry of the block partials (grid of ceil(STRIDE / 256) blocks; one block at WR = 1)
template <int WR>
__global__ __launch_bounds__(256) void k_outer_reduce(const double *__restrict__ part, double *__restrict__ out, int nblocks, int p)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= STRIDE<WR>) return;
    // eight independent running sums (block b goes to sum b % 8: eight loads in flight instead of a chain of nblocks dependent ones
    // -- 117 us for 512 blocks in round 3), combined in one fixed order: the result does not depend on timing
    double a[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    int b = 0;
    for (; b + 8 <= nblocks; b += 8) {
#pragma unroll
        for (int k = 0; k < 8; k++) a[k] += part[(size_t) (b + k) * STRIDE<WR> + t];
    }
    for (int k = 0; b < nblocks; b++, k++) a[k] += part[(size_t) b * STRIDE<WR> + t];
    const double s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    if (t < 3 * 64 * WR) { const int k = t / (64 * WR), i = t - k * (64 * WR); if (i < p) out[k * p + i] = s; }
    else out[3 * p + (t - 3 * 64 * WR)] = s;
}

template <int WR>
__global__ __launch_bounds__(256) void k_outer_apply(double *__restrict__ rho_c, double *__restrict__ xw, double *__restrict__ xadj,
                                                     const int32_t *__restrict__ flags, uint8_t *__restrict__ ran,
                                                     const double *__restrict__ avg_di, const double *__restrict__ norm,
                                                     int have_avg, int n, int p, int iter, int n_iter)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nw = gridDim.x * 4;
    for (int g = blockIdx.x * 4 + w; g < n; g += nw) {
        double r[WR], rmax = 0.0;
#pragma unroll
        for (int q = 0; q < WR; q++) {
            const int i = 64 * q + lane;
            r[q] = i < p ? rho_c[(size_t) g * p + i] : 0.0;
            rmax = r[q] > rmax ? r[q] : rmax;
        }
        const bool untouched = wave_max_d(rmax) == 0.0;
#pragma unroll
        for (int q = 0; q < WR; q++) {
            const int i = 64 * q + lane;
            if (i < p) {
                double rv = r[q];
                if (untouched && have_avg) rv = avg_di[i];                // correct_di_scores, nmf.py:157
                const double x = xw[(size_t) g * p + i];
                rho_c[(size_t) g * p + i] = rv;
                xadj[(size_t) g * p + i] = x / (1.0 - rv);                // nmf.py:581
                xw[(size_t) g * p + i] = x / norm[i];                     // nmf.py:587
            }
        }
        if (lane == 0 && iter < n_iter) ran[(size_t) g * n_iter + iter] = flags[g] != 0;      // nmf.py:403
    }
}

__global__ __launch_bounds__(256) void k_gather_rows(const double *__restrict__ rho_raw, const int32_t *__restrict__ flags,
                                                     const int64_t *__restrict__ rows, double *__restrict__ out_rho,
                                                     int32_t *__restrict__ out_flags, int n_rows, int p)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * p) return;
    const int k = t / p, i = t - k * p;
    out_rho[t] = rho_raw[(size_t) rows[k] * p + i];
    if (i == 0) out_flags[k] = flags[rows[k]];
}

// the first `cols` counters of every gene, packed: what comes back to the host per iteration when the caller does not want the
// whole trace (dn_set_trace_columns)
__global__ __launch_bounds__(256) void k_trace_head(const int32_t *__restrict__ trace, int32_t *__restrict__ head, long long n_cols_total, int cols)
{
    for (long long t = (long long) blockIdx.x * 256 + threadIdx.x; t < n_cols_total; t += (long long) gridDim.x * 256) {
        const long long g = t / cols;
        head[t] = trace[g * dn::TRACE_LEN + (t - g * cols)];
    }
}

// ---------------------------------------------------------------------------------------------------
// Launchers.  for_width is the one place that picks the instantiation of the outer-update family for a sample count.
// ---------------------------------------------------------------------------------------------------
template <class F> static void for_width(int p, F launch)
{
    if (p <= P_MAX) launch(std::integral_constant<int, 1>());
    else launch(std::integral_constant<int, 4>());          // up to P_WIDE_MAX samples
}

void partials(hipStream_t st, const double *rho_raw, double *rho_c, const double *xw, const int32_t *trace, const int32_t *flags,
              double *part, double *out, int64_t n, int p)
{
    const int blocks = blocks_for(n);
    for_width(p, [&](auto wr) {
        constexpr int WR = decltype(wr)::value;
        hipLaunchKernelGGL(k_outer_partials<WR>, dim3(blocks), dim3(256), 0, st, rho_raw, rho_c, xw, trace, flags, part, (int) n, p);
        hipLaunchKernelGGL(k_outer_reduce<WR>, dim3((STRIDE<WR> + 255) / 256), dim3(256), 0, st, part, out, blocks, p);
    });
}

void init_partials(hipStream_t st, const double *est, const double *cov, const int32_t *status, const double *x,
                   double *part, double *out, int64_t n, int p)
{
    const int blocks = blocks_for(n);
    for_width(p, [&](auto wr) {
        constexpr int WR = decltype(wr)::value;
        hipLaunchKernelGGL(k_init_partials<WR>, dim3(blocks), dim3(256), 0, st, est, cov, status, x, part, (int) n, p);
        hipLaunchKernelGGL(k_outer_reduce<WR>, dim3((STRIDE<WR> + 255) / 256), dim3(256), 0, st, part, out, blocks, p);
    });
}

void apply(hipStream_t st, double *rho_c, double *xw, double *xadj, const int32_t *flags, uint8_t *ran, const double *avg_di,
           const double *norm, bool have_avg, int64_t n, int p, int iter, int n_iter)
{
    for_width(p, [&](auto wr) {
        hipLaunchKernelGGL(k_outer_apply<decltype(wr)::value>, dim3(blocks_for(n)), dim3(256), 0, st, rho_c, xw, xadj, flags, ran, avg_di, norm,
                           have_avg ? 1 : 0, (int) n, p, iter, n_iter);
    });
}

void scale_reads(hipStream_t st, const double *x, const double *norm, double *xw, size_t np, int p)
{
    const int blocks = (int) std::min<size_t>(2048, (np + 255) / 256);
    hipLaunchKernelGGL(k_scale_reads, dim3(blocks), dim3(256), 0, st, x, norm, xw, (long long) np, p);
}

void gather_rows(hipStream_t st, const double *rho_raw, const int32_t *flags, const int64_t *rows, double *out_rho,
                 int32_t *out_flags, int n_rows, int p)
{
    hipLaunchKernelGGL(k_gather_rows, dim3((n_rows * p + 255) / 256), dim3(256), 0, st, rho_raw, flags, rows, out_rho, out_flags, n_rows, p);
}

void trace_head(hipStream_t st, const int32_t *trace, int32_t *head, size_t n_ints, int cols)
{
    const unsigned blocks = (unsigned) std::min<size_t>(1024, (n_ints + 255) / 256);
    hipLaunchKernelGGL(k_trace_head, dim3(blocks), dim3(256), 0, st, trace, head, (long long) n_ints, cols);
}

void row_max(hipStream_t st, const float *cov, const int64_t *goff, const int32_t *glen, float *rowmax, int32_t *x16,
             int64_t n, int p, int n_cus)
{
    const unsigned blocks = (unsigned) std::min<int64_t>(n, (int64_t) n_cus * 8);
    hipLaunchKernelGGL(k_row_max, dim3(blocks), dim3(256), 0, st, cov, goff, glen, rowmax, x16, (int) n, p);
}

}  // namespace outer
}  // namespace dn
