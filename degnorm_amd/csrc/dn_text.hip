// dn_text.hip -- coverage matrices -> the text of their files on the device (data_access.get_coverage_data;
// include/degnorm_amd.h, "Coverage matrices to text", defines the rule and dn_text.hpp holds it, one source for both builds).
//
// A batch of p x L_g float64 matrices goes to the GPU once and comes back as one run of text, gene after gene:
//   1  k_text_measure   one lane per line (a line is one base position: the p values of a column): the width of the line's
//                       text, the gene it belongs to, and the gene's flag when a value is outside the rule
//   2  hipcub::DeviceScan::ExclusiveSum over n_lines + 1 widths -> where every line's text starts; the widths are read
//                       through MaskedWidth, which gives 0 for the lines of a flagged gene, so such a gene's piece is empty
//   3  k_text_emit      one wavefront per 64 consecutive lines, whose text is one contiguous run of the output: the lanes
//                       write their lines into an LDS chunk of kChunk bytes that stands for an aligned stretch of the
//                       output, and the wavefront copies the chunk out in 16-byte pieces, with byte stores only at the
//                       run's two ends; a run longer than the chunk takes several trips
// Lanes own consecutive lines j, so their loads of x[i][j] are coalesced for every sample i.  Every LDS store passes a
// Window inside the chunk and inside the lane's own line; every global store lies inside the run [off[t0], off[t1]), which
// is checked against the size the text buffer was allocated with.
// dn_cov_text_host runs the same two walks line after line into a buffer of exactly the measured size.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_text.hpp"

// the text of one batch: pinned memory (device build) or plain memory (host build) of exactly `size` bytes
struct dn_text_ {
    dn::PinnedBuffer<uint8_t> pinned;
    std::vector<uint8_t> plain;
    int64_t size = 0;
};

namespace {

using dn::text::Window;

constexpr int kNT = 256;                          // k_text_measure
constexpr int kWave = 64;                         // k_text_emit: one wavefront a workgroup
constexpr int kChunk = 8192;                      // bytes of LDS a wavefront builds its run in
constexpr int kMaxP = 4096;                       // a line's width stays far inside 32 bits
constexpr int64_t kNoEnd = INT64_MAX;
constexpr int64_t kMaxLines = (int64_t) 1 << 30;  // of one batch: the scan counts in int

// the gene of line t: the last g with line_base[g] <= t (genes without lines share their successor's base)
__device__ inline int32_t gene_of(const int64_t *__restrict__ line_base, int32_t n_genes, int64_t t)
{
    int32_t lo = 0, hi = n_genes;                 // line_base[lo] <= t < line_base[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (line_base[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// width[t], gene[t] for t < n_lines, and width 0 in entry n_lines, which makes the exclusive sum end with the total
__global__ __launch_bounds__(kNT) void k_text_measure(const double *__restrict__ x, int32_t p, int32_t n_genes, const int64_t *__restrict__ beg,
                                                       const int64_t *__restrict__ len, const int64_t *__restrict__ line_base, int64_t n_lines,
                                                       int32_t *__restrict__ width, int32_t *__restrict__ gene, uint32_t *__restrict__ flag)
{
    const int64_t t = (int64_t) blockIdx.x * kNT + threadIdx.x;
    if (t > n_lines) return;
    if (t == n_lines) {
        width[t] = 0;
        gene[t] = 0;
        return;
    }
    const int32_t g = gene_of(line_base, n_genes, t);
    const int64_t L = len[g];
    int i = 0;
    int64_t at = 0;
    bool bad = false;
    const Window<false> none{nullptr, 0, 0, kNoEnd};
    dn::text::walk_line<false>(x + beg[g] + (t - line_base[g]), L, p, &i, &at, none, &bad);
    if (bad) atomicOr(flag + g, 1u);
    width[t] = (int32_t) at;
    gene[t] = g;
}

// what the scan adds up: the width of line t, 0 for a line of a flagged gene
struct MaskedWidth {
    const int32_t *width, *gene;
    const uint32_t *flag;
    __host__ __device__ int64_t operator()(int64_t t) const { return flag[gene[t]] ? 0 : (int64_t) width[t]; }
};

__global__ __launch_bounds__(kWave) void k_text_emit(const double *__restrict__ x, int32_t p, const int64_t *__restrict__ beg,
                                                      const int64_t *__restrict__ len, const int64_t *__restrict__ line_base, int64_t n_lines,
                                                      const int32_t *__restrict__ gene, const int64_t *__restrict__ off,
                                                      uint8_t *__restrict__ out, int64_t n_out)
{
    __shared__ __attribute__((aligned(16))) uint8_t chunk[kChunk];
    const int lane = threadIdx.x;
    const int64_t t0 = (int64_t) blockIdx.x * kWave;
    if (t0 >= n_lines) return;
    const int64_t t1 = t0 + kWave < n_lines ? t0 + kWave : n_lines, t = t0 + lane;
    const int64_t run_lo = off[t0], run_hi = off[t1];
    if (run_lo < 0 || run_hi < run_lo || run_hi > n_out) return;        // the same for every lane
    // this lane's line: [line_lo, line_hi) of the text; no bytes for a lane without a line or a line of a flagged gene
    int64_t line_lo = run_hi, line_hi = run_hi, L = 0;
    const double *col = x;
    if (t < t1) {
        const int32_t g = gene[t];
        line_lo = off[t];
        line_hi = off[t + 1];
        if (line_lo < run_lo || line_hi < line_lo || line_hi > run_hi) line_lo = line_hi = run_hi;
        L = len[g];
        col = x + beg[g] + (t - line_base[g]);
    }
    int i = 0;
    int64_t at = line_lo;
    bool bad = false;
    // trips over aligned stretches of the output: chunk[k] is the byte at c_lo + k
    for (int64_t c_lo = run_lo & ~(int64_t) 15; c_lo < run_hi; c_lo += kChunk) {
        const int64_t c_hi = c_lo + kChunk;
        const Window<true> w{chunk, c_lo, line_lo > c_lo ? line_lo : c_lo, line_hi < c_hi ? line_hi : c_hi};
        if (w.lo < w.hi) dn::text::walk_line<true>(col, L, p, &i, &at, w, &bad);
        __syncthreads();
        const int64_t lo = run_lo > c_lo ? run_lo : c_lo, hi = run_hi < c_hi ? run_hi : c_hi;
        const int64_t a_lo = (lo + 15) & ~(int64_t) 15, a_hi = hi & ~(int64_t) 15;
        if (a_lo >= a_hi) {
            for (int64_t o = lo + lane; o < hi; o += kWave) out[o] = chunk[o - c_lo];
        } else {
            for (int64_t o = lo + lane; o < a_lo; o += kWave) out[o] = chunk[o - c_lo];
            for (int64_t o = a_lo + 16 * lane; o < a_hi; o += 16 * kWave)
                *reinterpret_cast<uint4 *>(out + o) = *reinterpret_cast<const uint4 *>(chunk + (o - c_lo));
            for (int64_t o = a_hi + lane; o < hi; o += kWave) out[o] = chunk[o - c_lo];
        }
        __syncthreads();
    }
}

// piece[g] = off[line_base[g]] for g <= n_genes: where every gene's piece starts (a gene without lines: where the next line does)
__global__ __launch_bounds__(kNT) void k_text_pieces(const int64_t *__restrict__ off, const int64_t *__restrict__ line_base, int64_t n_genes,
                                                      int64_t *__restrict__ piece)
{
    const int64_t g = (int64_t) blockIdx.x * kNT + threadIdx.x;
    if (g <= n_genes) piece[g] = off[line_base[g]];
}

// what both entries check before any work; *n_lines = the lines of the batch
int check_call(const char *who, const double *x, int64_t n_x, int64_t n_genes, int32_t p, const int64_t *beg, const int64_t *len,
               int64_t *text_off, uint8_t *flag, dn_text *text, int64_t *n_lines)
{
    const std::string w(who);
    if (!x || !beg || !len || !text_off || !flag || !text) return dn::fail(DN_E_INVALID, w + ": null argument");
    *text = nullptr;
    if (p < 2) return dn::fail(DN_E_INVALID, w + ": fewer than 2 samples");
    if (p > kMaxP) return dn::fail(DN_E_INVALID, w + ": more than 4096 samples");
    if (n_x < 1 || n_genes < 1 || n_genes > INT32_MAX - 1) return dn::fail(DN_E_INVALID, w + ": bad argument");
    int64_t lines = 0;
    for (int64_t g = 0; g < n_genes; g++) {
        if (len[g] < 0) return dn::fail(DN_E_INVALID, w + ": gene " + std::to_string(g) + " has a negative length");
        if (beg[g] < 0 || beg[g] > n_x || len[g] > (n_x - beg[g]) / p)
            return dn::fail(DN_E_INVALID, w + ": gene " + std::to_string(g) + " leaves the buffer");
        lines += len[g];
        if (lines > kMaxLines) return dn::fail(DN_E_INVALID, w + ": more than 2^30 lines in one batch");
    }
    std::vector<int64_t> order;
    for (int64_t g = 0; g < n_genes; g++)
        if (len[g] > 0) order.push_back(g);
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return beg[a] < beg[b]; });
    for (size_t k = 1; k < order.size(); k++)
        if (beg[order[k - 1]] + (int64_t) p * len[order[k - 1]] > beg[order[k]])
            return dn::fail(DN_E_INVALID, w + ": genes " + std::to_string(std::min(order[k - 1], order[k])) + " and "
                            + std::to_string(std::max(order[k - 1], order[k])) + " overlap");
    *n_lines = lines;
    return DN_OK;
}

}  // namespace

extern "C" const uint8_t *dn_text_bytes(dn_text t) { return !t ? nullptr : t->pinned.get() ? t->pinned.get() : t->plain.data(); }
extern "C" int64_t dn_text_size(dn_text t) { return t ? t->size : 0; }
extern "C" void dn_text_free(dn_text t) { delete t; }

extern "C" int dn_cov_text_host(const double *x, int64_t n_x, int64_t n_genes, int32_t p, const int64_t *beg, const int64_t *len,
                                int64_t *text_off, uint8_t *flag, dn_text *text)
{
    dn::clear_error();
    int64_t lines = 0;
    const int rc = check_call("dn_cov_text_host", x, n_x, n_genes, p, beg, len, text_off, flag, text, &lines);
    if (rc != DN_OK) return rc;
    // the measure pass: every line's width, every gene's flag
    std::vector<int32_t> width((size_t) lines);
    const Window<false> none{nullptr, 0, 0, kNoEnd};
    int64_t t = 0, total = 0;
    for (int64_t g = 0; g < n_genes; g++) {
        bool bad = false;
        int64_t size = 0;
        for (int64_t j = 0; j < len[g]; j++, t++) {
            int i = 0;
            int64_t at = 0;
            dn::text::walk_line<false>(x + beg[g] + j, len[g], p, &i, &at, none, &bad);
            width[(size_t) t] = (int32_t) at;
            size += at;
        }
        flag[g] = bad ? 1 : 0;
        text_off[g] = total;
        if (!bad) total += size;
    }
    text_off[n_genes] = total;
    dn_text_ *h = new dn_text_;
    h->plain.resize((size_t) total);
    h->size = total;
    // the emit pass: every line through the window that is the line
    t = 0;
    for (int64_t g = 0; g < n_genes; g++) {
        int64_t o = text_off[g];
        for (int64_t j = 0; j < len[g]; j++, t++) {
            if (flag[g]) continue;
            const Window<true> w{h->plain.data(), 0, o, o + width[(size_t) t]};
            int i = 0;
            int64_t at = o;
            bool bad = false;
            dn::text::walk_line<true>(x + beg[g] + j, len[g], p, &i, &at, w, &bad);
            o += width[(size_t) t];
        }
    }
    *text = h;
    return DN_OK;
}

extern "C" int dn_cov_text(int device, const double *x, int64_t n_x, int64_t n_genes, int32_t p, const int64_t *beg, const int64_t *len,
                           int64_t *text_off, uint8_t *flag, dn_text *text, double *ms)
{
    dn::clear_error();
    int64_t lines = 0;
    const int rc = check_call("dn_cov_text", x, n_x, n_genes, p, beg, len, text_off, flag, text, &lines);
    if (rc != DN_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return dn::fail(DN_E_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return dn::fail(DN_E_INVALID, "dn_cov_text: device index out of range");
    std::vector<int64_t> line_base((size_t) n_genes + 1);
    for (int64_t g = 0; g < n_genes; g++) line_base[(size_t) g + 1] = line_base[(size_t) g] + len[g];
    std::vector<uint32_t> flag32((size_t) n_genes);
    std::vector<int64_t> line_off((size_t) n_genes + 1);        // where every gene's piece starts, and the total
    const size_t n_tab = sizeof(int64_t) * (size_t) n_genes;
    // what the stream reads or writes: owned here, so that it outlives the wait of dn::synced
    dn::Stream st;
    dn::Event e[7];                                    // around the five phases; e[6]: the emit launch, behind the allocations
    dn::DeviceBuffer<double> d_x;
    dn::DeviceBuffer<int64_t> d_beg, d_len, d_base, d_off, d_piece;
    dn::DeviceBuffer<int32_t> d_width, d_gene;
    dn::DeviceBuffer<uint32_t> d_flag;
    dn::DeviceBuffer<uint8_t> d_out;
    dn::Scratch scratch;
    dn_text_ *h = new dn_text_;
    int64_t total = 0;
    const int out_rc = [&]() -> int {
        DN_TRY(hipSetDevice(device));
        DN_TRY(st.create(hipStreamCreate));
        return dn::synced(st, [&]() -> int {
            for (auto &ev : e) DN_TRY(ev.create(hipEventCreate));
            DN_TRY(d_x.alloc(sizeof(double) * (size_t) n_x));
            DN_TRY(d_beg.alloc(n_tab));
            DN_TRY(d_len.alloc(n_tab));
            DN_TRY(d_base.alloc(n_tab + sizeof(int64_t)));
            DN_TRY(d_flag.alloc(sizeof(uint32_t) * (size_t) n_genes));
            DN_TRY(d_width.alloc(sizeof(int32_t) * (size_t) (lines + 1)));
            DN_TRY(d_gene.alloc(sizeof(int32_t) * (size_t) (lines + 1)));
            DN_TRY(d_off.alloc(sizeof(int64_t) * (size_t) (lines + 1)));
            DN_TRY(d_piece.alloc(n_tab + sizeof(int64_t)));
            DN_TRY(hipEventRecord(e[0], st));
            DN_TRY(hipMemcpyAsync(d_x, x, sizeof(double) * (size_t) n_x, hipMemcpyHostToDevice, st));
            DN_TRY(hipMemcpyAsync(d_beg, beg, n_tab, hipMemcpyHostToDevice, st));
            DN_TRY(hipMemcpyAsync(d_len, len, n_tab, hipMemcpyHostToDevice, st));
            DN_TRY(hipMemcpyAsync(d_base, line_base.data(), n_tab + sizeof(int64_t), hipMemcpyHostToDevice, st));
            DN_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t) * (size_t) n_genes, st));
            DN_TRY(hipEventRecord(e[1], st));
            hipLaunchKernelGGL(k_text_measure, dim3((unsigned) ((lines + 1 + kNT - 1) / kNT)), dim3(kNT), 0, st, (const double *) d_x.get(), p,
                               (int32_t) n_genes, (const int64_t *) d_beg.get(), (const int64_t *) d_len.get(), (const int64_t *) d_base.get(),
                               lines, d_width.get(), d_gene.get(), d_flag.get());
            DN_TRY(hipGetLastError());
            DN_TRY(hipEventRecord(e[2], st));
            const MaskedWidth masked{d_width.get(), d_gene.get(), d_flag.get()};
            hipcub::TransformInputIterator<int64_t, MaskedWidth, hipcub::CountingInputIterator<int64_t>> widths(
                hipcub::CountingInputIterator<int64_t>(0), masked);
            DN_TRY(scratch.run([&](void *tmp, size_t &bytes) {
                return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, widths, d_off.get(), (int) (lines + 1), st);
            }));
            DN_TRY(hipEventRecord(e[3], st));
            DN_TRY(hipMemcpyAsync(&total, d_off.get() + lines, sizeof(int64_t), hipMemcpyDeviceToHost, st));
            DN_TRY(hipMemcpyAsync(flag32.data(), d_flag, sizeof(uint32_t) * (size_t) n_genes, hipMemcpyDeviceToHost, st));
            DN_TRY(hipStreamSynchronize(st));
            if (total < 0 || total > n_x * (dn::text::kMaxValue + 1))
                return dn::fail(DN_E_STATE, "dn_cov_text: text size out of range");
            DN_TRY(d_out.alloc((size_t) (total > 0 ? total : 1)));
            DN_TRY(h->pinned.alloc((size_t) (total > 0 ? total : 1)));
            h->size = total;
            DN_TRY(hipEventRecord(e[6], st));
            if (lines > 0 && total > 0) {
                hipLaunchKernelGGL(k_text_emit, dim3((unsigned) ((lines + kWave - 1) / kWave)), dim3(kWave), 0, st, (const double *) d_x.get(), p,
                                   (const int64_t *) d_beg.get(), (const int64_t *) d_len.get(), (const int64_t *) d_base.get(), lines,
                                   (const int32_t *) d_gene.get(), (const int64_t *) d_off.get(), d_out.get(), total);
                DN_TRY(hipGetLastError());
            }
            DN_TRY(hipEventRecord(e[4], st));
            if (total > 0) DN_TRY(hipMemcpyAsync(h->pinned.get(), d_out, (size_t) total, hipMemcpyDeviceToHost, st));
            hipLaunchKernelGGL(k_text_pieces, dim3((unsigned) ((n_genes + 1 + kNT - 1) / kNT)), dim3(kNT), 0, st, (const int64_t *) d_off.get(),
                               (const int64_t *) d_base.get(), n_genes, d_piece.get());
            DN_TRY(hipGetLastError());
            DN_TRY(hipMemcpyAsync(line_off.data(), d_piece, n_tab + sizeof(int64_t), hipMemcpyDeviceToHost, st));
            DN_TRY(hipEventRecord(e[5], st));
            DN_TRY(hipStreamSynchronize(st));
            for (int64_t g = 0; g < n_genes; g++)        // the device wrote these: hold them to the buffer before they are used
                if (line_off[(size_t) g] < 0 || line_off[(size_t) g] > line_off[(size_t) g + 1] || line_off[(size_t) g + 1] > total)
                    return dn::fail(DN_E_STATE, "dn_cov_text: text offsets out of order");
            if (ms)
                for (int k = 0; k < 5; k++) {
                    float v = 0.f;
                    DN_TRY(hipEventElapsedTime(&v, e[k == 3 ? 6 : k], e[k + 1]));
                    ms[k] = v;
                }
            return DN_OK;
        });
    }();
    if (out_rc != DN_OK) {
        delete h;
        return out_rc;
    }
    memcpy(text_off, line_off.data(), sizeof(int64_t) * (size_t) (n_genes + 1));
    for (int64_t g = 0; g < n_genes; g++) flag[g] = flag32[(size_t) g] ? 1 : 0;
    *text = h;
    return DN_OK;
}
