// dn_assemble.hip -- coverage-matrix assembly on the device.
//
// Replaces the densify-and-slice loop of merge_chrom_coverage (reference reads_coverage_merge.py:283-353): per sample
// the chromosome coverage vector arrives as the index / value arrays of its 1 x N CSR row (reads.py:785-786 writes it
// with scipy.sparse.save_npz), is expanded into a dense fp32 vector in HBM, and every gene's exon intervals
// (union of its exons, ascending) are gathered straight into the packed layout the NMF-OA kernels read
// (gene g at p * sum(lengths[:g]), p rows of lengths[g]).  No float64 host dictionary is needed on the way to HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"

namespace {

__global__ __launch_bounds__(256) void k_scatter_csr(const int32_t *__restrict__ idx, const float *__restrict__ val,
                                                     int64_t nnz, float *__restrict__ dense, int64_t n)
{
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < nnz; i += (int64_t) gridDim.x * 256) {
        const int64_t j = idx[i];
        if (j >= 0 && j < n) dense[j] = val[i];
    }
}

// one block per (interval, 1024-column chunk): out[dst + t] = dense[src + t]
__global__ __launch_bounds__(256) void k_gather_intervals(const float *__restrict__ dense, int64_t n,
                                                          const int64_t *__restrict__ c_src, const int64_t *__restrict__ c_dst,
                                                          const int32_t *__restrict__ c_len, float *__restrict__ out)
{
    const int64_t s = c_src[blockIdx.x], d = c_dst[blockIdx.x];
    const int len = c_len[blockIdx.x];
    for (int t = threadIdx.x; t < len; t += 256) {
        const int64_t j = s + t;
        out[d + t] = (j >= 0 && j < n) ? dense[j] : 0.0f;
    }
}

}  // namespace

extern "C" int dn_assemble_coverage(int device, int64_t chrom_len, int32_t p, const int64_t *nnz,
                                    const int32_t *const *indices, const float *const *values,
                                    int64_t n_genes, const int64_t *lengths,
                                    int64_t n_chunks, const int32_t *chunk_gene, const int64_t *chunk_src,
                                    const int64_t *chunk_dst_in_gene, const int32_t *chunk_len,
                                    float *out_packed, double *device_ms)
{
    if (chrom_len <= 0 || p < 1 || n_genes < 1 || !lengths || !out_packed || n_chunks < 0) return dn::fail(DN_E_INVALID, "dn_assemble_coverage: bad argument");
    // The tables are checked before anything reaches the device: a chunk that leaves its gene would be a write outside d_out.
    // (chunk_src needs no check: k_gather_intervals reads zeros outside the chromosome.)
    if (!nnz || !indices || !values) return dn::fail(DN_E_INVALID, "dn_assemble_coverage: null sample table");
    if (n_chunks > 0 && (!chunk_gene || !chunk_src || !chunk_dst_in_gene || !chunk_len)) return dn::fail(DN_E_INVALID, "dn_assemble_coverage: null chunk table");
    for (int i = 0; i < p; i++) {
        if (nnz[i] < 0) return dn::fail(DN_E_INVALID, "dn_assemble_coverage: nnz of sample " + std::to_string(i) + " is negative");
        if (nnz[i] > 0 && (!indices[i] || !values[i])) return dn::fail(DN_E_INVALID, "dn_assemble_coverage: sample " + std::to_string(i) + " has nnz > 0 and a null index or value array");
    }
    for (int64_t g = 0; g < n_genes; g++)
        if (lengths[g] < 0) return dn::fail(DN_E_INVALID, "dn_assemble_coverage: length of gene " + std::to_string(g) + " is negative");
    for (int64_t c = 0; c < n_chunks; c++) {
        const char *bad = (chunk_gene[c] < 0 || chunk_gene[c] >= n_genes)               ? " names a gene outside [0, n_genes)"
                          : chunk_len[c] < 0                                             ? " has a negative length"
                          : chunk_dst_in_gene[c] < 0                                     ? " has a negative destination"
                          : chunk_dst_in_gene[c] > lengths[chunk_gene[c]] - chunk_len[c] ? " ends beyond its gene"
                                                                                         : nullptr;
        if (bad) return dn::fail(DN_E_INVALID, "dn_assemble_coverage: chunk " + std::to_string(c) + bad);
    }
    // absolute destination of every chunk for sample 0; sample i adds i * L_gene
    std::vector<int64_t> goff((size_t) n_genes + 1, 0);
    for (int64_t g = 0; g < n_genes; g++) goff[g + 1] = goff[g] + (int64_t) p * lengths[g];
    const int64_t total = goff[n_genes], chunk_cap = n_chunks > 0 ? n_chunks : 1;
    std::vector<int64_t> cdst((size_t) chunk_cap), cd((size_t) chunk_cap);
    for (int64_t c = 0; c < n_chunks; c++) cdst[c] = goff[chunk_gene[c]] + chunk_dst_in_gene[c];
    int64_t max_nnz = 1;
    for (int i = 0; i < p; i++) if (nnz[i] > max_nnz) max_nnz = nnz[i];

    dn::Stream st;
    dn::Event e0, e1;
    dn::DeviceBuffer<float> d_dense, d_out, d_val;
    dn::DeviceBuffer<int32_t> d_idx, d_clen;
    dn::DeviceBuffer<int64_t> d_csrc, d_cdst;
    DN_TRY(hipSetDevice(device));
    DN_TRY(st.create(hipStreamCreate));
    return dn::synced(st, [&]() -> int {
        DN_TRY(e0.create(hipEventCreate));
        DN_TRY(e1.create(hipEventCreate));
        DN_TRY(d_dense.alloc(sizeof(float) * (size_t) chrom_len));
        DN_TRY(d_out.alloc(sizeof(float) * (size_t) (total > 0 ? total : 1)));
        DN_TRY(d_idx.alloc(sizeof(int32_t) * (size_t) max_nnz));
        DN_TRY(d_val.alloc(sizeof(float) * (size_t) max_nnz));
        DN_TRY(d_csrc.alloc(sizeof(int64_t) * (size_t) (n_chunks > 0 ? n_chunks : 1)));
        DN_TRY(d_cdst.alloc(sizeof(int64_t) * (size_t) (n_chunks > 0 ? n_chunks : 1)));
        DN_TRY(d_clen.alloc(sizeof(int32_t) * (size_t) (n_chunks > 0 ? n_chunks : 1)));
        if (n_chunks > 0) {
            DN_TRY(hipMemcpyAsync(d_csrc, chunk_src, sizeof(int64_t) * (size_t) n_chunks, hipMemcpyHostToDevice, st));
            DN_TRY(hipMemcpyAsync(d_clen, chunk_len, sizeof(int32_t) * (size_t) n_chunks, hipMemcpyHostToDevice, st));
        }
        DN_TRY(hipEventRecord(e0, st));
        for (int i = 0; i < p; i++) {
            // per-sample destinations: row i of every gene (cd is rewritten only after the stream has read it)
            for (int64_t c = 0; c < n_chunks; c++) cd[c] = cdst[c] + (int64_t) i * lengths[chunk_gene[c]];
            hipError_t ee = n_chunks > 0 ? hipMemcpyAsync(d_cdst, cd.data(), sizeof(int64_t) * (size_t) n_chunks, hipMemcpyHostToDevice, st) : hipSuccess;
            if (ee == hipSuccess) ee = hipStreamSynchronize(st);
            DN_TRY(ee);
            DN_TRY(hipMemsetAsync(d_dense, 0, sizeof(float) * (size_t) chrom_len, st));        // missing file: all zeros (reference :309-316)
            if (nnz[i] > 0) {
                DN_TRY(hipMemcpyAsync(d_idx, indices[i], sizeof(int32_t) * (size_t) nnz[i], hipMemcpyHostToDevice, st));
                DN_TRY(hipMemcpyAsync(d_val, values[i], sizeof(float) * (size_t) nnz[i], hipMemcpyHostToDevice, st));
                const int grid = (int) ((nnz[i] + 255) / 256 < 65536 ? (nnz[i] + 255) / 256 : 65536);
                hipLaunchKernelGGL(k_scatter_csr, dim3(grid), dim3(256), 0, st, d_idx, d_val, nnz[i], d_dense, chrom_len);
            }
            if (n_chunks > 0)
                hipLaunchKernelGGL(k_gather_intervals, dim3((unsigned) n_chunks), dim3(256), 0, st, d_dense, chrom_len, d_csrc, d_cdst, d_clen, d_out);
            DN_TRY(hipGetLastError());
        }
        DN_TRY(hipEventRecord(e1, st));
        DN_TRY(hipMemcpyAsync(out_packed, d_out, sizeof(float) * (size_t) total, hipMemcpyDeviceToHost, st));
        DN_TRY(hipStreamSynchronize(st));
        if (device_ms) { float ms = 0.f; DN_TRY(hipEventElapsedTime(&ms, e0, e1)); *device_ms = ms; }
        return DN_OK;
    });
}
