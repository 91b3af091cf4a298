// dn_api.hip -- C ABI (include/degnorm_amd.h) over the kernels of dn_kernels.hpp: device handle, host packer,
// resident buffers, launches.  Host side only; the kernels are instantiated per sample count in dn_inst.hip, and the ones this
// unit launches itself (outer update, row maxima, gathers) are in dn_outer.hip behind the launchers of dn_outer.hpp.
#include "dn_kernels.hpp"
#include "dn_host.hpp"
#include "dn_outer.hpp"
#include "../../include/degnorm_amd.h"

#include <dlfcn.h>
#include <rccl/rccl.h>          // types and constants only: the entry points are resolved at run time (rccl_api below)

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

// sample counts with compiled kernels (dn_inst.hip is built once per entry; keep in sync with build.py)
#ifndef DN_P_MAX_TEMPLATED
#define DN_P_MAX_TEMPLATED 64        // templated kernels for 2 .. this many samples (build.py compiles the same list)
#endif
#define DN_P_2_16(X)  X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#define DN_P_17_24(X) X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24)
#define DN_P_25_32(X) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#define DN_P_33_48(X) X(33) X(34) X(35) X(36) X(37) X(38) X(39) X(40) X(41) X(42) X(43) X(44) X(45) X(46) X(47) X(48)
#define DN_P_49_64(X) X(49) X(50) X(51) X(52) X(53) X(54) X(55) X(56) X(57) X(58) X(59) X(60) X(61) X(62) X(63) X(64)
#if DN_P_MAX_TEMPLATED >= 64
#define DN_FOR_EACH_P(X) DN_P_2_16(X) DN_P_17_24(X) DN_P_25_32(X) DN_P_33_48(X) DN_P_49_64(X)
#elif DN_P_MAX_TEMPLATED >= 48
#define DN_FOR_EACH_P(X) DN_P_2_16(X) DN_P_17_24(X) DN_P_25_32(X) DN_P_33_48(X)
#elif DN_P_MAX_TEMPLATED >= 32
#define DN_FOR_EACH_P(X) DN_P_2_16(X) DN_P_17_24(X) DN_P_25_32(X)
#elif DN_P_MAX_TEMPLATED >= 24
#define DN_FOR_EACH_P(X) DN_P_2_16(X) DN_P_17_24(X)
#elif DN_P_MAX_TEMPLATED >= 16
#define DN_FOR_EACH_P(X) DN_P_2_16(X)
#else
#error "DN_P_MAX_TEMPLATED must be 16, 24, 32, 48 or 64"
#endif

namespace dn {
#ifndef DN_WIDE_NT
#define DN_WIDE_NT 256               // threads per workgroup of the wide gene class (build.py compiles this variant)
#endif
#define DN_CAT4_(a, b, c, d) a##b##c##d
#define DN_CAT4(a, b, c, d) DN_CAT4_(a, b, c, d)
#define DN_WIDE_SET(P) DN_CAT4(kernel_set_p, P, _nt, DN_WIDE_NT)
#define DN_DECL(P) const KernelSet *DN_WIDE_SET(P)(); const KernelSet *kernel_set_p##P##_nt128();
DN_FOR_EACH_P(DN_DECL)
#undef DN_DECL

// Pair build (dn_inst.hip -DDN_PAIR): 128-thread workgroups carrying two genes, one per wavefront, for the shortest genes;
// compiled where the register tier exists
#ifndef DN_P_PAIR                 // build.py passes the list it compiles (-D'DN_P_PAIR(X)=X(8) ...'): ONE source of truth
#define DN_P_PAIR(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
#endif
#define DN_DECL(P) const KernelSet *kernel_set_p##P##_pair();
DN_P_PAIR(DN_DECL)
#undef DN_DECL
const KernelSet *kernel_set_pair(int p)
{
    switch (p) {
#define DN_CASE(P) case P: return kernel_set_p##P##_pair();
        DN_P_PAIR(DN_CASE)
#undef DN_CASE
        default: return nullptr;
    }
}

// 128-thread workgroups (two per CU) for the narrow gene class
const KernelSet *kernel_set_narrow(int p)
{
    switch (p) {
#define DN_CASE(P) case P: return kernel_set_p##P##_nt128();
        DN_FOR_EACH_P(DN_CASE)
#undef DN_CASE
        default: return nullptr;
    }
}

const KernelSet *kernel_set_rows();       // dn_generic.hip compiled with DN_GEN_NT=64: one wavefront per gene

const KernelSet *kernel_set_for(int p)
{
    // DN_FORCE_GENERIC=1 routes every supported p through the run-time-p kernels (used by the tests to
    // cross-check the two kernel families on the same inputs)
    const char *force = getenv("DN_FORCE_GENERIC");
    if (force && force[0] == '1' && p >= 2 && p <= P_MAX) return kernel_set_generic();
    switch (p) {
#define DN_CASE(P) case P: return DN_WIDE_SET(P)();
        DN_FOR_EACH_P(DN_CASE)
#undef DN_CASE
        default: return (p > DN_P_MAX_TEMPLATED && p <= P_MAX) ? kernel_set_generic()
                      : (p > P_MAX && p <= P_WIDE_MAX)           ? kernel_set_wide()       // wide cohorts: 65 .. 256 samples
                                                                 : nullptr;
    }
}
}  // namespace dn

// the library's one error text (dn_host.hpp); every dn_*_last_error returns it
static thread_local std::string g_err;

int dn::fail(int code, const std::string &msg) { g_err = msg; return code; }
int dn::fail_hip(const char *what, hipError_t e) { return fail(DN_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
void dn::clear_error() { g_err.clear(); }
const char *dn::last_error() { return g_err.c_str(); }
using dn::fail;

struct dn_handle_s {
    int device = -1;
    int n_cus = 0;
    static constexpr int NCLS = 3;   // gene classes, see GeneClass
    // one stream and one pair of timing events per gene class; stream[0] is also the handle's stream for everything else
    // (declared before `data`, so that the buffers are released first)
    dn::Stream stream[NCLS];
    dn::Event ev_start[NCLS], ev_end[NCLS];
    dn::Event ev_mid[NCLS];          // end of a class's first launch (hand-down: the next class's second launch waits for it)
    dn::Event ev_ready, ev_i0, ev_i1;
    const dn::KernelSet *ks = nullptr;

    int64_t n = 0;
    int32_t p = 0;
    int64_t total = 0;            // floats in the packed coverage
    int32_t lmax = 0;
    std::vector<int64_t> goff;    // n + 1
    std::vector<int32_t> glen;
    std::vector<int64_t> svoff;   // n + 1, in columns

    // Gene classes: [0] wide genes on the main kernel set (256-thread workgroups, one per CU, the whole LDS for one
    // gene), [1] narrow genes (length <= split_len) on 128-thread workgroups, two per CU, so that the serial
    // reduction / eigen-solver phases of one gene overlap the pass of another.  Each class has its own longest-first
    // queue, scratch slots and stream; class 0 is launched first and class 1 fills the CUs as they drain.
    // [2]: the shortest genes (length <= tiny_len), one wavefront per gene, two genes per 128-thread workgroup (the pair
    // build): no cross-wave step, the serial phases are paid by ONE SIMD
    struct GeneClass {
        const dn::KernelSet *ks = nullptr;
        int32_t n = 0;
        int32_t longest = 0;              // longest gene of the class
        // Hand-down (see dn_baseline_iteration): genes of the next wider class, parked between two nmf() calls of their drop loop once
        // they have shrunk to hand_cols columns, are finished by a second launch of this class
        int32_t recv_longest = 0;         // longest gene this class may receive (0: it receives none); its slots hold that too
        int32_t hand_cols = 0;            // THIS class parks a gene at that width: what the next class holds in registers + LDS (0: never)
        dn::DeviceBuffer<int32_t> d_inq;  // continuation queue: gene ids of the donor class, in order of arrival; its length is d_counter[2],
                                          // the head of the second launch d_counter[1]
        int32_t parked = 0;               // genes this class parked in the most recent iteration
        dn::DeviceBuffer<int32_t> d_order;
        std::vector<int32_t> order;       // host copy of the work queue (gene ids)
        dn::DeviceBuffer<int32_t> d_counter;
        dn::DeviceBuffer<char> d_ws;
        int slots = 0;
        int32_t S = 0;
        int64_t slot_bytes = 0;
        int32_t lds_cols = 0;
        size_t dyn_lds = 0;
        float last_ms = 0.f;
    };
    // the buffers and state of one uploaded data set: free_device releases them all at once
    struct DataSet {
        dn::DeviceBuffer<float> d_cov;
        dn::DeviceBuffer<int64_t> d_goff;
        dn::DeviceBuffer<int32_t> d_glen;
        dn::DeviceBuffer<int32_t> d_order;
        dn::DeviceBuffer<int32_t> d_counter;
        dn::DeviceBuffer<int64_t> d_ds;
        dn::DeviceBuffer<double> d_rho;
        dn::DeviceBuffer<int32_t> d_flags;
        dn::DeviceBuffer<int32_t> d_trace;
        dn::DeviceBuffer<double> d_kfin;
        dn::DeviceBuffer<int32_t> d_emode;
        dn::DeviceBuffer<double> d_svec;
        dn::DeviceBuffer<int64_t> d_svoff;
        dn::DeviceBuffer<float> d_rowmax;     // n x p row maxima of the raw coverage (k_row_max at upload)
        dn::PinnedBuffer<int32_t> host_parked;   // per donor class: genes parked in the last iteration
        dn::DeviceBuffer<int32_t> d_hand_int; // hand-down: the continuation records, n x HAND_INTS integers and
        dn::DeviceBuffer<double> d_hand_dbl;  //   n x (5 p + 1) doubles (IterFields)
        dn::DeviceBuffer<int32_t> d_x16;      // n: 1 when every count of the gene is a whole number <= 65535 (packable into 16 bits)
        // outer-update state (dn_outer_begin): clipped / corrected DI, x_weighted, x_adj, ran_baseline_selection, partial sums
        dn::DeviceBuffer<double> d_rhoc, d_xw, d_xadj, d_part, d_pvec;
        dn::DeviceBuffer<double> d_scales;    // wide cohorts: the scale factors and, at P_WIDE_MAX, their reciprocals (the kernels read them through a pointer)
        dn::DeviceBuffer<double> d_x;         // the read counts (n x p), resident for the device-side initial normalisation (dn_init_begin)
        dn::DeviceBuffer<uint8_t> d_ran;
        int32_t n_iter = 0;
        dn::DeviceBuffer<double> d_est_sums, d_cov_sums;
        dn::DeviceBuffer<int32_t> d_status;
        dn::DeviceBuffer<double> d_est;
        dn::DeviceBuffer<int32_t> d_tile_gene, d_tile_col;
        GeneClass cls[NCLS];
        bool have_estimate_state = false;
        // per-gene counters of the previous dn_baseline_iteration: the narrow class orders its queue by the work they predict
        dn::PinnedBuffer<int32_t> host_trace;     // the per-gene counters come back every iteration (n x trace_cols)
        size_t host_trace_len = 0;
        dn::DeviceBuffer<int32_t> d_trace_head;   // n x trace_cols, packed (only when trace_cols < TRACE_LEN)
    } data;
    int64_t n_tiles = 0;
    int32_t split_len = 0, tiny_len = 0;
    double last_scale[dn::P_WIDE_MAX] = {0};     // of the last iteration: est_args reads it for the sets of p <= 64 (the wide set reads d_scales)
    double scales_host[2 * dn::P_WIDE_MAX] = {0};   // what d_scales is filled from: outlives the queued copy
    float last_ms = 0.f;
    float last_span_ms = 0.f;     // first launch to last end of the class kernels of the most recent dn_baseline_iteration
    float last_init_ms = 0.f;     // device time of the most recent dn_ratio_svd_sums kernel
    float last_rowmax_ms = 0.f;   // device time of k_row_max at the most recent upload
    float last_f64_ms = 0.f;      // device time of the most recent dn_nmf_f64 / dn_baseline_selection_f64 kernels
    char init_name[64] = {0};
    // the collective inside the library (dn_comm_*): one RCCL communicator per handle, all-reduces on the handle's stream
    void *comm = nullptr;         // ncclComm_t
    int32_t comm_rank = 0, comm_size = 0;
    dn::DeviceBuffer<double> d_comm;     // DN_COMM_MAX_DOUBLES of scratch (ranks without genes, small host vectors)
    int32_t ds_hint = 1;          // take-every rate the caller intends to use (dn_set_downsample_hint); 1 = none
    int32_t max_steps = dn::EIG_MAX_STEPS_DEFAULT;   // step cap of one eigen-solve (dn_set_solver_step_cap)
    int32_t trace_cols = dn::TRACE_LEN;   // leading trace columns copied back per iteration (dn_set_trace_columns)
    bool have_trace = false;
};

// The exit rule (dn::synced, dn_host.hpp) of the calls that queue on more than the handle's main stream -- the upload and
// dn_baseline_iteration: run `body`, then wait for every class stream.  dn_destroy waits the same way before it deletes.
static void wait_streams(dn_handle h) { for (const dn::Stream &st : h->stream) if (st) (void) hipStreamSynchronize(st); }

template <class F> static int synced_classes(dn_handle h, F body)
{
    const int rc = body();
    wait_streams(h);
    return rc;
}

// the other entry points: on the handle's device, `body` under dn::synced on the main stream
template <class F> static int on_main_stream(dn_handle h, F body)
{
    DN_TRY(hipSetDevice(h->device));
    return dn::synced(h->stream[0], body);
}

// ---------------------------------------------------------------------------------------------------
// RCCL, resolved at run time.  The library carries no link-time dependency on librccl: a host process that already
// has one mapped (PyTorch ships its own copy) must share THAT copy -- two RCCL instances in one process each bring their
// own proxy threads and IPC state --, and a host without any multi-GPU use never loads it.  Order: a copy already in
// the process (RTLD_NOLOAD), DN_RCCL_PATH, the system's librccl.so.1.
// ---------------------------------------------------------------------------------------------------
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int *) = nullptr;
    std::string path;
};

static RcclApi *rccl_api(std::string &err)
{
    static RcclApi api;
    static bool tried = false;
    static std::string load_err;
    if (!tried) {
        tried = true;
        const char *names[] = {"librccl.so.1", "librccl.so"};
        for (const char *n : names) if (!api.lib) { api.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD); if (api.lib) api.path = std::string(n) + " (already in the process)"; }
        if (!api.lib) { const char *e = getenv("DN_RCCL_PATH"); if (e && *e) { api.lib = dlopen(e, RTLD_NOW | RTLD_LOCAL); if (api.lib) api.path = e; } }
        const char *sys[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
        for (const char *n : sys) if (!api.lib) { api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (api.lib) api.path = n; }
        if (!api.lib) {
            const char *why = dlerror();                        // once: the call clears the message
            load_err = std::string("librccl not found (") + (why ? why : "?") + "); set DN_RCCL_PATH";
        } else {
            api.GetUniqueId = (decltype(api.GetUniqueId)) dlsym(api.lib, "ncclGetUniqueId");
            api.CommInitRank = (decltype(api.CommInitRank)) dlsym(api.lib, "ncclCommInitRank");
            api.CommDestroy = (decltype(api.CommDestroy)) dlsym(api.lib, "ncclCommDestroy");
            api.AllReduce = (decltype(api.AllReduce)) dlsym(api.lib, "ncclAllReduce");
            api.GetErrorString = (decltype(api.GetErrorString)) dlsym(api.lib, "ncclGetErrorString");
            api.GetVersion = (decltype(api.GetVersion)) dlsym(api.lib, "ncclGetVersion");
            if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce || !api.GetErrorString) {
                load_err = "librccl (" + api.path + ") lacks an entry point of the nccl API";
                api.lib = nullptr;
            }
        }
    }
    if (!api.lib) { err = load_err; return nullptr; }
    return &api;
}

static void free_device(dn_handle h) { h->data = dn_handle_s::DataSet(); }

// ---------------------------------------------------------------------------------------------------------------
// The float64-input path (dn_generic.hip, DN_GEN_F64 build): per-call device buffers, freed on every return path; the
// handle contributes its device, stream, CU count and solver step cap only.
// ---------------------------------------------------------------------------------------------------------------
namespace {
// a per-call buffer of `count` elements (at least one)
template <class T> hipError_t alloc_f64(dn::DeviceBuffer<T> &b, size_t count) { return b.alloc(sizeof(T) * std::max<size_t>(count, 1)); }

// Persistent workgroups for a float64-path kernel: as many as fit on the device (occupancy x CUs), at most one per item,
// fewer when their scratch slots would take more than a third of free HBM.  0 and g_err set when one slot alone is too big.
int f64_grid(dn_handle h, int which, int64_t items, int64_t slot_bytes)
{
    int per_cu = dn::blocks_per_cu_f64(which);
    if (per_cu < 1) per_cu = 1;
    int64_t grid = std::min<int64_t>(items, (int64_t) per_cu * h->n_cus);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return fail(0, "hipMemGetInfo failed");
    const int64_t budget = (int64_t) (free_b / 3);
    if (slot_bytes > budget) return fail(0, "a matrix is too wide for the device scratch");
    grid = std::max<int64_t>(1, std::min<int64_t>(grid, budget / std::max<int64_t>(slot_bytes, 1)));
    return (int) grid;
}

int check_f64_batch(dn_handle h, int64_t n, int32_t p, const double *const *x, const int64_t *lengths, const char *what)
{
    if (!h) return fail(DN_E_STATE, std::string(what) + ": null handle");
    if (p < 2 || p > dn::P_MAX) return fail(DN_E_UNSUPPORTED, std::string(what) + ": p = " + std::to_string(p) + " outside [2, 64]");
    if (n < 1 || n > INT32_MAX || !x || !lengths) return fail(DN_E_INVALID, std::string(what) + ": bad batch");
    for (int64_t m = 0; m < n; m++) {
        if (!x[m]) return fail(DN_E_INVALID, std::string(what) + ": null matrix");
        if (lengths[m] < 1 || lengths[m] > (1 << 26)) return fail(DN_E_INVALID, std::string(what) + ": matrix length out of [1, 2^26]");
    }
    return DN_OK;
}

// Pack a float64 batch as the device takes it: matrix m (p x lengths[m], row-major) goes to off[m] of `packed`, its columns
// start at col[m] (both n + 1 long, off = p * col), `order` is the work queue, longest first.  Returns the longest length.
// Queued copies read these vectors: the entry point declares them outside its body.
int64_t pack_f64(int64_t n, int32_t p, const double *const *x, const int64_t *lengths, std::vector<int64_t> &off, std::vector<int64_t> &col,
                 std::vector<int32_t> &len, std::vector<int32_t> &order, std::vector<double> &packed)
{
    int64_t longest = 0;
    off.assign(n + 1, 0); col.assign(n + 1, 0); len.resize(n); order.resize(n);
    for (int64_t m = 0; m < n; m++) {
        len[m] = (int32_t) lengths[m];
        col[m + 1] = col[m] + lengths[m];
        off[m + 1] = (int64_t) p * col[m + 1];
        longest = std::max<int64_t>(longest, lengths[m]);
    }
    packed.resize((size_t) off[n]);
    for (int64_t m = 0; m < n; m++) std::memcpy(packed.data() + off[m], x[m], sizeof(double) * (size_t) p * (size_t) lengths[m]);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return len[a] > len[b]; });
    return longest;
}

// estimate tiles of gene g: (gene, first column) per 256 columns
void add_tiles(std::vector<int32_t> &tg, std::vector<int32_t> &tc, int64_t g, int32_t len)
{
    for (int32_t c = 0; c < len; c += 256) { tg.push_back((int32_t) g); tc.push_back(c); }
}

// the dn_params of a baseline iteration and the take-every offsets of its n genes; length(g) is the length of gene g
template <class L> int check_params(const dn_params *prm, const int64_t *ds_start, int64_t n, L length)
{
    if (prm->nmf_iter < 1) return fail(DN_E_INVALID, "nmf_iter must be >= 1");
    if (prm->bins < 1 || prm->bins > dn::MAX_BINS) return fail(DN_E_INVALID, "bins must be in [1, 64]");
    if (prm->min_high_coverage < 2) return fail(DN_E_INVALID, "min_high_coverage must be >= 2 (nmf.py:34)");
    if (prm->downsample_rate < 1) return fail(DN_E_INVALID, "downsample_rate must be >= 1");
    if (prm->downsample_rate > 1) {
        if (!ds_start) return fail(DN_E_INVALID, "downsample_rate > 1 needs per-gene start offsets");
        for (int64_t g = 0; g < n; g++) {
            // nmf.py:443-444 / :479-481: cannot downsample at a rate >= gene length
            if (length(g) <= prm->downsample_rate) return fail(DN_E_INVALID, "downsample_rate is too large; take-every size > at least one gene.");
            if (ds_start[g] < 0 || ds_start[g] >= prm->downsample_rate) return fail(DN_E_INVALID, "ds_start out of [0, rate)");
        }
    }
    return DN_OK;
}
}  // namespace

extern "C" {

#ifndef DN_BUILD_STAMP
#define DN_BUILD_STAMP "unknown build"
#endif
// the library, its target, and the build it is: compiler version and code-generation flags (degnorm_amd/build.py build_stamp).
// Results are bit-reproducible per binary; what may differ between two builds is named here.
const char *dn_version(void) { return "degnorm_amd 0.2.0 (gfx950) [" DN_BUILD_STAMP "]"; }
const char *dn_last_error(void) { return dn::last_error(); }
const char *dn_reads_last_error(void) { return dn::last_error(); }
const char *dn_assemble_last_error(void) { return dn::last_error(); }
const char *dn_gtf_last_error(void) { return dn::last_error(); }

int dn_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dn_p_supported(int p) { return p <= dn::P_MAX && dn::kernel_set_for(p) != nullptr; }
int dn_p_max(void) { return dn::P_WIDE_MAX; }

static int create_streams(dn_handle h)
{
    // The class kernels of a sweep are queued together on three streams and must start in class order: the wide class needs
    // whole CUs, and a CU that a narrow or pair workgroup reaches first is lost to it until that (persistent) workgroup has
    // emptied its queue (seen: the wide kernel then ends LAST, sweep 291 -> 307 ms).  Stream priorities make the dispatcher
    // place pending wide workgroups first, then narrow ones, then pairs.
    int prio_least = 0, prio_greatest = 0;
    DN_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    const int prio[dn_handle_s::NCLS] = {prio_greatest, (prio_least + prio_greatest) / 2, prio_least};
    for (int c = 0; c < dn_handle_s::NCLS; c++) {
        DN_TRY(h->stream[c].create(hipStreamCreateWithPriority, hipStreamNonBlocking, prio[c]));
        DN_TRY(h->ev_start[c].create(hipEventCreate));
        DN_TRY(h->ev_end[c].create(hipEventCreate));
        DN_TRY(h->ev_mid[c].create(hipEventCreateWithFlags, hipEventDisableTiming));
    }
    DN_TRY(h->ev_ready.create(hipEventCreateWithFlags, hipEventDisableTiming));
    DN_TRY(h->ev_i0.create(hipEventCreate));
    DN_TRY(h->ev_i1.create(hipEventCreate));
    return DN_OK;
}

int dn_create(int device, dn_handle *out)
{
    if (!out) return fail(DN_E_INVALID, "dn_create: out is null");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DN_E_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(DN_E_INVALID, "dn_create: device index out of range");
    DN_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    DN_TRY(hipGetDeviceProperties(&prop, device));
    dn_handle h = std::make_unique<dn_handle_s>().release();      // dn_destroy deletes it
    h->device = device;
    h->n_cus = prop.multiProcessorCount;
    const int rc = create_streams(h);
    if (rc != DN_OK) {                       // nothing leaks: dn_destroy releases whatever was created
        const std::string msg = g_err;
        (void) dn_destroy(h);
        return fail(rc, msg);
    }
    *out = h;
    return DN_OK;
}

int dn_destroy(dn_handle h)
{
    if (!h) return DN_OK;
    (void) hipSetDevice(h->device);
    wait_streams(h);
    (void) dn_comm_destroy(h);
    delete h;                                // the owners release the buffers, then the events and streams
    return DN_OK;
}

// Lambda LDS tier of kernel set `ks` at `per_cu` resident workgroups, in columns per gene: whatever of the CU's 160 KiB is
// left per workgroup after the static part, shared by the genes the workgroup carries; a column is p doubles, rounded up to
// an even number (16-byte aligned).  Only the pair build carries more than one gene (units = 2); the wide and narrow sets
// have units = 1, and the narrow boundary of class_lengths, which never divided by units, relies on that.
static int64_t lds_tier_cols(const dn::KernelSet *ks, int per_cu, int32_t p)
{
    const int64_t lds_per_block = (160 * 1024) / per_cu - (int64_t) ks->static_lds_bytes - 256;
    const int64_t ps = p + (p & 1);
    return lds_per_block > 0 ? lds_per_block / std::max(1, ks->units) / (8 * ps) : 0;
}

// Scratch slots and LDS tier of one gene class for genes of up to `cols` active columns.  The new scratch is allocated
// FIRST and swapped in only on success: a failed (re)size leaves the class exactly as it was, still valid.
static int size_class(dn_handle h, dn_handle_s::GeneClass &C, int32_t cols)
{
    const int32_t p = h->p;
    int per_cu = C.ks->blocks_per_cu(0);
    if (per_cu < 1) per_cu = 1;
    const int units = std::max(1, C.ks->units);          // genes a workgroup carries at once: a slot and an LDS tile per unit
    int slots = (int) std::min<int64_t>(((int64_t) C.n + units - 1) / units * units, (int64_t) per_cu * h->n_cus * units);
    const int32_t S = (cols + 63) & ~63;
    // slot: Fs, Fb (fp32, p x S) + x + lambda spill (fp64, ps = p rounded up to even doubles per column: planes of double2) +
    // s_start, residual profile, A^T u (fp64 [S])
    const int64_t slot_bytes = (int64_t) S * ((int64_t) p * 2 * sizeof(float) + (int64_t) (p + (p & 1)) * sizeof(double) + 3 * sizeof(double)) +
                               (int64_t) C.ks->slot_extra_bytes;
    {
        // one very long gene sizes every slot of its class: keep the scratch within a share of free HBM by
        // running fewer persistent workgroups rather than failing (the old scratch, still allocated, counts as free)
        size_t free_b = 0, total_b = 0;
        DN_TRY(hipMemGetInfo(&free_b, &total_b));
        const int64_t budget = (int64_t) ((free_b + (C.d_ws ? (size_t) C.slot_bytes * (size_t) std::max(C.slots, 1) : 0)) / 3);
        if (slot_bytes > budget) return fail(DN_E_INVALID, "a gene is too long for the device scratch (" + std::to_string(S) + " columns)");
        slots = (int) std::max<int64_t>(units, std::min<int64_t>(slots, budget / slot_bytes / units * units));
    }
    dn::DeviceBuffer<char> ws;
    DN_TRY(ws.alloc((size_t) slot_bytes * (size_t) std::max(slots, 1)));
    C.d_ws = std::move(ws);                                // releases the old scratch
    C.slots = slots; C.S = S; C.slot_bytes = slot_bytes;
    const int64_t lcols = std::min<int64_t>(lds_tier_cols(C.ks, per_cu, p), C.S) & ~(int64_t) 1;
    C.lds_cols = (int32_t) lcols;                          // per unit
    C.dyn_lds = (size_t) units * (size_t) lcols * 8 * (size_t) (p + (p & 1));
    return DN_OK;
}

// Where the coverage comes from: already packed host memory (one copy), or a routine that packs the genes [g0, g1) into a
// staging buffer (dn_upload_ragged: float64 dict values -> float32, threads), called chunk by chunk while the previous
// chunk's copy is in flight.
struct CoverageSource {
    const float *packed = nullptr;
    const void *const *genes = nullptr;
    int32_t is_f32 = 0, n_threads = 1;
    std::atomic<int64_t> *bad = nullptr;
};

static void pack_genes(dn_handle h, const CoverageSource &src, int64_t g0, int64_t g1, float *stage)
{
    const int32_t p = h->p;
    const int64_t base = h->goff[g0];
    std::atomic<int64_t> next(g0);
    auto work = [&]() {
        int64_t local_bad = 0;
        for (;;) {
            const int64_t a = next.fetch_add(16);
            if (a >= g1) break;
            const int64_t b = std::min(g1, a + 16);
            for (int64_t g = a; g < b; g++) {
                const int64_t cnt = (int64_t) p * h->glen[g];
                float *dst = stage + (h->goff[g] - base);
                if (src.is_f32) std::memcpy(dst, src.genes[g], sizeof(float) * (size_t) cnt);
                else {
                    const double *s = (const double *) src.genes[g];
                    for (int64_t k = 0; k < cnt; k++) { const float f = (float) s[k]; dst[k] = f; local_bad += ((double) f != s[k]); }
                }
            }
        }
        if (src.bad) *src.bad += local_bad;
    };
    const int nt = (int) std::max<int64_t>(1, std::min<int64_t>(src.n_threads, (g1 - g0 + 15) / 16));
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

// Chunked, double-buffered upload of a ragged data set: two pinned staging buffers of ~128 MB; the host threads pack chunk
// k + 1 while chunk k travels (a single 2 GB pinned buffer cost more to allocate than the whole copy takes).
// The staging pair and the events that tell when each is free again belong to the caller: they outlive its wait for the stream.
static int upload_ragged_chunks(dn_handle h, const CoverageSource &src, dn::PinnedBuffer<float> (&stage)[2], dn::Event (&done)[2])
{
    const int64_t n = h->n;
    int64_t chunk = (int64_t) 32 << 20;                                     // floats per staging buffer
    if (const char *env = getenv("DN_UPLOAD_CHUNK_FLOATS")) chunk = std::max<int64_t>(1, atoll(env));    // tests: many small chunks
    for (int64_t g = 0; g < n; g++) chunk = std::max(chunk, (int64_t) h->p * h->glen[g]);
    chunk = std::min(chunk, std::max<int64_t>(h->total, 1));
    for (int b = 0; b < 2; b++) {
        if (stage[b].alloc(sizeof(float) * (size_t) chunk) != hipSuccess ||
            done[b].create(hipEventCreateWithFlags, hipEventDisableTiming) != hipSuccess) return fail(DN_E_HIP, "upload: pinned staging buffer");
    }
    int64_t g0 = 0;
    for (int k = 0; g0 < n; k++) {
        int64_t g1 = g0, fl = 0;
        while (g1 < n && fl + (int64_t) h->p * h->glen[g1] <= chunk) { fl += (int64_t) h->p * h->glen[g1]; g1++; }
        const int b = k & 1;
        if (k >= 2 && hipEventSynchronize(done[b]) != hipSuccess) return fail(DN_E_HIP, "upload: event");
        pack_genes(h, src, g0, g1, stage[b]);
        if (hipMemcpyAsync(h->data.d_cov + h->goff[g0], stage[b], sizeof(float) * (size_t) fl, hipMemcpyHostToDevice, h->stream[0]) != hipSuccess ||
            hipEventRecord(done[b], h->stream[0]) != hipSuccess) return fail(DN_E_HIP, "upload: copy");
        g0 = g1;
    }
    if (hipStreamSynchronize(h->stream[0]) != hipSuccess) return fail(DN_E_HIP, "upload: synchronize");
    return DN_OK;
}

// Class boundaries of a cohort of p samples served by kernel set `ks` (see dn_handle_s::GeneClass): genes longer than
// split_len run one per CU (wide class), the others two per CU (narrow), those of at most tiny_len bases one wavefront each
// (pair class; `pair` = its kernel set or null).  0 = the class does not exist.  Needs the device (occupancy queries).
static void class_lengths(const dn::KernelSet *ks, int32_t p, int32_t &split_len, int32_t &tiny_len, const dn::KernelSet *&pair)
{
    {
        const char *env = getenv("DN_SPLIT_LEN");
        const dn::KernelSet *narrow = (ks->p != 0) ? dn::kernel_set_narrow(p) : nullptr;
        split_len = 0;
        if (env) split_len = atoi(env);
        else if (narrow) {
            // Narrow class (128-thread workgroups, two genes per CU): its fixed cost per inner iteration (reduce +
            // eigen-solve) is paid by half a CU instead of a whole one, so it wins for every gene it can
            // keep mostly on chip.  On-chip columns of a narrow workgroup = register tier + LDS tier (p = 10: 1 280 + 975);
            // measured optimum of the boundary on config 2: 3 600-4 000 bases, i.e. ~1.7 x that capacity (split 2 600 /
            // 3 000 / 3 400 / 3 800 / 4 200 -> 11 510 / 11 740 / 11 920 / 11 950 / 11 890 genes/s).  Without a register
            // tier: ~2.1 x the LDS columns (round 1: 2 000-2 200 at 975 columns).
            const int64_t lds_cols_n = lds_tier_cols(narrow, std::max(1, narrow->blocks_per_cu(0)), p);
            const int64_t reg_cols_n = narrow->reg_tier_cols;
            // round 3: 1.775 x capacity (4 000 bases at p = 10) instead of 1.7 x (3 831): the same on the full configuration (-0.2 %), but
            // +2.4 % at the shard sizes of 2 and 8 GPUs (10 000 / 2 500 genes: 727 vs 745 ms, 191 vs 196 ms per run) -- with few genes
            // per GPU the wide class (one gene per CU, launched first) is what quantises: 500 instead of 595 genes on 256 slots
            split_len = (int32_t) (reg_cols_n > 0 ? (int64_t) (1.775 * (double) (reg_cols_n + lds_cols_n)) : (int64_t) (2.1 * (double) lds_cols_n));
        }
        if (!narrow) split_len = 0;
        if (!env && p >= 25) split_len = 0;     // wide cohorts (MFMA Gram): one class measured 3-5 % faster than two
        // Pair class: one wavefront per gene pays reduce + eigen-solve on ONE SIMD instead of two and needs no cross-wave step;
        // two such genes share a workgroup of the narrow class's shape.  A wavefront keeps its register tier plus its half of
        // the workgroup's LDS tile on chip (p = 10: 640 + ~480 columns); as for the narrow class the measured optimum of the
        // boundary is ~1.7 x that capacity (config 2, sweep in ms at 900 / 1 120 / 1 300 / 1 500 / 1 700 / 2 000 / 2 300 /
        // 2 600 / 3 000: 300.1 / 298.3 / 295.4 / 293.5 / 292.2 / 291.7 / 293.0 / 296.1 / 304.7; without the class 307.7).
        // DN_TINY_LEN overrides the boundary (0: no such class).
        pair = (ks->p != 0 && split_len > 0) ? dn::kernel_set_pair(p) : nullptr;
        tiny_len = 0;
        if (pair) {
            const char *tenv = getenv("DN_TINY_LEN");
            if (tenv) tiny_len = atoi(tenv);
            else tiny_len = (int32_t) (1.7 * (double) (pair->reg_tier_cols + lds_tier_cols(pair, std::max(1, pair->blocks_per_cu(0)), p)));
            tiny_len = std::min(tiny_len, split_len);
            if (tiny_len <= 0) { pair = nullptr; tiny_len = 0; }
        }
    }
}

// Queue the upload and wait for it.  What the queued copies read -- the work queue, the estimate tiles, the staging pair of a
// ragged upload -- is declared here, outside the body.  A failed upload leaves the handle EMPTY (no resident coverage, later
// calls return DN_E_STATE), never half-sized.
static int finish_upload(dn_handle h, const CoverageSource &src)
{
    std::vector<int32_t> order, tg, tc;
    dn::PinnedBuffer<float> stage[2];
    dn::Event done[2];
    const int rc = synced_classes(h, [&]() -> int {
        const int64_t n = h->n;
        const int32_t p = h->p;
        free_device(h);
        DN_TRY(hipSetDevice(h->device));

        // work queue: longest gene first (a 17-call gene costs ~17x a 1-call gene)
        h->have_trace = false;
        order.resize(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return h->glen[a] > h->glen[b]; });

        h->svoff.assign(n + 1, 0);
        for (int64_t g = 0; g < n; g++) h->svoff[g + 1] = h->svoff[g] + h->glen[g];

        for (int64_t g = 0; g < n; g++) add_tiles(tg, tc, g, h->glen[g]);
        h->n_tiles = (int64_t) tg.size();

        DN_TRY(h->data.d_cov.alloc(sizeof(float) * (size_t) std::max<int64_t>(h->total, 1)));
        DN_TRY(h->data.d_goff.alloc(sizeof(int64_t) * (size_t) (n + 1)));
        DN_TRY(h->data.d_glen.alloc(sizeof(int32_t) * (size_t) n));
        DN_TRY(h->data.d_order.alloc(sizeof(int32_t) * (size_t) n));
        DN_TRY(h->data.d_counter.alloc(sizeof(int32_t) * 4));
        DN_TRY(h->data.d_ds.alloc(sizeof(int64_t) * (size_t) n));
        DN_TRY(h->data.d_rho.alloc(sizeof(double) * (size_t) n * p));
        DN_TRY(h->data.d_flags.alloc(sizeof(int32_t) * (size_t) n));
        DN_TRY(h->data.d_trace.alloc(sizeof(int32_t) * (size_t) n * dn::TRACE_LEN));
        DN_TRY(h->data.d_kfin.alloc(sizeof(double) * (size_t) n * p));
        DN_TRY(h->data.d_emode.alloc(sizeof(int32_t) * (size_t) n));
        DN_TRY(h->data.d_svoff.alloc(sizeof(int64_t) * (size_t) (n + 1)));
        DN_TRY(h->data.d_est_sums.alloc(sizeof(double) * (size_t) n * p));
        DN_TRY(h->data.d_cov_sums.alloc(sizeof(double) * (size_t) n * p));
        DN_TRY(h->data.d_status.alloc(sizeof(int32_t) * (size_t) n));
        DN_TRY(h->data.d_rowmax.alloc(sizeof(float) * (size_t) n * p));
        DN_TRY(h->data.d_x16.alloc(sizeof(int32_t) * (size_t) n));
        if (h->ks->baseline_ptr) DN_TRY(h->data.d_scales.alloc(sizeof(double) * 2 * dn::P_WIDE_MAX));
        DN_TRY(h->data.d_tile_gene.alloc(sizeof(int32_t) * (size_t) std::max<int64_t>(h->n_tiles, 1)));
        DN_TRY(h->data.d_tile_col.alloc(sizeof(int32_t) * (size_t) std::max<int64_t>(h->n_tiles, 1)));

        if (src.packed) DN_TRY(hipMemcpyAsync(h->data.d_cov, src.packed, sizeof(float) * (size_t) h->total, hipMemcpyHostToDevice, h->stream[0]));
        else { const int rcu = upload_ragged_chunks(h, src, stage, done); if (rcu != DN_OK) return rcu; }
        DN_TRY(hipMemcpyAsync(h->data.d_goff, h->goff.data(), sizeof(int64_t) * (size_t) (n + 1), hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(h->data.d_glen, h->glen.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(h->data.d_order, order.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(h->data.d_svoff, h->svoff.data(), sizeof(int64_t) * (size_t) (n + 1), hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(h->data.d_tile_gene, tg.data(), sizeof(int32_t) * tg.size(), hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(h->data.d_tile_col, tc.data(), sizeof(int32_t) * tc.size(), hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipEventRecord(h->ev_i0, h->stream[0]));
        dn::outer::row_max(h->stream[0], h->data.d_cov, h->data.d_goff, h->data.d_glen, h->data.d_rowmax, h->data.d_x16, n, (int) p, h->n_cus);
        DN_TRY(hipGetLastError());
        DN_TRY(hipEventRecord(h->ev_i1, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        (void) hipEventElapsedTime(&h->last_rowmax_ms, h->ev_i0, h->ev_i1);

        // gene classes
        const dn::KernelSet *pair = nullptr;
        class_lengths(h->ks, p, h->split_len, h->tiny_len, pair);
        std::vector<int32_t> ord[dn_handle_s::NCLS];
        for (int32_t g : order) {                                                                           // stays longest-first
            const int32_t L = h->glen[g];
            ord[(h->split_len > 0 && L <= h->split_len) ? ((pair && L <= h->tiny_len) ? 2 : 1) : 0].push_back(g);
        }
        h->data.cls[0].ks = h->ks;
        h->data.cls[1].ks = (h->ks->p != 0 && h->split_len > 0) ? dn::kernel_set_narrow(p) : nullptr;
        h->data.cls[2].ks = pair;
        if (ord[0].size() >= 8) {
            // Queue order of the wide class: longest first, then zigzagged (longest, shortest, 2nd longest, 2nd shortest, ...).
            // Long genes keep most of their state in the spill tier and pull ~60 GB/s per CU through the fabric, short
            // ones a quarter of that; running only long genes everywhere at the start of a launch saturates the fabric
            // (their pass is 1.4x slower than alone on the chip, tools/contention.sh).  The zigzag keeps the demand level
            // over the launch: +2.9 % on config 2 and more on short queues (+6 % at 5 000 genes per GPU against ordering
            // by the cost predicted from the previous iteration's counters, which clusters the heavy genes even more).
            const size_t n0 = ord[0].size();
            std::vector<int32_t> mixed;
            mixed.reserve(n0);
            for (size_t i = 0, j = n0 - 1; i < j; i++, j--) { mixed.push_back(ord[0][i]); mixed.push_back(ord[0][j]); }
            if (n0 & 1) mixed.push_back(ord[0][n0 / 2]);
            ord[0] = mixed;
        }
        // Hand-down between the classes of the templated kernels (DN_HANDDOWN=0: off)
        const char *henv = getenv("DN_HANDDOWN");
        const bool handdown = h->ks->p != 0 && !h->ks->baseline_ptr && !(henv && henv[0] == '0');
        for (int c = 0; c < dn_handle_s::NCLS; c++) {
            auto &C = h->data.cls[c];
            C.n = (int32_t) ord[c].size();
            if (C.n == 0 || !C.ks) { C.n = 0; continue; }
            DN_TRY(C.d_order.alloc(sizeof(int32_t) * (size_t) C.n));
            DN_TRY(C.d_counter.alloc(sizeof(int32_t) * 4));
            DN_TRY(hipMemcpy(C.d_order, ord[c].data(), sizeof(int32_t) * (size_t) C.n, hipMemcpyHostToDevice));
            C.order = ord[c];
            // columns a scratch slot must hold: the longest gene of the class, or -- for the one-wave-per-gene family,
            // chosen because the announced take-every rate leaves every gene at most 12 active columns -- that bound
            int32_t cols = C.longest = h->glen[ord[c][0]];
            C.recv_longest = 0; C.hand_cols = 0; C.parked = 0;
            if (handdown && c > 0 && h->data.cls[c - 1].n > 0) {        // a class that receives holds the donor's longest gene too
                C.recv_longest = h->data.cls[c - 1].longest;
                DN_TRY(C.d_inq.alloc(sizeof(int32_t) * (size_t) h->data.cls[c - 1].n));
                cols = std::max(cols, C.recv_longest);
            }
            if (C.ks == dn::kernel_set_rows()) cols = (cols + h->ds_hint - 1) / h->ds_hint;
            const int rc = size_class(h, C, cols);
            if (rc != DN_OK) return rc;
        }
        {
            // a class parks a gene once the next class would hold it on chip: that class's register tier + its LDS tier
            // (DN_HANDDOWN_COLS=a,b overrides the wide and the narrow class's width)
            int32_t over[2] = {-1, -1};
            if (const char *cenv = getenv("DN_HANDDOWN_COLS")) (void) sscanf(cenv, "%d,%d", &over[0], &over[1]);
            bool any = false;
            for (int c = 0; c + 1 < dn_handle_s::NCLS; c++) {
                const auto &R = h->data.cls[c + 1];
                if (h->data.cls[c].n == 0 || R.n == 0 || h->ks->p == 0 || h->ks->baseline_ptr) continue;
                h->data.cls[c].hand_cols = over[c] >= 0 ? over[c] : R.ks->reg_tier_cols + R.lds_cols;     // known also with hand-down off (diagnostic builds)
                any = any || (R.recv_longest > 0 && h->data.cls[c].hand_cols > 0);
            }
            if (any) {
                DN_TRY(h->data.host_parked.alloc(sizeof(int32_t) * dn_handle_s::NCLS));
                DN_TRY(h->data.d_hand_int.alloc(sizeof(int32_t) * (size_t) n * dn::HAND_INTS));
                DN_TRY(h->data.d_hand_dbl.alloc(sizeof(double) * (size_t) n * (size_t) (5 * p + 1)));
            }
        }
        if (h->data.cls[0].n == 0 && (h->data.cls[1].n > 0 || h->data.cls[2].n > 0) && h->ks->p == 0) return fail(DN_E_STATE, "internal: empty wide class for the generic kernels");
        return DN_OK;
    });
    if (rc != DN_OK) {
        const std::string msg = g_err;
        free_device(h);
        h->n = 0; h->total = 0;
        return fail(rc, msg);
    }
    return DN_OK;
}

static int check_shape(dn_handle h, int64_t n_genes, int32_t p, const int64_t *lengths)
{
    if (!h) return fail(DN_E_INVALID, "null handle");
    if (n_genes <= 0 || n_genes > INT32_MAX) return fail(DN_E_INVALID, "n_genes must be in [1, 2^31)");
    if (p < 2) return fail(DN_E_INVALID, "need at least 2 samples (svds(k=1) requires 1 < min(shape), nmf.py:63)");
    const dn::KernelSet *ks = dn::kernel_set_for(p);
    if (!ks) return fail(DN_E_UNSUPPORTED, "no kernels compiled for p = " + std::to_string(p) +
                                           (p > dn::P_WIDE_MAX ? " (the widest cohort is " + std::to_string(dn::P_WIDE_MAX) + " samples, dn_p_max())" : std::string()));
    // validate into locals; the handle is only touched once everything checks out
    std::vector<int64_t> goff((size_t) n_genes + 1, 0);
    std::vector<int32_t> glen((size_t) n_genes, 0);
    int32_t lmax = 0;
    for (int64_t g = 0; g < n_genes; g++) {
        if (lengths[g] < 1 || lengths[g] > (int64_t) 1 << 26) return fail(DN_E_INVALID, "gene length out of range at gene " + std::to_string(g));
        glen[g] = (int32_t) lengths[g];
        goff[g + 1] = goff[g] + (int64_t) p * lengths[g];
        lmax = std::max(lmax, glen[g]);
    }
    // Down-sampled regime announced by the caller: when no gene can keep more than 12 active columns the run-time-p
    // kernels serve it row-wise, one wavefront per gene (dn_generic.hip, nmf_rows) -- faster than the column-parallel
    // templated kernels from p ~ 8 on (p = 16: 76 000 vs 41 000 genes/s per run, p = 32: 5x).
    const bool rows_regime = h->ds_hint > 1 && p >= 8 && p <= dn::P_MAX && (lmax + h->ds_hint - 1) / h->ds_hint <= 12;
    const char *force = getenv("DN_FORCE_GENERIC");
    if (rows_regime && !(force && force[0] == '2')) ks = dn::kernel_set_rows();      // DN_FORCE_GENERIC=2: keep the 256-thread family
    else if (rows_regime) ks = dn::kernel_set_generic();
    // commit: the previous data set (if any) is released first, so that a later failure cannot leave old device
    // buffers behind new host-side shapes
    free_device(h);
    h->ks = ks;
    h->n = n_genes; h->p = p;
    h->goff.swap(goff); h->glen.swap(glen);
    h->total = h->goff[n_genes];
    h->lmax = lmax;
    return DN_OK;
}

int dn_set_downsample_hint(dn_handle h, int32_t rate)
{
    if (!h) return fail(DN_E_INVALID, "null handle");
    if (rate < 1) return fail(DN_E_INVALID, "downsample rate must be >= 1");
    h->ds_hint = rate;
    return DN_OK;
}

int dn_set_trace_columns(dn_handle h, int32_t cols)
{
    if (!h) return fail(DN_E_INVALID, "null handle");
    if (cols < 8 || cols > dn::TRACE_LEN) return fail(DN_E_INVALID, "trace columns must be in [8, DN_TRACE_LEN]");
    h->trace_cols = cols;
    h->have_trace = false;                                // the host copy changes shape: no stale counters for the queue order
    return DN_OK;
}

int dn_set_solver_step_cap(dn_handle h, int32_t max_steps)
{
    if (!h) return fail(DN_E_INVALID, "null handle");
    if (max_steps < 1) return fail(DN_E_INVALID, "the solver step cap must be >= 1");
    h->max_steps = max_steps;
    return DN_OK;
}

int dn_upload_packed(dn_handle h, int64_t n_genes, int32_t p, const float *packed, const int64_t *lengths)
{
    if (!packed || !lengths) return fail(DN_E_INVALID, "dn_upload_packed: null argument");
    int rc = check_shape(h, n_genes, p, lengths);
    if (rc != DN_OK) return rc;
    CoverageSource src;
    src.packed = packed;
    return finish_upload(h, src);
}

int dn_upload_ragged(dn_handle h, int64_t n_genes, int32_t p, const void *const *genes, const int64_t *lengths,
                     int32_t is_f32, int32_t n_threads, int64_t *inexact)
{
    if (!genes || !lengths) return fail(DN_E_INVALID, "dn_upload_ragged: null argument");
    int rc = check_shape(h, n_genes, p, lengths);
    if (rc != DN_OK) return rc;
    DN_TRY(hipSetDevice(h->device));
    if (n_threads < 1) n_threads = (int32_t) std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::atomic<int64_t> bad(0);
    CoverageSource src;
    src.genes = genes; src.is_f32 = is_f32; src.n_threads = n_threads; src.bad = &bad;
    rc = finish_upload(h, src);
    if (inexact) *inexact = bad.load();
    return rc;
}

int dn_ratio_svd_sums(dn_handle h, double *est_sums, double *cov_sums, int32_t *status)
{
    if (!h || !h->data.d_cov) return fail(DN_E_STATE, "dn_ratio_svd_sums: nothing uploaded");
    if ((est_sums == nullptr) != (cov_sums == nullptr)) return fail(DN_E_INVALID, "dn_ratio_svd_sums: the two sums are fetched together or not at all");
    dn::InitArgs a;
    a.cov = h->data.d_cov; a.goff = h->data.d_goff; a.glen = h->data.d_glen; a.order = h->data.d_order; a.counter = h->data.d_counter;
    a.est_sums = h->data.d_est_sums; a.cov_sums = h->data.d_cov_sums; a.status = h->data.d_status; a.n_genes = (int32_t) h->n;
    a.p = h->p; a.ws = h->data.cls[0].d_ws; a.slot_bytes = h->data.cls[0].slot_bytes; a.S = h->data.cls[0].S; a.max_steps = h->max_steps;
    a.x16 = h->data.d_x16;
    { const char *f64 = getenv("DN_INIT_FP64"); a.force_fp64 = (f64 && f64[0] == '1') ? 1 : 0; }
    return on_main_stream(h, [&]() -> int {
        DN_TRY(hipMemsetAsync(h->data.d_counter, 0, sizeof(int32_t) * 4, h->stream[0]));
        // occupancy of the kernel that ks->init() will start: from 17 samples on it is the matrix-core variant (round 2 asked for
        // the power-iteration kernel's figure here and ran k_ratio_svd_mg at ONE workgroup per CU instead of two)
        const int which_init = h->p >= 17 ? 2 : 1;        // (the wide-cohort set has one initial pass and answers for it either way)
        int per_cu = std::max(1, h->ks->blocks_per_cu(which_init));
        int grid = (int) std::min<int64_t>(h->n, (int64_t) per_cu * h->n_cus);
        if (h->ks->p == 0) grid = std::min(grid, h->data.cls[0].slots);          // generic kernels work in the scratch slots
        DN_TRY(hipEventRecord(h->ev_i0, h->stream[0]));
        h->ks->init(a, grid, h->stream[0]);
        DN_TRY(hipGetLastError());
        DN_TRY(hipEventRecord(h->ev_i1, h->stream[0]));
        const size_t np = (size_t) h->n * h->p;
        if (est_sums) {                     // null: the sums stay on the device (dn_init_partials reduces them there)
            DN_TRY(hipMemcpyAsync(est_sums, h->data.d_est_sums, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream[0]));
            DN_TRY(hipMemcpyAsync(cov_sums, h->data.d_cov_sums, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream[0]));
        }
        if (status) DN_TRY(hipMemcpyAsync(status, h->data.d_status, sizeof(int32_t) * (size_t) h->n, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        DN_TRY(hipEventElapsedTime(&h->last_init_ms, h->ev_i0, h->ev_i1));
        if (h->ks->init_name) snprintf(h->init_name, sizeof(h->init_name), "%s", h->ks->init_name);
        else if (h->ks->p >= 2 && h->ks->p <= 16) snprintf(h->init_name, sizeof(h->init_name), "k_ratio_svd<%d,%d>", h->ks->p, h->ks->nt);
        else snprintf(h->init_name, sizeof(h->init_name), h->p >= 17 ? "gen::k_ratio_svd_mg" : "gen::k_ratio_svd_gen");
        return DN_OK;
    });
}

int dn_baseline_iteration(dn_handle h, const double *scale, const dn_params *prm, const int64_t *ds_start,
                          double *rho, int32_t *flags, int32_t *trace)
{
    if (!h || !h->data.d_cov) return fail(DN_E_STATE, "dn_baseline_iteration: nothing uploaded");
    if (!scale || !prm) return fail(DN_E_INVALID, "dn_baseline_iteration: null argument");
    if ((rho == nullptr) != (flags == nullptr)) return fail(DN_E_INVALID, "dn_baseline_iteration: rho and flags are fetched together or not at all");
    { const int rc = check_params(prm, ds_start, h->n, [&](int64_t g) { return h->glen[g]; }); if (rc != DN_OK) return rc; }
    for (int i = 0; i < h->p; i++) if (!(scale[i] > 0.0) || !std::isfinite(scale[i])) return fail(DN_E_INVALID, "scale factors must be positive and finite");
    DN_TRY(hipSetDevice(h->device));
    return synced_classes(h, [&]() -> int {
        // the scratch slots were sized at upload (for the announced take-every rate in the one-wave-per-gene family):
        // grow them if this iteration's rate leaves more active columns than they hold
        const int32_t rate = prm->downsample_rate;
        for (auto &C : h->data.cls) {
            if (C.n == 0 || !C.ks) continue;
            const int32_t longest = std::max(C.longest, C.recv_longest);
            const int32_t need = rate > 1 ? (longest + rate - 1) / rate : longest;
            if (need > C.S) {
                DN_TRY(hipStreamSynchronize(h->stream[0]));
                const int rc = size_class(h, C, need);
                if (rc != DN_OK) return rc;
            }
        }
        if (prm->want_estimates && !h->data.d_svec)
            DN_TRY(h->data.d_svec.alloc(sizeof(double) * (size_t) std::max<int64_t>(h->svoff[h->n], 1)));

        dn::IterArgs a;
        std::memset(&a, 0, sizeof(a));
        a.cov = h->data.d_cov; a.goff = h->data.d_goff; a.glen = h->data.d_glen; a.order = h->data.d_order; a.counter = h->data.d_counter;
        a.ds_start = nullptr;
        a.ws = h->data.cls[0].d_ws; a.rho = h->data.d_rho; a.flags = h->data.d_flags; a.trace = h->data.d_trace; a.kfin = h->data.d_kfin; a.emode = h->data.d_emode;
        a.svec = h->data.d_svec; a.svoff = h->data.d_svoff; a.slot_bytes = h->data.cls[0].slot_bytes; a.n_genes = (int32_t) h->n; a.S = h->data.cls[0].S;
        a.p = h->p; a.rowmax = h->data.d_rowmax; a.x16 = h->data.d_x16; a.max_steps = h->max_steps;
        a.T = prm->nmf_iter; a.bins = prm->bins; a.min_hc = prm->min_high_coverage; a.rate = prm->downsample_rate;
        a.skip = prm->skip_baseline_selection ? 1 : 0; a.want_est = prm->want_estimates ? 1 : 0;
        for (int i = 0; i < h->p; i++) h->last_scale[i] = scale[i];
        if (h->ks->baseline_ptr) {          // wide cohorts: the factors travel through d_scales, the struct's arrays stay zero
            for (int i = 0; i < h->p; i++) { h->scales_host[i] = scale[i]; h->scales_host[dn::P_WIDE_MAX + i] = 1.0 / scale[i]; }
            DN_TRY(hipMemcpyAsync(h->data.d_scales, h->scales_host, sizeof(double) * 2 * dn::P_WIDE_MAX, hipMemcpyHostToDevice, h->stream[0]));
        } else {
            for (int i = 0; i < h->p; i++) { a.scale[i] = scale[i]; a.inv_scale[i] = 1.0 / scale[i]; }
            for (int i = h->p; i < dn::P_MAX; i++) { a.scale[i] = 1.0; a.inv_scale[i] = 1.0; }
        }
        if (prm->downsample_rate > 1) {
            DN_TRY(hipMemcpyAsync(h->data.d_ds, ds_start, sizeof(int64_t) * (size_t) h->n, hipMemcpyHostToDevice, h->stream[0]));
            a.ds_start = h->data.d_ds;
        }
        // The narrow class (state in LDS, little fabric traffic) orders its queue most expensive first from the second
        // iteration on, the cost of a gene predicted from the previous iteration's counters (sum of active columns over its
        // nmf() calls plus a fixed part per call worth ~4 columns per lane): its genes are what fills the end of a launch.
        // The wide class keeps the zigzag (it is bound by the fabric, see upload).
        for (int wc = 1; wc < dn_handle_s::NCLS; wc++) {
            auto &C = h->data.cls[wc];
            if (!h->have_trace || C.n == 0 || !C.ks) continue;
            const double per_call = 4.0 * (double) (C.ks->nt > 0 ? C.ks->nt : 128);
            std::vector<std::pair<double, int32_t>> key((size_t) C.n);
            for (int32_t k = 0; k < C.n; k++) {
                const int32_t g = C.order[k];
                const int32_t *tr = &h->data.host_trace[(size_t) g * h->trace_cols];
                key[k] = {(double) tr[2] + per_call * (double) tr[1] + 1e-3 * (double) h->glen[g], g};
            }
            std::stable_sort(key.begin(), key.end(), [](const std::pair<double, int32_t> &a, const std::pair<double, int32_t> &b) { return a.first > b.first; });
            for (int32_t k = 0; k < C.n; k++) C.order[k] = key[k].second;
            DN_TRY(hipMemcpyAsync(C.d_order, C.order.data(), sizeof(int32_t) * (size_t) C.n, hipMemcpyHostToDevice, h->stream[0]));
        }
        DN_TRY(hipMemsetAsync(h->data.d_trace, 0, sizeof(int32_t) * (size_t) h->n * dn::TRACE_LEN, h->stream[0]));
        for (auto &C : h->data.cls) if (C.n > 0) DN_TRY(hipMemsetAsync(C.d_counter, 0, sizeof(int32_t) * 4, h->stream[0]));
        DN_TRY(hipEventRecord(h->ev_ready, h->stream[0]));
        int first_cls = -1;
        // hand-down needs the whole gene in the drop loop's own columns and no estimate state: off with want_estimates (the s_start
        // vector stays in the donor's slot), with down-sampling, and when the record cannot hold the bin list
        const bool hand_ok = h->data.d_hand_int && !prm->want_estimates && prm->downsample_rate <= 1 && prm->bins <= dn::HAND_MAX_BINS;
        bool donor_parks = false, parked_from[dn_handle_s::NCLS] = {false, false, false};
        for (int c = 0; c < dn_handle_s::NCLS; c++) {
            auto &C = h->data.cls[c];
            C.last_ms = 0.f;
            if (C.n == 0) continue;
            if (first_cls < 0) first_cls = c;
            hipStream_t st = h->stream[c];
            if (c > 0) DN_TRY(hipStreamWaitEvent(st, h->ev_ready, 0));
            a.order = C.d_order; a.counter = C.d_counter; a.ws = C.d_ws; a.slot_bytes = C.slot_bytes; a.S = C.S;
            a.lds_cols = C.lds_cols; a.n_genes = C.n;
            // Hand-down.  The first launch of a class parks the genes that its drop loop has shrunk to hand_cols columns into the next
            // class's continuation queue; that class's SECOND launch, queued on its own stream behind its first and behind the end of
            // this one (ev_mid), finishes them.  Every dependency sits at a kernel boundary: no workgroup waits for another kernel,
            // and a second launch whose queue is empty ends at once.  One level per gene: a second launch parks nothing, so a wide
            // gene never reaches the pair class.
            C.parked = 0;
            a.handdown_cols = C.hand_cols;
            a.hand_int = h->data.d_hand_int; a.hand_dbl = h->data.d_hand_dbl;
            a.park_queue = nullptr; a.park_count = nullptr; a.resume_queue = nullptr; a.resume_count = nullptr;
            const bool parks = hand_ok && c + 1 < dn_handle_s::NCLS && C.hand_cols > 0 && h->data.cls[c + 1].recv_longest > 0 && h->data.cls[c + 1].n > 0;
            if (parks) { a.park_queue = h->data.cls[c + 1].d_inq; a.park_count = h->data.cls[c + 1].d_counter + 2; }
            DN_TRY(hipEventRecord(h->ev_start[c], st));
            const int lrc = C.ks->baseline_ptr ? C.ks->baseline_ptr(a, h->data.d_scales, C.slots, st) : C.ks->baseline(a, C.slots, C.dyn_lds, st);
            if (lrc != 0) return fail(DN_E_HIP, std::string("k_baseline launch: ") + hipGetErrorString((hipError_t) lrc));
            if (parks) DN_TRY(hipEventRecord(h->ev_mid[c], st));
            if (c > 0 && donor_parks) {
                DN_TRY(hipStreamWaitEvent(st, h->ev_mid[c - 1], 0));
                a.park_queue = nullptr; a.park_count = nullptr;
                a.counter = C.d_counter + 1; a.resume_queue = C.d_inq; a.resume_count = C.d_counter + 2;
                const int lrc2 = C.ks->baseline(a, C.slots, C.dyn_lds, st);
                if (lrc2 != 0) return fail(DN_E_HIP, std::string("k_baseline launch (continuations): ") + hipGetErrorString((hipError_t) lrc2));
            }
            DN_TRY(hipEventRecord(h->ev_end[c], st));
            parked_from[c] = c > 0 && donor_parks;
            donor_parks = parks;
        }
        for (int c = 1; c < dn_handle_s::NCLS; c++)                                   // results are copied on the main stream
            if (h->data.cls[c].n > 0) DN_TRY(hipStreamWaitEvent(h->stream[0], h->ev_end[c], 0));
        for (int c = 1; c < dn_handle_s::NCLS; c++)                                   // how many genes each donor parked (dn_handdown)
            if (parked_from[c]) DN_TRY(hipMemcpyAsync(h->data.host_parked + (c - 1), h->data.cls[c].d_counter + 2, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream[0]));
        if (rho) {                          // null: the DI rows stay on the device (dn_outer_partials / dn_outer_apply / dn_fetch_outer)
            DN_TRY(hipMemcpyAsync(rho, h->data.d_rho, sizeof(double) * (size_t) h->n * h->p, hipMemcpyDeviceToHost, h->stream[0]));
            DN_TRY(hipMemcpyAsync(flags, h->data.d_flags, sizeof(int32_t) * (size_t) h->n, hipMemcpyDeviceToHost, h->stream[0]));
        }
        const int32_t tcols = h->trace_cols;
        const size_t trace_ints = (size_t) h->n * (size_t) tcols;
        if (h->data.host_trace_len < trace_ints) {
            h->data.host_trace_len = 0;
            DN_TRY(h->data.host_trace.alloc(sizeof(int32_t) * trace_ints));
            h->data.host_trace_len = trace_ints;
        }
        if (tcols == dn::TRACE_LEN)
            DN_TRY(hipMemcpyAsync(h->data.host_trace, h->data.d_trace, sizeof(int32_t) * trace_ints, hipMemcpyDeviceToHost, h->stream[0]));
        else {
            if (!h->data.d_trace_head) DN_TRY(h->data.d_trace_head.alloc(sizeof(int32_t) * (size_t) h->n * dn::TRACE_LEN));
            dn::outer::trace_head(h->stream[0], h->data.d_trace, h->data.d_trace_head, trace_ints, (int) tcols);
            DN_TRY(hipGetLastError());
            DN_TRY(hipMemcpyAsync(h->data.host_trace, h->data.d_trace_head, sizeof(int32_t) * trace_ints, hipMemcpyDeviceToHost, h->stream[0]));
        }
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        for (int c = 1; c < dn_handle_s::NCLS; c++) if (parked_from[c]) h->data.cls[c - 1].parked = h->data.host_parked[c - 1];
        h->have_trace = (prm->downsample_rate <= 1);          // with down-sampling the active columns are redrawn every iteration
        if (trace) std::memcpy(trace, h->data.host_trace, sizeof(int32_t) * trace_ints);
        h->last_span_ms = 0.f;
        for (int c = 0; c < dn_handle_s::NCLS; c++) {
            if (h->data.cls[c].n == 0) continue;
            DN_TRY(hipEventElapsedTime(&h->data.cls[c].last_ms, h->ev_start[c], h->ev_end[c]));
            float span = 0.f;                                                // the classes are launched in order: the first start opens the span
            DN_TRY(hipEventElapsedTime(&span, h->ev_start[first_cls], h->ev_end[c]));
            h->last_span_ms = std::max(h->last_span_ms, span);
        }
        h->last_ms = first_cls >= 0 ? h->data.cls[first_cls].last_ms : 0.f;
        h->data.have_estimate_state = prm->want_estimates != 0;
        return DN_OK;
    });
}

// d_pvec: the 3p + 4 sums, then (at PVEC_SUMS) avg_di and norm, P_WIDE_MAX doubles each
constexpr int PVEC_SUMS = 3 * dn::P_WIDE_MAX + 4;

static int outer_alloc(dn_handle h, int32_t degnorm_iter)
{
    const size_t np = (size_t) h->n * h->p;
    if (!h->data.d_rhoc) {
        DN_TRY(h->data.d_rhoc.alloc(sizeof(double) * np));
        DN_TRY(h->data.d_xw.alloc(sizeof(double) * np));
        DN_TRY(h->data.d_xadj.alloc(sizeof(double) * np));
    }
    if (!h->data.d_part) {
        DN_TRY(h->data.d_part.alloc(sizeof(double) * dn::outer::PART_DOUBLES));     // sized for the widest cohort
        DN_TRY(h->data.d_pvec.alloc(sizeof(double) * (PVEC_SUMS + 2 * dn::P_WIDE_MAX)));
    }
    if (degnorm_iter > 0 && h->data.n_iter != degnorm_iter) {
        DN_TRY(h->data.d_ran.alloc((size_t) h->n * degnorm_iter));
        h->data.n_iter = degnorm_iter;
    }
    return DN_OK;
}

// Queue "block partials + reduce" on the handle's stream: the sums of the initial normalisation (k_init_partials) or of an
// outer update (k_outer_partials) over the handle's genes, block by block, then added in block order into d_pvec[0 .. 3p + 4)
static int queue_partials(dn_handle h, bool initial)
{
    const dn_handle_s::DataSet &d = h->data;
    if (initial) dn::outer::init_partials(h->stream[0], d.d_est_sums, d.d_cov_sums, d.d_status, d.d_x, d.d_part, d.d_pvec, h->n, (int) h->p);
    else dn::outer::partials(h->stream[0], d.d_rho, d.d_rhoc, d.d_xw, d.d_trace, d.d_flags, d.d_part, d.d_pvec, h->n, (int) h->p);
    DN_TRY(hipGetLastError());
    return DN_OK;
}

int dn_init_begin(dn_handle h, const double *reads)
{
    if (!h || !h->data.d_cov) return fail(DN_E_STATE, "dn_init_begin: nothing uploaded");
    if (!reads) return fail(DN_E_INVALID, "dn_init_begin: null argument");
    return on_main_stream(h, [&]() -> int {
        const size_t np = (size_t) h->n * h->p;
        if (!h->data.d_x) DN_TRY(h->data.d_x.alloc(sizeof(double) * np));
        DN_TRY(hipMemcpyAsync(h->data.d_x, reads, sizeof(double) * np, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

int dn_init_partials(dn_handle h, double *partials)
{
    if (!h || !h->data.d_x) return fail(DN_E_STATE, "dn_init_partials: dn_init_begin has not been called");
    if (!partials) return fail(DN_E_INVALID, "dn_init_partials: null output");
    return on_main_stream(h, [&]() -> int {
        { const int rc = outer_alloc(h, 0); if (rc != DN_OK) return rc; }
        { const int rc = queue_partials(h, true); if (rc != DN_OK) return rc; }
        DN_TRY(hipMemcpyAsync(partials, h->data.d_pvec, sizeof(double) * (size_t) (3 * h->p + 4), hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

int dn_outer_begin_scaled(dn_handle h, const double *norm, int32_t degnorm_iter)
{
    if (!h || !h->data.d_x) return fail(DN_E_STATE, "dn_outer_begin_scaled: dn_init_begin has not been called");
    if (!norm || degnorm_iter < 1) return fail(DN_E_INVALID, "dn_outer_begin_scaled: bad argument");
    return on_main_stream(h, [&]() -> int {
        { const int rc = outer_alloc(h, degnorm_iter); if (rc != DN_OK) return rc; }
        const size_t np = (size_t) h->n * h->p;
        double *d_norm = h->data.d_pvec + PVEC_SUMS + dn::P_WIDE_MAX;
        DN_TRY(hipMemsetAsync(h->data.d_ran, 0, (size_t) h->n * degnorm_iter, h->stream[0]));
        DN_TRY(hipMemcpyAsync(d_norm, norm, sizeof(double) * (size_t) h->p, hipMemcpyHostToDevice, h->stream[0]));
        dn::outer::scale_reads(h->stream[0], h->data.d_x, d_norm, h->data.d_xw, np, (int) h->p);
        DN_TRY(hipGetLastError());
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

int dn_outer_begin(dn_handle h, const double *x_weighted, int32_t degnorm_iter)
{
    if (!h || !h->data.d_cov) return fail(DN_E_STATE, "dn_outer_begin: nothing uploaded");
    if (!x_weighted || degnorm_iter < 1) return fail(DN_E_INVALID, "dn_outer_begin: bad argument");
    return on_main_stream(h, [&]() -> int {
        const size_t np = (size_t) h->n * h->p;
        { const int rc = outer_alloc(h, degnorm_iter); if (rc != DN_OK) return rc; }
        DN_TRY(hipMemsetAsync(h->data.d_ran, 0, (size_t) h->n * degnorm_iter, h->stream[0]));
        DN_TRY(hipMemcpyAsync(h->data.d_xw, x_weighted, sizeof(double) * np, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

int dn_outer_partials(dn_handle h, double *partials)
{
    if (!h || !h->data.d_xw) return fail(DN_E_STATE, "dn_outer_partials: dn_outer_begin has not been called");
    if (!partials) return fail(DN_E_INVALID, "dn_outer_partials: null output");
    return on_main_stream(h, [&]() -> int {
        { const int rc = queue_partials(h, false); if (rc != DN_OK) return rc; }
        DN_TRY(hipMemcpyAsync(partials, h->data.d_pvec, sizeof(double) * (size_t) (3 * h->p + 4), hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

int dn_outer_partials_device(dn_handle h, double **d_partials)
{
    if (!h || !h->data.d_xw) return fail(DN_E_STATE, "dn_outer_partials_device: dn_outer_begin has not been called");
    if (!d_partials) return fail(DN_E_INVALID, "dn_outer_partials_device: null output");
    return on_main_stream(h, [&]() -> int {
        { const int rc = queue_partials(h, false); if (rc != DN_OK) return rc; }
        DN_TRY(hipStreamSynchronize(h->stream[0]));           // the collective runs on the caller's stream: the sums must be there
        *d_partials = h->data.d_pvec;
        return DN_OK;
    });
}

int dn_outer_apply(dn_handle h, const double *avg_di, const double *norm, int32_t iter)
{
    if (!h || !h->data.d_xw) return fail(DN_E_STATE, "dn_outer_apply: dn_outer_begin has not been called");
    if (!norm || iter < 0) return fail(DN_E_INVALID, "dn_outer_apply: bad argument");
    return on_main_stream(h, [&]() -> int {
        double *d_avg = h->data.d_pvec + PVEC_SUMS, *d_norm = d_avg + dn::P_WIDE_MAX;
        if (avg_di) DN_TRY(hipMemcpyAsync(d_avg, avg_di, sizeof(double) * (size_t) h->p, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(d_norm, norm, sizeof(double) * (size_t) h->p, hipMemcpyHostToDevice, h->stream[0]));
        dn::outer::apply(h->stream[0], h->data.d_rhoc, h->data.d_xw, h->data.d_xadj, h->data.d_flags, h->data.d_ran, d_avg, d_norm, avg_di != nullptr,
                         h->n, (int) h->p, (int) iter, (int) h->data.n_iter);
        DN_TRY(hipGetLastError());
        DN_TRY(hipStreamSynchronize(h->stream[0]));           // the host buffers behind avg_di / norm may go away
        return DN_OK;
    });
}

// ---------------------------------------------------------------------------------------------------
// The collective of the sharded run inside the library (nmf_mpi.py:758-815 moves whole coverage chunks and DI matrices
// through rank 0; here 3p + 4 doubles are summed over the GPUs in place, on the handle's own stream, by RCCL over xGMI).
// ---------------------------------------------------------------------------------------------------
#define RCCL_TRY(api, expr)                                                                        \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess)                                                                     \
            return fail(DN_E_HIP, std::string(#expr) + ": " + (api)->GetErrorString(r_));          \
    } while (0)

int dn_comm_unique_id(uint8_t *id)
{
    if (!id) return fail(DN_E_INVALID, "dn_comm_unique_id: null argument");
    std::string err;
    RcclApi *api = rccl_api(err);
    if (!api) return fail(DN_E_STATE, "dn_comm_unique_id: " + err);
    static_assert(sizeof(ncclUniqueId) == DN_COMM_ID_BYTES, "DN_COMM_ID_BYTES must be sizeof(ncclUniqueId)");
    ncclUniqueId u;
    RCCL_TRY(api, api->GetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return DN_OK;
}

int dn_comm_create(dn_handle h, const uint8_t *id, int32_t rank, int32_t size)
{
    if (!h) return fail(DN_E_INVALID, "dn_comm_create: null handle");
    if (!id || size < 1 || rank < 0 || rank >= size) return fail(DN_E_INVALID, "dn_comm_create: bad argument");
    if (h->comm) return fail(DN_E_STATE, "dn_comm_create: this handle already has a communicator");
    std::string err;
    RcclApi *api = rccl_api(err);
    if (!api) return fail(DN_E_STATE, "dn_comm_create: " + err);
    DN_TRY(hipSetDevice(h->device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t c = nullptr;
    RCCL_TRY(api, api->CommInitRank(&c, size, u, rank));
    h->comm = c; h->comm_rank = rank; h->comm_size = size;
    if (!h->d_comm) DN_TRY(h->d_comm.alloc(sizeof(double) * DN_COMM_MAX_DOUBLES));
    return DN_OK;
}

int dn_comm_destroy(dn_handle h)
{
    if (!h || !h->comm) return DN_OK;
    std::string err;
    RcclApi *api = rccl_api(err);
    (void) hipSetDevice(h->device);
    if (h->stream[0]) (void) hipStreamSynchronize(h->stream[0]);
    if (api) (void) api->CommDestroy((ncclComm_t) h->comm);
    h->comm = nullptr; h->comm_size = 0; h->comm_rank = 0;
    h->d_comm.reset();
    return DN_OK;
}

int32_t dn_comm_size(dn_handle h) { return h ? h->comm_size : 0; }

const char *dn_comm_library(void)
{
    std::string err;
    RcclApi *api = rccl_api(err);
    static std::string text;
    if (!api) { text = ""; return text.c_str(); }
    int v = 0;
    if (api->GetVersion) (void) api->GetVersion(&v);
    text = api->path + ", nccl api " + std::to_string(v);
    return text.c_str();
}

// sum d_buf[0 .. count) over the ranks in place on the handle's stream, then copy the totals to the host
static int allreduce_to_host(dn_handle h, double *d_buf, int32_t count, double *totals)
{
    std::string err;
    RcclApi *api = rccl_api(err);
    if (!api) return fail(DN_E_STATE, err);
    RCCL_TRY(api, api->AllReduce(d_buf, d_buf, (size_t) count, ncclDouble, ncclSum, (ncclComm_t) h->comm, h->stream[0]));
    DN_TRY(hipMemcpyAsync(totals, d_buf, sizeof(double) * (size_t) count, hipMemcpyDeviceToHost, h->stream[0]));
    DN_TRY(hipStreamSynchronize(h->stream[0]));
    return DN_OK;
}

int dn_comm_allreduce(dn_handle h, double *buf, int32_t count)
{
    if (!h || !h->comm) return fail(DN_E_STATE, "dn_comm_allreduce: dn_comm_create has not been called");
    if (!buf || count < 1 || count > DN_COMM_MAX_DOUBLES) return fail(DN_E_INVALID, "dn_comm_allreduce: 1 .. " + std::to_string(DN_COMM_MAX_DOUBLES) + " doubles");
    return on_main_stream(h, [&]() -> int {
        DN_TRY(hipMemcpyAsync(h->d_comm, buf, sizeof(double) * (size_t) count, hipMemcpyHostToDevice, h->stream[0]));
        return allreduce_to_host(h, h->d_comm, count, buf);
    });
}

int dn_init_allreduce(dn_handle h, double *totals)
{
    if (!h || !h->comm) return fail(DN_E_STATE, "dn_init_allreduce: dn_comm_create has not been called");
    if (!h->data.d_x) return fail(DN_E_STATE, "dn_init_allreduce: dn_init_begin has not been called");
    if (!totals) return fail(DN_E_INVALID, "dn_init_allreduce: null output");
    return on_main_stream(h, [&]() -> int {
        { const int rc = outer_alloc(h, 0); if (rc != DN_OK) return rc; }
        { const int rc = queue_partials(h, true); if (rc != DN_OK) return rc; }
        return allreduce_to_host(h, h->data.d_pvec, 3 * h->p + 4, totals);
    });
}

int dn_outer_allreduce(dn_handle h, double *totals)
{
    if (!h || !h->comm) return fail(DN_E_STATE, "dn_outer_allreduce: dn_comm_create has not been called");
    if (!h->data.d_xw) return fail(DN_E_STATE, "dn_outer_allreduce: dn_outer_begin has not been called");
    if (!totals) return fail(DN_E_INVALID, "dn_outer_allreduce: null output");
    return on_main_stream(h, [&]() -> int {
        { const int rc = queue_partials(h, false); if (rc != DN_OK) return rc; }
        return allreduce_to_host(h, h->data.d_pvec, 3 * h->p + 4, totals);
    });
}

int dn_fetch_outer(dn_handle h, double *rho, double *x_adj, double *x_weighted, uint8_t *ran)
{
    if (!h || !h->data.d_xw) return fail(DN_E_STATE, "dn_fetch_outer: dn_outer_begin has not been called");
    return on_main_stream(h, [&]() -> int {
        const size_t np = (size_t) h->n * h->p;
        if (rho) DN_TRY(hipMemcpyAsync(rho, h->data.d_rhoc, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream[0]));
        if (x_adj) DN_TRY(hipMemcpyAsync(x_adj, h->data.d_xadj, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream[0]));
        if (x_weighted) DN_TRY(hipMemcpyAsync(x_weighted, h->data.d_xw, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream[0]));
        if (ran) DN_TRY(hipMemcpyAsync(ran, h->data.d_ran, (size_t) h->n * h->data.n_iter, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

int dn_fetch_rows(dn_handle h, int64_t n_rows, const int64_t *rows, double *rho_raw, int32_t *flags)
{
    if (!h || !h->data.d_cov) return fail(DN_E_STATE, "dn_fetch_rows: nothing uploaded");
    if (n_rows <= 0 || !rows || !rho_raw || !flags) return fail(DN_E_INVALID, "dn_fetch_rows: bad argument");
    for (int64_t k = 0; k < n_rows; k++) if (rows[k] < 0 || rows[k] >= h->n) return fail(DN_E_INVALID, "dn_fetch_rows: row out of range");
    const char *what = "dn_fetch_rows";
    dn::DeviceBuffer<int64_t> d_rows;
    dn::DeviceBuffer<double> d_out;
    dn::DeviceBuffer<int32_t> d_fl;
    return on_main_stream(h, [&]() -> int {
        DN_TRY(d_rows.alloc(sizeof(int64_t) * (size_t) n_rows));
        DN_TRY_AS(what, d_out.alloc(sizeof(double) * (size_t) n_rows * h->p));
        DN_TRY_AS(what, d_fl.alloc(sizeof(int32_t) * (size_t) n_rows));
        DN_TRY_AS(what, hipMemcpyAsync(d_rows, rows, sizeof(int64_t) * (size_t) n_rows, hipMemcpyHostToDevice, h->stream[0]));
        dn::outer::gather_rows(h->stream[0], h->data.d_rho, h->data.d_flags, d_rows, d_out, d_fl, (int) n_rows, (int) h->p);
        DN_TRY_AS(what, hipGetLastError());
        DN_TRY_AS(what, hipMemcpyAsync(rho_raw, d_out, sizeof(double) * (size_t) n_rows * h->p, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY_AS(what, hipMemcpyAsync(flags, d_fl, sizeof(int32_t) * (size_t) n_rows, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY_AS(what, hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

// The test seam (TEST-ONLY, see the header): state that only a kernel writes, overwritten from host memory, and the two upload
// outputs that nothing else returns, copied out.  Copies on the main stream, no kernel.
int dn_debug_plant(dn_handle h, int32_t which, const void *src)
{
    if (!h) return fail(DN_E_INVALID, "dn_debug_plant: null handle");
    if (!src) return fail(DN_E_INVALID, "dn_debug_plant: null source");
    if (which < DN_PLANT_RHO_RAW || which > DN_PLANT_INIT_STATUS) return fail(DN_E_INVALID, "dn_debug_plant: unknown array");
    if (!h->data.d_cov) return fail(DN_E_STATE, "dn_debug_plant: nothing uploaded");
    return on_main_stream(h, [&]() -> int {
        const size_t n = (size_t) h->n, np = n * (size_t) h->p;
        switch (which) {
            case DN_PLANT_RHO_RAW: DN_TRY(hipMemcpyAsync(h->data.d_rho, src, sizeof(double) * np, hipMemcpyHostToDevice, h->stream[0])); break;
            case DN_PLANT_FLAGS: DN_TRY(hipMemcpyAsync(h->data.d_flags, src, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream[0])); break;
            case DN_PLANT_ITER_STATUS:                         // column 6 of the n x TRACE_LEN counters: a strided copy
                DN_TRY(hipMemcpy2DAsync(h->data.d_trace + 6, sizeof(int32_t) * dn::TRACE_LEN, src, sizeof(int32_t), sizeof(int32_t), n,
                                        hipMemcpyHostToDevice, h->stream[0]));
                break;
            case DN_PLANT_EST_SUMS: DN_TRY(hipMemcpyAsync(h->data.d_est_sums, src, sizeof(double) * np, hipMemcpyHostToDevice, h->stream[0])); break;
            case DN_PLANT_COV_SUMS: DN_TRY(hipMemcpyAsync(h->data.d_cov_sums, src, sizeof(double) * np, hipMemcpyHostToDevice, h->stream[0])); break;
            default: DN_TRY(hipMemcpyAsync(h->data.d_status, src, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream[0])); break;
        }
        DN_TRY(hipStreamSynchronize(h->stream[0]));           // the host buffer behind src may go away
        return DN_OK;
    });
}

int dn_debug_peek(dn_handle h, int32_t which, void *dst)
{
    if (!h) return fail(DN_E_INVALID, "dn_debug_peek: null handle");
    if (!dst) return fail(DN_E_INVALID, "dn_debug_peek: null destination");
    if (which != DN_PEEK_ROWMAX && which != DN_PEEK_X16) return fail(DN_E_INVALID, "dn_debug_peek: unknown array");
    if (!h->data.d_rowmax || !h->data.d_x16) return fail(DN_E_STATE, "dn_debug_peek: nothing uploaded");
    return on_main_stream(h, [&]() -> int {
        const size_t n = (size_t) h->n;
        if (which == DN_PEEK_ROWMAX) DN_TRY(hipMemcpyAsync(dst, h->data.d_rowmax, sizeof(float) * n * (size_t) h->p, hipMemcpyDeviceToHost, h->stream[0]));
        else DN_TRY(hipMemcpyAsync(dst, h->data.d_x16, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

// First touch of a large, freshly allocated host buffer from several threads at once (one write per 4 KiB page; the caller
// overwrites every byte afterwards): a single thread faults ~4 GB of new pages in 0.15-0.2 s on the GPU box, which is more
// than the copy that fills them takes.
static void prefault_pages(void *ptr, size_t bytes, int n_threads)
{
    if (!ptr || bytes < ((size_t) 64 << 20)) return;
    char *base = (char *) ptr;
    const size_t page = 4096, n_pages = (bytes + page - 1) / page;
    n_threads = std::max(1, std::min(n_threads, 16));
    std::vector<std::thread> th;
    for (int t = 0; t < n_threads; t++)
        th.emplace_back([=]() {
            const size_t lo = n_pages * (size_t) t / (size_t) n_threads, hi = n_pages * (size_t) (t + 1) / (size_t) n_threads;
            for (size_t k = lo; k < hi; k++) { volatile char *q = base + std::min(k * page, bytes - 1); *q = 0; }
        });
    for (auto &t : th) t.join();
}

// the arguments of the estimates kernel after an iteration with want_estimates: gene g goes to out + ooff[g], or, ooff
// null, to where its coverage lies in the packed layout
static dn::EstArgs est_args(dn_handle h, double *out, const int64_t *ooff)
{
    dn::EstArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cov = h->data.d_cov; a.goff = h->data.d_goff; a.glen = h->data.d_glen; a.kfin = h->data.d_kfin; a.emode = h->data.d_emode;
    a.svec = h->data.d_svec; a.svoff = h->data.d_svoff; a.out = out; a.ooff = ooff; a.n_genes = (int32_t) h->n; a.p = h->p;
    if (!h->ks->est_ptr) for (int i = 0; i < dn::P_MAX; i++) a.scale[i] = i < h->p ? h->last_scale[i] : 1.0;
    return a;
}

// the estimates kernel of the handle's kernel set; the wide-cohort set reads the scale factors of the last iteration from d_scales
static void launch_estimates(dn_handle h, const dn::EstArgs &a, const int32_t *tg, const int32_t *tc, int n_tiles)
{
    if (h->ks->est_ptr) h->ks->est_ptr(a, h->data.d_scales, tg, tc, n_tiles, h->stream[0]);
    else h->ks->est(a, tg, tc, n_tiles, h->stream[0]);
}

int dn_fetch_estimates(dn_handle h, double *out)
{
    if (!h || !h->data.d_cov) return fail(DN_E_STATE, "dn_fetch_estimates: nothing uploaded");
    if (!h->data.have_estimate_state) return fail(DN_E_STATE, "dn_fetch_estimates: last iteration did not run with want_estimates = 1");
    if (!out) return fail(DN_E_INVALID, "dn_fetch_estimates: null output");
    return on_main_stream(h, [&]() -> int {
        if (!h->data.d_est) DN_TRY(h->data.d_est.alloc(sizeof(double) * (size_t) h->total));
        launch_estimates(h, est_args(h, h->data.d_est, nullptr), h->data.d_tile_gene, h->data.d_tile_col, (int) h->n_tiles);
        DN_TRY(hipGetLastError());
        prefault_pages(out, sizeof(double) * (size_t) h->total, (int) std::thread::hardware_concurrency());     // while the kernel runs
        DN_TRY(hipMemcpyAsync(out, h->data.d_est, sizeof(double) * (size_t) h->total, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

int dn_fetch_estimates_subset(dn_handle h, int64_t n_sel, const int64_t *gene_ids, double *out)
{
    if (!h || !h->data.d_cov) return fail(DN_E_STATE, "dn_fetch_estimates_subset: nothing uploaded");
    if (!h->data.have_estimate_state) return fail(DN_E_STATE, "dn_fetch_estimates_subset: last iteration did not run with want_estimates = 1");
    if (n_sel <= 0 || !gene_ids || !out) return fail(DN_E_INVALID, "dn_fetch_estimates_subset: bad argument");
    std::vector<int64_t> ooff(h->n, -1);
    std::vector<int32_t> tg, tc;
    const char *what = "dn_fetch_estimates_subset";
    dn::DeviceBuffer<double> d_out;
    dn::DeviceBuffer<int64_t> d_ooff;
    dn::DeviceBuffer<int32_t> d_tg, d_tc;
    return on_main_stream(h, [&]() -> int {
        int64_t total = 0;
        for (int64_t k = 0; k < n_sel; k++) {
            const int64_t g = gene_ids[k];
            if (g < 0 || g >= h->n) return fail(DN_E_INVALID, "dn_fetch_estimates_subset: gene id out of range");
            if (ooff[g] >= 0) return fail(DN_E_INVALID, "dn_fetch_estimates_subset: duplicate gene id");
            ooff[g] = total;
            total += (int64_t) h->p * h->glen[g];
            add_tiles(tg, tc, g, h->glen[g]);
        }
        DN_TRY_AS(what, d_out.alloc(sizeof(double) * (size_t) total));
        DN_TRY_AS(what, d_ooff.alloc(sizeof(int64_t) * (size_t) h->n));
        DN_TRY_AS(what, d_tg.alloc(sizeof(int32_t) * tg.size()));
        DN_TRY_AS(what, d_tc.alloc(sizeof(int32_t) * tc.size()));
        DN_TRY_AS(what, hipMemcpyAsync(d_ooff, ooff.data(), sizeof(int64_t) * (size_t) h->n, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY_AS(what, hipMemcpyAsync(d_tg, tg.data(), sizeof(int32_t) * tg.size(), hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY_AS(what, hipMemcpyAsync(d_tc, tc.data(), sizeof(int32_t) * tc.size(), hipMemcpyHostToDevice, h->stream[0]));
        launch_estimates(h, est_args(h, d_out, d_ooff), d_tg, d_tc, (int) tg.size());
        DN_TRY_AS(what, hipGetLastError());
        DN_TRY_AS(what, hipMemcpyAsync(out, d_out, sizeof(double) * (size_t) total, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY_AS(what, hipStreamSynchronize(h->stream[0]));
        return DN_OK;
    });
}

int dn_nmf_f64(dn_handle h, int64_t n, int32_t p, const double *const *x, const int64_t *lengths, int32_t mode,
               int32_t nmf_iter, double *K, double *E, double *est, int32_t *status)
{
    { const int rc = check_f64_batch(h, n, p, x, lengths, "dn_nmf_f64"); if (rc != DN_OK) return rc; }
    if (!K || !E || !status) return fail(DN_E_INVALID, "dn_nmf_f64: null output");
    if (mode != DN_NMF_RANK_ONE && mode != DN_NMF && mode != DN_NMF_RATIO) return fail(DN_E_INVALID, "dn_nmf_f64: unknown mode");
    if (mode == DN_NMF && nmf_iter < 0) return fail(DN_E_INVALID, "dn_nmf_f64: nmf_iter must be >= 0");
    std::vector<int64_t> xoff, eoff;
    std::vector<int32_t> ncol, order;                                 // widest first
    std::vector<double> packed;
    dn::DeviceBuffer<double> d_x, d_K, d_E, d_est;
    dn::DeviceBuffer<int64_t> d_xoff, d_eoff;
    dn::DeviceBuffer<int32_t> d_ncol, d_order, d_counter, d_status;
    dn::DeviceBuffer<char> d_ws;
    dn::Event e0, e1;
    return on_main_stream(h, [&]() -> int {
        const int64_t maxn = pack_f64(n, p, x, lengths, xoff, eoff, ncol, order, packed), total = xoff[n];
        // slot: x + lambda [p][n], residual profile, s_start, A^T u [n] -- fp64, 256-byte aligned
        const int64_t slot_bytes = ((int64_t) sizeof(double) * (p + 3) * maxn + 255) & ~(int64_t) 255;
        const int grid = f64_grid(h, 1, n, slot_bytes);
        if (grid < 1) return fail(DN_E_INVALID, "dn_nmf_f64: " + g_err);
        DN_TRY(alloc_f64(d_x, (size_t) total));
        DN_TRY(alloc_f64(d_xoff, (size_t) n));
        DN_TRY(alloc_f64(d_eoff, (size_t) n));
        DN_TRY(alloc_f64(d_ncol, (size_t) n));
        DN_TRY(alloc_f64(d_order, (size_t) n));
        DN_TRY(alloc_f64(d_counter, 4));
        DN_TRY(alloc_f64(d_status, (size_t) n));
        DN_TRY(alloc_f64(d_K, (size_t) n * p));
        DN_TRY(alloc_f64(d_E, (size_t) eoff[n]));
        if (est) DN_TRY(alloc_f64(d_est, (size_t) total));
        DN_TRY(alloc_f64(d_ws, (size_t) slot_bytes * (size_t) grid));
        DN_TRY(e0.create(hipEventCreate));
        DN_TRY(e1.create(hipEventCreate));
        DN_TRY(hipMemcpyAsync(d_x, packed.data(), sizeof(double) * (size_t) total, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(d_xoff, xoff.data(), sizeof(int64_t) * (size_t) n, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(d_eoff, eoff.data(), sizeof(int64_t) * (size_t) n, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(d_ncol, ncol.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemsetAsync(d_counter, 0, sizeof(int32_t) * 4, h->stream[0]));
        dn::NmfArgsF64 a;
        std::memset(&a, 0, sizeof(a));
        a.x = d_x; a.xoff = d_xoff; a.ncol = d_ncol; a.eoff = d_eoff; a.order = d_order; a.counter = d_counter;
        a.K = d_K; a.E = d_E; a.est = d_est; a.status = d_status; a.ws = d_ws; a.slot_bytes = slot_bytes;
        a.n = (int32_t) n; a.p = p; a.T = mode == DN_NMF ? nmf_iter : 0; a.ratio = mode == DN_NMF_RATIO ? 1 : 0;
        a.max_steps = h->max_steps;
        DN_TRY(hipEventRecord(e0, h->stream[0]));
        const int lrc = dn::launch_nmf_f64(a, grid, h->stream[0]);
        if (lrc != 0) return fail(DN_E_HIP, std::string("k_nmf_f64 launch: ") + hipGetErrorString((hipError_t) lrc));
        DN_TRY(hipEventRecord(e1, h->stream[0]));
        DN_TRY(hipMemcpyAsync(K, d_K, sizeof(double) * (size_t) n * p, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipMemcpyAsync(E, d_E, sizeof(double) * (size_t) eoff[n], hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToHost, h->stream[0]));
        if (est) DN_TRY(hipMemcpyAsync(est, d_est, sizeof(double) * (size_t) total, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        DN_TRY(hipEventElapsedTime(&h->last_f64_ms, e0, e1));
        return DN_OK;
    });
}

int dn_baseline_selection_f64(dn_handle h, int64_t n, int32_t p, const double *const *F, const int64_t *lengths,
                              const dn_params *prm, const int64_t *ds_start, double *rho, int32_t *flags,
                              int32_t *trace, double *est)
{
    { const int rc = check_f64_batch(h, n, p, F, lengths, "dn_baseline_selection_f64"); if (rc != DN_OK) return rc; }
    if (!prm || !rho || !flags) return fail(DN_E_INVALID, "dn_baseline_selection_f64: null argument");
    { const int rc = check_params(prm, ds_start, n, [&](int64_t g) { return lengths[g]; }); if (rc != DN_OK) return rc; }
    std::vector<int64_t> goff, svoff;
    std::vector<int32_t> glen, order, tg, tc;                         // order: longest first
    std::vector<double> packed;
    dn::DeviceBuffer<double> d_cov, d_rowmax, d_rho, d_kfin, d_svec, d_est;
    dn::DeviceBuffer<int64_t> d_goff, d_ds, d_svoff;
    dn::DeviceBuffer<int32_t> d_glen, d_order, d_counter, d_flags, d_trace, d_emode, d_tg, d_tc;
    dn::DeviceBuffer<char> d_ws;
    dn::Event e0, e1;
    return on_main_stream(h, [&]() -> int {
        const int64_t maxl = pack_f64(n, p, F, lengths, goff, svoff, glen, order, packed), total = goff[n];
        if (est)
            for (int64_t g = 0; g < n; g++) add_tiles(tg, tc, g, glen[g]);
        // slot: Fs, Fb (fp64, p x S) + x + lambda (fp64 [p][S]) + s_start, residual profile, A^T u (fp64 [S])
        const int32_t S = (int32_t) ((maxl + 63) & ~(int64_t) 63);
        const int64_t slot_bytes = (int64_t) S * ((int64_t) p * 3 * sizeof(double) + 3 * sizeof(double));
        const int grid = f64_grid(h, 0, n, slot_bytes);
        if (grid < 1) return fail(DN_E_INVALID, "dn_baseline_selection_f64: " + g_err);
        DN_TRY(alloc_f64(d_cov, (size_t) total));
        DN_TRY(alloc_f64(d_goff, (size_t) n + 1));
        DN_TRY(alloc_f64(d_glen, (size_t) n));
        DN_TRY(alloc_f64(d_order, (size_t) n));
        DN_TRY(alloc_f64(d_counter, 4));
        DN_TRY(alloc_f64(d_rowmax, (size_t) n * p));
        DN_TRY(alloc_f64(d_rho, (size_t) n * p));
        DN_TRY(alloc_f64(d_flags, (size_t) n));
        DN_TRY(alloc_f64(d_trace, (size_t) n * dn::TRACE_LEN));
        DN_TRY(alloc_f64(d_kfin, (size_t) n * p));
        DN_TRY(alloc_f64(d_emode, (size_t) n));
        DN_TRY(alloc_f64(d_ws, (size_t) slot_bytes * (size_t) grid));
        if (prm->downsample_rate > 1) DN_TRY(alloc_f64(d_ds, (size_t) n));
        if (est) {
            DN_TRY(alloc_f64(d_svoff, (size_t) n + 1));
            DN_TRY(alloc_f64(d_svec, (size_t) svoff[n]));
            DN_TRY(alloc_f64(d_est, (size_t) total));
            DN_TRY(alloc_f64(d_tg, tg.size()));
            DN_TRY(alloc_f64(d_tc, tc.size()));
        }
        DN_TRY(e0.create(hipEventCreate));
        DN_TRY(e1.create(hipEventCreate));
        DN_TRY(hipMemcpyAsync(d_cov, packed.data(), sizeof(double) * (size_t) total, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(d_goff, goff.data(), sizeof(int64_t) * (size_t) (n + 1), hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(d_glen, glen.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, h->stream[0]));
        DN_TRY(hipMemsetAsync(d_counter, 0, sizeof(int32_t) * 4, h->stream[0]));
        DN_TRY(hipMemsetAsync(d_trace, 0, sizeof(int32_t) * (size_t) n * dn::TRACE_LEN, h->stream[0]));
        if (d_ds) DN_TRY(hipMemcpyAsync(d_ds, ds_start, sizeof(int64_t) * (size_t) n, hipMemcpyHostToDevice, h->stream[0]));
        if (est) {
            DN_TRY(hipMemcpyAsync(d_svoff, svoff.data(), sizeof(int64_t) * (size_t) (n + 1), hipMemcpyHostToDevice, h->stream[0]));
            DN_TRY(hipMemcpyAsync(d_tg, tg.data(), sizeof(int32_t) * tg.size(), hipMemcpyHostToDevice, h->stream[0]));
            DN_TRY(hipMemcpyAsync(d_tc, tc.data(), sizeof(int32_t) * tc.size(), hipMemcpyHostToDevice, h->stream[0]));
        }
        DN_TRY(hipEventRecord(e0, h->stream[0]));
        int lrc = dn::launch_row_max_f64(d_cov, d_goff, d_glen, d_rowmax, (int) n, p,
                                         (int) std::min<int64_t>(n, (int64_t) h->n_cus * 8), h->stream[0]);
        if (lrc != 0) return fail(DN_E_HIP, std::string("k_row_max_f64 launch: ") + hipGetErrorString((hipError_t) lrc));
        dn::IterArgsF64 a;
        std::memset(&a, 0, sizeof(a));
        a.cov = d_cov; a.goff = d_goff; a.glen = d_glen; a.order = d_order; a.counter = d_counter; a.ds_start = d_ds;
        a.rowmax = d_rowmax; a.x16 = nullptr; a.ws = d_ws; a.rho = d_rho; a.flags = d_flags; a.trace = d_trace; a.kfin = d_kfin;
        a.emode = d_emode; a.svec = d_svec; a.svoff = d_svoff; a.slot_bytes = slot_bytes; a.n_genes = (int32_t) n; a.S = S;
        a.lds_cols = 0; a.T = prm->nmf_iter; a.bins = prm->bins; a.min_hc = prm->min_high_coverage; a.rate = prm->downsample_rate;
        a.skip = prm->skip_baseline_selection ? 1 : 0; a.want_est = est ? 1 : 0; a.p = p; a.max_steps = h->max_steps;
        for (int i = 0; i < dn::P_MAX; i++) { a.scale[i] = 1.0; a.inv_scale[i] = 1.0; }      // F as given
        lrc = dn::launch_baseline_f64(a, grid, h->stream[0]);
        if (lrc != 0) return fail(DN_E_HIP, std::string("k_baseline_gen (float64) launch: ") + hipGetErrorString((hipError_t) lrc));
        if (est) {
            dn::EstArgsF64 e;
            std::memset(&e, 0, sizeof(e));
            e.cov = d_cov; e.goff = d_goff; e.glen = d_glen; e.kfin = d_kfin; e.emode = d_emode; e.svec = d_svec; e.svoff = d_svoff;
            e.out = d_est; e.ooff = nullptr; e.n_genes = (int32_t) n; e.p = p;
            for (int i = 0; i < dn::P_MAX; i++) e.scale[i] = 1.0;
            lrc = dn::launch_est_f64(e, d_tg, d_tc, (int) tg.size(), h->stream[0]);
            if (lrc != 0) return fail(DN_E_HIP, std::string("k_estimates_gen (float64) launch: ") + hipGetErrorString((hipError_t) lrc));
        }
        DN_TRY(hipEventRecord(e1, h->stream[0]));
        DN_TRY(hipMemcpyAsync(rho, d_rho, sizeof(double) * (size_t) n * p, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipMemcpyAsync(flags, d_flags, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToHost, h->stream[0]));
        if (trace) DN_TRY(hipMemcpyAsync(trace, d_trace, sizeof(int32_t) * (size_t) n * dn::TRACE_LEN, hipMemcpyDeviceToHost, h->stream[0]));
        if (est) DN_TRY(hipMemcpyAsync(est, d_est, sizeof(double) * (size_t) total, hipMemcpyDeviceToHost, h->stream[0]));
        DN_TRY(hipStreamSynchronize(h->stream[0]));
        DN_TRY(hipEventElapsedTime(&h->last_f64_ms, e0, e1));
        return DN_OK;
    });
}

double dn_last_f64_ms(dn_handle h) { return h ? (double) h->last_f64_ms : 0.0; }

double dn_last_kernel_ms(dn_handle h) { return h ? (double) h->last_ms : 0.0; }
double dn_last_init_ms(dn_handle h) { return h ? (double) h->last_init_ms : 0.0; }
double dn_last_span_ms(dn_handle h) { return h ? (double) h->last_span_ms : 0.0; }
double dn_last_rowmax_ms(dn_handle h) { return h ? (double) h->last_rowmax_ms : 0.0; }
const char *dn_init_kernel_name(dn_handle h) { return h ? h->init_name : ""; }
const char *dn_main_kernel_name(dn_handle h) { return (h && h->ks) ? h->ks->baseline_name : ""; }
double dn_class_kernel_ms(dn_handle h, int cls) { return (h && cls >= 0 && cls < dn_handle_s::NCLS) ? (double) h->data.cls[cls].last_ms : 0.0; }
const char *dn_class_kernel_name(dn_handle h, int cls) { return (h && cls >= 0 && cls < dn_handle_s::NCLS && h->data.cls[cls].ks && h->data.cls[cls].n > 0) ? h->data.cls[cls].ks->baseline_name : ""; }
int32_t dn_tiny_length(dn_handle h) { return h ? h->tiny_len : 0; }

int dn_handdown(dn_handle h, int cls, int32_t *cols, int32_t *parked)
{
    if (!h || !cols || !parked) return fail(DN_E_INVALID, "dn_handdown: null argument");
    if (cls < 0 || cls >= dn_handle_s::NCLS) return fail(DN_E_INVALID, "dn_handdown: no such class");
    *cols = h->data.cls[cls].hand_cols;
    *parked = h->data.cls[cls].parked;
    return DN_OK;
}
int dn_class_tier_cols(dn_handle h, int cls, int32_t *reg_cols, int32_t *lds_cols)
{
    if (!h || cls < 0 || cls >= dn_handle_s::NCLS || !reg_cols || !lds_cols) return fail(DN_E_INVALID, "dn_class_tier_cols: bad argument");
    const auto &C = h->data.cls[cls];
    const bool live = C.ks && C.n > 0;
    *reg_cols = live ? C.ks->reg_tier_cols : 0;
    *lds_cols = live ? C.lds_cols : 0;
    return DN_OK;
}
int dn_class_lengths(dn_handle h, int32_t p, int32_t downsample_rate, int32_t *split_len, int32_t *tiny_len)
{
    if (!h || !split_len || !tiny_len) return fail(DN_E_INVALID, "dn_class_lengths: null argument");
    const dn::KernelSet *ks = dn::kernel_set_for(p);
    if (!ks) return fail(DN_E_UNSUPPORTED, "no kernels compiled for p = " + std::to_string(p));
    DN_TRY(hipSetDevice(h->device));
    *split_len = 0; *tiny_len = 0;
    if (downsample_rate > 1 && p >= 8) return DN_OK;        // the one-wavefront-per-gene family of the down-sampled regime has one class
    const dn::KernelSet *pair = nullptr;
    class_lengths(ks, p, *split_len, *tiny_len, pair);
    return DN_OK;
}
int32_t dn_split_length(dn_handle h) { return h ? h->split_len : 0; }
int dn_synchronize(dn_handle h)
{
    if (!h) return fail(DN_E_INVALID, "null handle");
    DN_TRY(hipSetDevice(h->device));
    DN_TRY(hipStreamSynchronize(h->stream[0]));
    return DN_OK;
}

}  // extern "C"

// stream-copy ceiling ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_copy4(const float4 *__restrict__ src, float4 *__restrict__ dst, size_t n4)
{
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t) gridDim.x * blockDim.x) dst[i] = src[i];
}

// read-only stream: every lane keeps four 16-byte loads in flight and folds them into one number (nothing is written but a
// few partial sums): the ceiling a streaming READ kernel can reach on this device ("measured stream-read ceiling")
__global__ __launch_bounds__(256) void k_read4(const float4 *__restrict__ src, float *__restrict__ sink, size_t n4)
{
    float acc = 0.f;
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const float4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        acc += (a.x + a.y + a.z + a.w) + (b.x + b.y + b.z + b.w) + (c.x + c.y + c.z + c.w) + (d.x + d.y + d.z + d.w);
    }
    for (; i < n4; i += stride) { const float4 a = src[i]; acc += a.x + a.y + a.z + a.w; }
    if (acc == 12345.678f) sink[0] = acc;                  // never true for the memset pattern: keeps the loads alive
}

// the same with eight non-temporal 16-byte loads per lane in flight
__global__ __launch_bounds__(256) void k_read8nt(const float4 *__restrict__ src, float *__restrict__ sink, size_t n4)
{
    float acc = 0.f;
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 7 * stride < n4; i += 8 * stride) {
        typedef float vf4 __attribute__((ext_vector_type(4)));
        vf4 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(src + i + k * stride));
#pragma unroll
        for (int k = 0; k < 8; k++) acc += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    }
    for (; i < n4; i += stride) { const float4 a = src[i]; acc += a.x + a.y + a.z + a.w; }
    if (acc == 12345.678f) sink[0] = acc;
}

// Best GB/s over `reps` timed launches (one more, the first, is not counted) of a kernel that moves `bytes` per launch; the
// launches run on the handle's stream between its class-0 events, one at a time
template <class Launch> static double best_gbps(dn_handle h, int reps, double bytes, Launch launch)
{
    double best = 0.0;
    for (int r = 0; r < reps + 1; r++) {
        (void) hipEventRecord(h->ev_start[0], h->stream[0]);
        launch();
        (void) hipEventRecord(h->ev_end[0], h->stream[0]);
        (void) hipStreamSynchronize(h->stream[0]);
        float ms = 0.f;
        (void) hipEventElapsedTime(&ms, h->ev_start[0], h->ev_end[0]);
        if (r > 0 && ms > 0.f) best = std::max(best, bytes / (ms * 1e-3) / 1e9);
    }
    return best;
}

extern "C" double dn_measure_read_gbps(dn_handle h, int64_t bytes, int reps)
{
    if (!h || bytes < (1 << 20)) return 0.0;
    if (hipSetDevice(h->device) != hipSuccess) return 0.0;
    dn::DeviceBuffer<float4> a;
    dn::DeviceBuffer<float> sink;
    const size_t n4 = (size_t) bytes / sizeof(float4);
    if (a.alloc(n4 * sizeof(float4)) != hipSuccess || sink.alloc(256) != hipSuccess) return 0.0;
    double best = 0.0;
    (void) dn::synced(h->stream[0], [&]() -> int {
        (void) hipMemsetAsync(a, 1, n4 * sizeof(float4), h->stream[0]);
        for (int mult : {4, 8, 16, 32}) {                      // workgroups per CU: the best grid is the ceiling
            const double b4 = best_gbps(h, reps, (double) n4 * sizeof(float4), [&]() { hipLaunchKernelGGL(k_read4, dim3(h->n_cus * mult), dim3(256), 0, h->stream[0], a, sink, n4); });
            const double b8 = best_gbps(h, reps, (double) n4 * sizeof(float4), [&]() { hipLaunchKernelGGL(k_read8nt, dim3(h->n_cus * mult), dim3(256), 0, h->stream[0], a, sink, n4); });
            best = std::max(best, std::max(b4, b8));
        }
        return DN_OK;
    });
    return best;
}

extern "C" double dn_measure_copy_gbps(dn_handle h, int64_t bytes, int reps)
{
    if (!h || bytes < (1 << 20)) return 0.0;
    if (hipSetDevice(h->device) != hipSuccess) return 0.0;
    dn::DeviceBuffer<float4> a, b;
    const size_t n4 = (size_t) bytes / sizeof(float4);
    if (a.alloc(n4 * sizeof(float4)) != hipSuccess || b.alloc(n4 * sizeof(float4)) != hipSuccess) return 0.0;
    double best = 0.0;
    (void) dn::synced(h->stream[0], [&]() -> int {
        (void) hipMemsetAsync(a, 1, n4 * sizeof(float4), h->stream[0]);
        best = best_gbps(h, reps, 2.0 * (double) n4 * sizeof(float4), [&]() { hipLaunchKernelGGL(k_copy4, dim3(h->n_cus * 8), dim3(256), 0, h->stream[0], a, b, n4); });
        return DN_OK;
    });
    return best;
}
