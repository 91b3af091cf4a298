// dn_gz.hip -- gzip members (RFC 1952) inflated chunk by chunk: guess, walk, stitch, fix up, propagate windows, emit.
// include/degnorm_amd.h ("gzip streams") is the definition; DESIGN.md ("gzip inflate") has the LDS layouts and the argument
// why the stitch equals the serial decode.
//
// The decoder is the library's one (dn_inflate_core.hpp): inflate_span from any bit, with a stop rule (one block, a bit to
// reach, a guess to meet), a history of `have` bytes behind the entry and a 64-bit output position, against HostMem (plain
// arrays, lane after lane: the build that is tested and sanitised without a device) or WaveMem (one wave; LDS: 2 KiB of
// input, the tables, and the ring: none / 64 KiB of markers / 32 KiB of bytes).
//
// The stitch (Gz::next) is host code over a Backend: the host one runs the routines in loops, the device one launches
// k_gz_guess, k_gz_walk, k_gz_windows and k_gz_emit.  Input is untrusted.  Every read of the compressed bytes is bounded by
// the span (bytes beyond it read as zero and are counted as an overrun), every ring index is masked, a tail or a window has
// a slot that the host counted, and the emit never leaves the length its walk measured (`limit`).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/degnorm_amd.h"
#include "dn_host.hpp"
#include "dn_gz.hpp"

#define DN_HD __host__ __device__ __forceinline__
#include "dn_inflate_core.hpp"

namespace {

using dn::gz::Unit;
using dn::gz::Emit;
using dn::gz::EmitResult;
template <int kMode> using SpanHost = HostMem<kMode, int64_t>;      // a gzip segment is counted in 64 bits
template <int kMode> using SpanWave = WaveMem<kMode, int64_t>;

// rules 1 and 2 of a guess on the 96 bits at a bit offset (lo: the first 64, hi: the next 32); left: the bits from there to
// the end of the span
DN_HD bool guess_header(uint64_t lo, uint32_t hi, int64_t left)
{
    if (left < 17 || (lo & 7u) != 4u) return false;
    if (((lo >> 3) & 31u) > 29u || ((lo >> 8) & 31u) > 29u) return false;
    const int n_cl = (int) ((lo >> 13) & 15u) + 4;
    if (17 + 3 * n_cl > left) return false;
    int kraft = 0;
    for (int i = 0; i < n_cl; i++) {
        const int q = 17 + 3 * i;
        const uint32_t l = (q >= 64 ? hi >> (q - 64) : (uint32_t) (lo >> q) | (q > 32 ? hi << (64 - q) : 0u)) & 7u;
        if (l) kraft += 128 >> l;
    }
    return kraft == 128;
}

template <class M> DN_HD bool guess_candidate(M &m, int64_t b, int32_t n_in)        // the words of b's step are in reach
{
    const int32_t q = (int32_t) ((b >> 5) << 2);
    const int s = (int) (b & 31);
    const uint64_t w01 = (uint64_t) m.word(q, n_in) | ((uint64_t) m.word(q + 4, n_in) << 32);
    const uint64_t w23 = (uint64_t) m.word(q + 8, n_in) | ((uint64_t) m.word(q + 12, n_in) << 32);
    const uint64_t lo = s ? (w01 >> s) | (w23 << (64 - s)) : w01;
    return guess_header(lo, (uint32_t) (w23 >> s), (int64_t) n_in * 8 - b);
}

// rules 3 .. 6 (and again 1 and 2, through the decoder) at bit b
template <class M> DN_HD bool guess_block(M &m, const Tables &t, int32_t n_in, int64_t b)
{
    BitReader r;
    r.n_in = n_in;
    seek_bit(r, m, b);
    refill(r, m);
    if (take(r, 3) != 4u) return false;
    int n_lit, n_dist;
    if (read_dynamic(r, m, t, n_lit, n_dist)) return false;
    if (build_table(m, t.lens, n_lit, t.cnt_l, t.sym_l, t.offs, t.lit, kLitBits, true) || !complete(t.cnt_l)) return false;
    if (build_table(m, t.lens + n_lit, n_dist, t.cnt_d, t.sym_d, t.offs, t.dist, kDistBits, true)) return false;
    int64_t out_pos = 0;
    if (symbols(r, m, t, n_in, out_pos, (int64_t) kHist, kNoLimit, false)) return false;
    m.ensure_in(r.next, kSymbolBytes, n_in);
    refill(r, m);
    const uint32_t next = take(r, 3);
    return !overrun(r) && (next >> 1) != 3u;
}

struct HostTables {
    uint16_t lit[1 << kLitBits], dist[1 << kDistBits], sym_l[288], sym_d[32], cnt_l[16], cnt_d[16], offs[16];
    uint8_t lens[320];
    Tables get() { return Tables{lit, dist, sym_l, sym_d, cnt_l, cnt_d, offs, lens}; }
};

#define DN_GZ_SHARED_TABLES                                                                                                          \
    __shared__ __attribute__((aligned(16))) uint32_t s_win[kWin / 4];                                                                \
    __shared__ uint16_t s_lit[1 << kLitBits], s_dist[1 << kDistBits], s_sym_l[288], s_sym_d[32], s_cnt_l[16], s_cnt_d[16], s_offs[16]; \
    __shared__ uint8_t s_lens[320];                                                                                                  \
    const Tables t{s_lit, s_dist, s_sym_l, s_sym_d, s_cnt_l, s_cnt_d, s_offs, s_lens}

template <int kMode> __device__ __forceinline__ SpanWave<kMode> make_wave(typename SpanWave<kMode>::Sym *ring, uint32_t *win, const uint8_t *comp, int64_t comp_cap)
{
    SpanWave<kMode> m;
    m.ring = ring; m.win = win; m.comp = comp; m.comp_cap = comp_cap;
    m.abs0 = 0; m.wbase = -4 * (int64_t) kWin;
    m.lane = (int) threadIdx.x;
    m.skip = 0; m.keep = 0;
    m.dst = nullptr; m.tail = nullptr; m.flushed = 0; m.check = false; m.crc = 0;
    return m;
}

// guess[k] = the smallest bit of chunk k that passes the guess rule, or -1
__global__ __launch_bounds__(64) void k_gz_guess(const uint8_t *__restrict__ comp, int64_t comp_cap, int32_t n_in, int64_t n_chunks, int32_t shift,
                                                 int64_t *__restrict__ guess)
{
    DN_GZ_SHARED_TABLES;
    const int64_t k = blockIdx.x;
    if (k >= n_chunks) return;
    SpanWave<kTrial> m = make_wave<kTrial>(nullptr, s_win, comp, comp_cap);
    const int64_t lo = k << shift, end = (int64_t) n_in * 8;
    const int64_t hi = ((k + 1) << shift) < end ? ((k + 1) << shift) : end;
    int64_t g = -1;
    for (int64_t b0 = lo; b0 < hi && g < 0; b0 += 64) {
        m.ensure_in((int32_t) (b0 >> 3), 32, n_in);
        const int64_t b = b0 + m.lane;
        unsigned long long mask = __ballot(b < hi && guess_candidate(m, b, n_in));
        while (mask) {
            const int j = __ffsll(mask) - 1;
            mask &= mask - 1;
            if (guess_block(m, t, n_in, b0 + j)) { g = b0 + j; break; }
        }
    }
    if (threadIdx.x == 0) guess[k] = g;
}

// units == nullptr: workgroup k walks chunk k from its guess to the first block end at or beyond the chunk's end (slot k).
// Otherwise workgroup k walks units[k], a fix-up.
__global__ __launch_bounds__(64) void k_gz_walk(const uint8_t *__restrict__ comp, int64_t comp_cap, int32_t n_in, const int64_t *__restrict__ guess,
                                                int64_t n_chunks, int32_t shift, const Unit *__restrict__ units, int64_t n_units,
                                                Segment *__restrict__ res, uint16_t *__restrict__ tails)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_ring[kHist];
    DN_GZ_SHARED_TABLES;
    const int64_t k = blockIdx.x;
    if (k >= (units ? n_units : n_chunks)) return;
    Stop stop{Stop::kReach, shift, (k + 1) << shift, guess, n_chunks};
    int64_t entry = 0, slot = k;
    if (units) { entry = units[k].entry; slot = units[k].slot; stop.mode = Stop::kGuess; }
    else entry = guess[k];
    if (entry < 0) {
        if (threadIdx.x == 0) res[slot] = Segment{-1, -1, 0, 0, 0, -1, 0};
        return;
    }
    for (int j = (int) threadIdx.x; j < kHist; j += 64) s_ring[j] = (uint16_t) (0x8000 | j);
    SpanWave<kMarkers> m = make_wave<kMarkers>(s_ring, s_win, comp, comp_cap);
    m.tail = tails + slot * kHist;
    m.fence();
    Segment o;
    inflate_span(m, t, n_in, entry, stop, kHist, kNoLimit, o);
    if (threadIdx.x == 0) res[slot] = o;
}

// wins[s] = the window of chain segment s: zero at a member's first segment, else the window before it seen through the
// tail of the segment before it.  wins[0] arrives filled (the bytes carried from the span before).
__global__ __launch_bounds__(1024) void k_gz_windows(const uint16_t *__restrict__ tails, const Emit *__restrict__ chain, int64_t n_seg,
                                                     uint8_t *__restrict__ wins)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][kHist];
    const int tid = (int) threadIdx.x;
    if (n_seg <= 0) return;
    const bool zero0 = chain[0].reset != 0;
    for (int j = tid; j < kHist; j += 1024) {
        const uint8_t v = zero0 ? (uint8_t) 0 : wins[j];
        s_w[0][j] = v;
        if (zero0) wins[j] = 0;
    }
    for (int64_t s = 1; s < n_seg; s++) {
        __syncthreads();
        const uint8_t *src = s_w[(s - 1) & 1];
        uint8_t *dst = s_w[s & 1];
        const bool zero = chain[s].reset != 0;
        const uint16_t *tail = tails + (int64_t) chain[s - 1].slot * kHist;
        uint8_t *w = wins + s * kHist;
        for (int v = tid; v < kHist / 8; v += 1024) {
            const uint4 q = reinterpret_cast<const uint4 *>(tail)[v];
            const uint32_t in[4] = {q.x, q.y, q.z, q.w};
            uint32_t o[2] = {0, 0};
            for (int k = 0; k < 8 && !zero; k++) {
                const uint32_t sym = (in[k >> 1] >> (16 * (k & 1))) & 0xffffu;
                const uint32_t b = sym < 256u ? sym : (uint32_t) src[sym & 0x7fffu];
                o[k >> 2] |= b << (8 * (k & 3));
            }
            reinterpret_cast<uint2 *>(dst)[v] = make_uint2(o[0], o[1]);
            reinterpret_cast<uint2 *>(w)[v] = make_uint2(o[0], o[1]);
        }
    }
}

__global__ __launch_bounds__(64) void k_gz_emit(const uint8_t *__restrict__ comp, int64_t comp_cap, int32_t n_in, const Emit *__restrict__ chain,
                                                int64_t n_seg, const uint8_t *__restrict__ wins, uint8_t *__restrict__ out, int32_t check,
                                                EmitResult *__restrict__ res)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[kHist];
    DN_GZ_SHARED_TABLES;
    const int64_t s = blockIdx.x;
    if (s >= n_seg) return;
    const Emit E = chain[s];
    for (int j = (int) threadIdx.x; j < kHist / 16; j += 64)
        reinterpret_cast<uint4 *>(s_ring)[j] = reinterpret_cast<const uint4 *>(wins + s * kHist)[j];
    SpanWave<kBytes> m = make_wave<kBytes>(s_ring, s_win, comp, comp_cap);
    m.dst = out + E.out_off;
    m.keep = E.out_len;
    m.check = check != 0;
    m.fence();
    const Stop stop{Stop::kReach, 0, E.exit, nullptr, 0};
    Segment o;
    inflate_span(m, t, n_in, E.entry, stop, E.have, E.out_len, o);
    if (o.status == 0 && (o.exit != E.exit || o.out_len != E.out_len || o.kind != E.kind)) o.status = DN_INFLATE_E_SIZE;
    if (threadIdx.x == 0) res[s] = EmitResult{m.crc, o.status};
}

// --- the two builds behind the stitch -----------------------------------------------------------------------------------------

int bad(const std::string &msg) { return dn::fail(DN_E_INVALID, msg); }

struct Backend {
    double ms[6] = {0, 0, 0, 0, 0, 0};       // copy, guess, walk, windows, emit, copy back
    virtual ~Backend() {}
    // take the span's bytes; guess its n_chunks chunks and walk the guessed ones (slot = chunk); room for n_slots tails
    virtual int scan(const uint8_t *span, int64_t n_span, int64_t n_chunks, int32_t shift, int64_t n_slots, std::vector<int64_t> &guess,
                     std::vector<Segment> &res) = 0;
    virtual int fixup(const Unit &u, Segment &res) = 0;
    // windows and emit of the chain; carry: the kHist bytes before the chain's first segment.  *out: total bytes, the backend's.
    virtual int emit(const std::vector<Emit> &chain, const uint8_t *carry, int64_t total, bool check, const uint8_t **out,
                     std::vector<EmitResult> &res) = 0;
};

struct HostBackend : Backend {
    const uint8_t *span = nullptr;
    int32_t n_in = 0, shift = 0;
    const std::vector<int64_t> *guess = nullptr;
    std::vector<uint16_t> tails, ring16;
    std::vector<uint8_t> out, ring8;
    HostTables tab;

    Segment walk(int64_t entry, const Stop &stop, int64_t slot)
    {
        ring16.resize(kHist);
        for (int j = 0; j < kHist; j++) ring16[(size_t) j] = (uint16_t) (0x8000 | j);
        SpanHost<kMarkers> m{span, ring16.data(), nullptr, tails.data() + slot * kHist, false};
        Segment o;
        inflate_span(m, tab.get(), n_in, entry, stop, kHist, kNoLimit, o);
        return o;
    }
    int scan(const uint8_t *bytes, int64_t n_span, int64_t n_chunks, int32_t sh, int64_t n_slots, std::vector<int64_t> &g, std::vector<Segment> &res) override
    {
        span = bytes; n_in = (int32_t) n_span; shift = sh; guess = &g;
        tails.resize((size_t) (n_slots * kHist));
        g.assign((size_t) n_chunks, -1);
        res.assign((size_t) n_chunks, Segment{-1, -1, 0, 0, 0, -1, 0});
        const Tables t = tab.get();
        for (int64_t k = 0; k < n_chunks; k++) {
            SpanHost<kTrial> m{span, nullptr, nullptr, nullptr, false};
            const int64_t lo = k << shift, end = n_span * 8, hi = ((k + 1) << shift) < end ? ((k + 1) << shift) : end;
            for (int64_t b = lo; b < hi; b++)
                if (guess_candidate(m, b, n_in) && guess_block(m, t, n_in, b)) { g[(size_t) k] = b; break; }
        }
        for (int64_t k = 0; k < n_chunks; k++)
            if (g[(size_t) k] >= 0) res[(size_t) k] = walk(g[(size_t) k], Stop{Stop::kReach, shift, (k + 1) << shift, g.data(), n_chunks}, k);
        return DN_OK;
    }
    int fixup(const Unit &u, Segment &res) override
    {
        res = walk(u.entry, Stop{Stop::kGuess, shift, 0, guess->data(), (int64_t) guess->size()}, u.slot);
        return DN_OK;
    }
    int emit(const std::vector<Emit> &chain, const uint8_t *carry, int64_t total, bool check, const uint8_t **out_bytes, std::vector<EmitResult> &res) override
    {
        out.resize((size_t) total);
        res.resize(chain.size());
        ring8.resize(kHist);
        std::vector<uint8_t> win(carry, carry + kHist), next((size_t) kHist);
        for (size_t s = 0; s < chain.size(); s++) {
            const Emit &E = chain[s];
            if (s > 0) {
                const uint16_t *tail = tails.data() + (int64_t) chain[s - 1].slot * kHist;
                for (int j = 0; j < kHist; j++) next[(size_t) j] = tail[j] < 256 ? (uint8_t) tail[j] : win[tail[j] & 0x7fff];
                win.swap(next);
            }
            if (E.reset) win.assign((size_t) kHist, 0);
            ring8 = win;
            SpanHost<kBytes> m{span, ring8.data(), out.data() + E.out_off, nullptr, check};
            Segment o;
            inflate_span(m, tab.get(), n_in, E.entry, Stop{Stop::kReach, 0, E.exit, nullptr, 0}, E.have, E.out_len, o);
            if (o.status == 0 && (o.exit != E.exit || o.out_len != E.out_len || o.kind != E.kind)) o.status = DN_INFLATE_E_SIZE;
            res[s] = EmitResult{m.crc, o.status};
        }
        *out_bytes = out.data();
        return DN_OK;
    }
};

struct DeviceBackend : Backend {
    int device;
    dn::Stream st;
    dn::Event e0, e1;
    dn::GrowBuffer<uint8_t> d_comp, d_out, d_wins;
    dn::GrowBuffer<uint16_t> d_tails;
    dn::GrowBuffer<int64_t> d_guess;
    dn::GrowBuffer<Segment> d_res;
    dn::GrowBuffer<Unit> d_unit;
    dn::GrowBuffer<Emit> d_chain;
    dn::GrowBuffer<EmitResult> d_eres;
    dn::PinnedBuffer<uint8_t> h_out;
    int64_t h_out_cap = 0, comp_cap = 0, n_chunks = 0, n_slots = 0;
    int32_t n_in = 0, shift = 0;

    explicit DeviceBackend(int dev) : device(dev) {}

    int init()
    {
        DN_TRY(hipSetDevice(device));
        DN_TRY(st.create(hipStreamCreate));
        DN_TRY(e0.create(hipEventCreate));
        DN_TRY(e1.create(hipEventCreate));
        return DN_OK;
    }
    // queue `work`, wait for it, add its time to ms[stage]
    template <class F> int timed(int stage, F work)
    {
        DN_TRY(hipEventRecord(e0, st));
        const int rc = work();
        if (rc != DN_OK) return rc;
        DN_TRY(hipEventRecord(e1, st));
        DN_TRY(hipStreamSynchronize(st));
        float t = 0.f;
        DN_TRY(hipEventElapsedTime(&t, e0, e1));
        ms[stage] += t;
        return DN_OK;
    }
    // bytes that buffers of `have` elements must still grow by to hold `need`
    template <class T> static int64_t growth(const dn::GrowBuffer<T> &b, int64_t need)
    {
        return need > b.cap ? (int64_t) sizeof(T) * dn::grown_capacity(b.cap, need) + 16 : 0;
    }
    int fits(int64_t more, const std::string &what)
    {
        size_t free_b = 0, total_b = 0;
        DN_TRY(hipMemGetInfo(&free_b, &total_b));
        if (more > 0 && (uint64_t) more + (64u << 20) > free_b)
            return bad("dn_gz_next: " + what + " needs " + std::to_string(more) + " more bytes of device memory, " + std::to_string(free_b) +
                       " are free: use smaller spans (window_bytes) or larger chunks (chunk_bytes)");
        return DN_OK;
    }

    int scan(const uint8_t *span, int64_t n_span, int64_t chunks, int32_t sh, int64_t slots, std::vector<int64_t> &guess, std::vector<Segment> &res) override
    {
        n_in = (int32_t) n_span; n_chunks = chunks; n_slots = slots; shift = sh;
        comp_cap = ((n_span + 15) & ~(int64_t) 15) + 16;
        guess.assign((size_t) chunks, -1);
        res.assign((size_t) slots, Segment{-1, -1, 0, 0, 0, -1, 0});
        DN_TRY(hipSetDevice(device));
        return dn::synced(st, [&]() -> int {
            const int64_t more = growth(d_comp, comp_cap) + growth(d_tails, slots * kHist) + growth(d_wins, slots * kHist) + growth(d_guess, chunks) +
                                 growth(d_res, slots);
            int rc = fits(more, "a span of " + std::to_string(n_span) + " compressed bytes in " + std::to_string(chunks) + " chunks");
            if (rc != DN_OK) return rc;
            DN_TRY(d_comp.reserve(comp_cap, 0, st)); DN_TRY(d_tails.reserve(slots * kHist, 0, st)); DN_TRY(d_wins.reserve(slots * kHist, 0, st));
            DN_TRY(d_guess.reserve(chunks, 0, st)); DN_TRY(d_res.reserve(slots, 0, st)); DN_TRY(d_unit.reserve(1, 0, st));
            rc = timed(0, [&]() -> int {
                DN_TRY(hipMemcpyAsync(d_comp, span, (size_t) n_span, hipMemcpyHostToDevice, st));
                DN_TRY(hipMemsetAsync(d_comp + n_span, 0, (size_t) (comp_cap - n_span), st));
                return DN_OK;
            });
            if (rc != DN_OK) return rc;
            rc = timed(1, [&]() -> int {
                hipLaunchKernelGGL(k_gz_guess, dim3((unsigned) chunks), dim3(64), 0, st, d_comp, comp_cap, n_in, chunks, shift, d_guess);
                DN_TRY(hipGetLastError());
                return DN_OK;
            });
            if (rc != DN_OK) return rc;
            rc = timed(2, [&]() -> int {
                hipLaunchKernelGGL(k_gz_walk, dim3((unsigned) chunks), dim3(64), 0, st, d_comp, comp_cap, n_in, d_guess, chunks, shift,
                                   (const Unit *) nullptr, (int64_t) 0, d_res, d_tails);
                DN_TRY(hipGetLastError());
                return DN_OK;
            });
            if (rc != DN_OK) return rc;
            DN_TRY(hipMemcpyAsync(guess.data(), d_guess, sizeof(int64_t) * (size_t) chunks, hipMemcpyDeviceToHost, st));
            DN_TRY(hipMemcpyAsync(res.data(), d_res, sizeof(Segment) * (size_t) chunks, hipMemcpyDeviceToHost, st));
            DN_TRY(hipStreamSynchronize(st));
            return DN_OK;
        });
    }
    int fixup(const Unit &u, Segment &res) override
    {
        DN_TRY(hipSetDevice(device));
        return dn::synced(st, [&]() -> int {
            const int rc = timed(2, [&]() -> int {
                DN_TRY(hipMemcpyAsync(d_unit, &u, sizeof(Unit), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_gz_walk, dim3(1), dim3(64), 0, st, d_comp, comp_cap, n_in, d_guess, n_chunks, shift, (const Unit *) d_unit,
                                   (int64_t) 1, d_res, d_tails);
                DN_TRY(hipGetLastError());
                return DN_OK;
            });
            if (rc != DN_OK) return rc;
            DN_TRY(hipMemcpyAsync(&res, d_res + u.slot, sizeof(Segment), hipMemcpyDeviceToHost, st));
            DN_TRY(hipStreamSynchronize(st));
            return DN_OK;
        });
    }
    int emit(const std::vector<Emit> &chain, const uint8_t *carry, int64_t total, bool check, const uint8_t **out, std::vector<EmitResult> &res) override
    {
        const int64_t n_seg = (int64_t) chain.size();
        res.assign(chain.size(), EmitResult{0, 0});
        *out = h_out;
        if (n_seg == 0) return DN_OK;
        DN_TRY(hipSetDevice(device));
        return dn::synced(st, [&]() -> int {
            int rc = fits(growth(d_out, total + 16) + growth(d_chain, n_seg) + growth(d_eres, n_seg), "a span that inflates to " + std::to_string(total) + " bytes");
            if (rc != DN_OK) return rc;
            DN_TRY(d_out.reserve(total + 16, 0, st)); DN_TRY(d_chain.reserve(n_seg, 0, st)); DN_TRY(d_eres.reserve(n_seg, 0, st));
            if (total > h_out_cap) {
                DN_TRY(h_out.alloc((size_t) dn::grown_capacity(h_out_cap, total)));
                h_out_cap = dn::grown_capacity(h_out_cap, total);
            }
            *out = h_out;
            rc = timed(0, [&]() -> int {
                DN_TRY(hipMemcpyAsync(d_chain, chain.data(), sizeof(Emit) * (size_t) n_seg, hipMemcpyHostToDevice, st));
                DN_TRY(hipMemcpyAsync(d_wins, carry, (size_t) kHist, hipMemcpyHostToDevice, st));
                return DN_OK;
            });
            if (rc != DN_OK) return rc;
            rc = timed(3, [&]() -> int {
                hipLaunchKernelGGL(k_gz_windows, dim3(1), dim3(1024), 0, st, d_tails, d_chain, n_seg, d_wins);
                DN_TRY(hipGetLastError());
                return DN_OK;
            });
            if (rc != DN_OK) return rc;
            rc = timed(4, [&]() -> int {
                hipLaunchKernelGGL(k_gz_emit, dim3((unsigned) n_seg), dim3(64), 0, st, d_comp, comp_cap, n_in, d_chain, n_seg, d_wins, d_out, check ? 1 : 0,
                                   d_eres);
                DN_TRY(hipGetLastError());
                return DN_OK;
            });
            if (rc != DN_OK) return rc;
            return timed(5, [&]() -> int {
                if (total > 0) DN_TRY(hipMemcpyAsync(h_out, d_out, (size_t) total, hipMemcpyDeviceToHost, st));
                DN_TRY(hipMemcpyAsync(res.data(), d_eres, sizeof(EmitResult) * (size_t) n_seg, hipMemcpyDeviceToHost, st));
                return DN_OK;
            });
        });
    }
};

// --- the stitch ------------------------------------------------------------------------------------------------------------

const char *status_text(int status)
{
    switch (status) {
    case DN_INFLATE_E_HEADER: return "invalid block header";
    case DN_INFLATE_E_LENGTHS: return "invalid code lengths";
    case DN_INFLATE_E_CODE: return "invalid code";
    case DN_INFLATE_E_DISTANCE: return "distance beyond the start of the member";
    case DN_INFLATE_E_INPUT: return "truncated deflate stream";
    default: return "inflated length disagrees with the walk";
    }
}

uint32_t crc_shift64(uint32_t c, int64_t n)
{
    for (; n > 0x40000000; n -= 0x40000000) c = crc_shift(c, 0x40000000u);
    return crc_shift(c, (uint32_t) n);
}

struct MemberEnd {                           // the member that ends behind chain segment `seg`
    size_t seg;
    int64_t start, trailer, out_len;
};

}  // namespace

struct dn_gz_ {
    const uint8_t *comp = nullptr;
    int64_t n = 0, chunk = 0, window = 0, grown = 0;
    int32_t shift = 0;
    bool verify = true, emit_on = true, done = false, failed = false, in_member = false;
    int64_t pos = 0;                         // outside a member: where padding or the next header starts
    int64_t entry = 0;                       // inside: the next true entry, an absolute bit
    int64_t member_start = 0, member_out = 0;
    uint32_t crc_reg = 0xffffffffu;
    std::vector<uint8_t> hist = std::vector<uint8_t>((size_t) kHist, 0);     // the member's last bytes, right-aligned
    int64_t c[DN_GZ_N_COUNTERS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int64_t> guess_abs, segments;
    std::unique_ptr<Backend> be;

    std::string at(int64_t offset, const std::string &what) const { return "gzip member at byte " + std::to_string(offset) + ": " + what; }

    // Padding and the header at pos.  true: inside a member (entry set) or done; false: err is set.
    bool header(std::string &err)
    {
        int64_t p = pos;
        if (c[0] > 0) {
            while (p < n && comp[p] == 0) p++;
            if (p < n && !(comp[p] == 0x1f && p + 1 < n && comp[p + 1] == 0x8b)) { err = at(p, "trailing garbage"); return false; }
        }
        if (p >= n) { done = true; return true; }
        const int64_t start = p;
        const auto cut = [&]() { err = at(start, "truncated header"); return false; };
        if (n - p < 10) {
            if (!(comp[p] == 0x1f && (p + 1 >= n || comp[p + 1] == 0x8b))) { err = at(start, "bad magic"); return false; }
            return cut();
        }
        if (comp[p] != 0x1f || comp[p + 1] != 0x8b) { err = at(start, "bad magic"); return false; }
        if (comp[p + 2] != 8) { err = at(start, "compression method " + std::to_string((int) comp[p + 2])); return false; }
        const int flg = comp[p + 3];
        if (flg & 0xe0) { err = at(start, "reserved flag bits set"); return false; }
        p += 10;
        if (flg & 4) {
            if (n - p < 2) return cut();
            const int64_t xlen = comp[p] | (comp[p + 1] << 8);
            if (n - p - 2 < xlen) return cut();
            p += 2 + xlen;
        }
        for (int bit : {8, 16})
            if (flg & bit) {
                while (p < n && comp[p] != 0) p++;
                if (p >= n) return cut();
                p++;
            }
        if (flg & 2) {
            if (n - p < 2) return cut();
            if (verify) {
                const uint32_t crc = crc_host(0xffffffffu, comp + start, p - start, 1, 1 << 20) ^ 0xffffffffu;
                if ((crc & 0xffffu) != (uint32_t) (comp[p] | (comp[p + 1] << 8))) { err = at(start, "header CRC mismatch"); return false; }
            }
            p += 2;
        }
        c[0]++;
        in_member = true;
        member_start = start; member_out = 0;    // crc_reg restarts at the member's first segment, when its bytes are checked
        entry = p * 8;
        return true;
    }

    int next(const uint8_t **out, int64_t *n_out, int32_t *done_out)
    {
        *out = nullptr; *n_out = 0; *done_out = 0;
        if (failed) return dn::fail(DN_E_STATE, "dn_gz_next: the stream has failed");
        std::vector<int64_t> guess;
        std::vector<Segment> res;
        std::vector<Emit> chain;
        std::vector<EmitResult> eres;
        std::vector<MemberEnd> ends;
        std::string err;
        for (;;) {
            if (!in_member && !done && !header(err)) { failed = true; return bad(err); }
            if (done) { *done_out = 1; return DN_OK; }
            // An entry at the end of the file (a header, or a block that is not final, ends the bytes): there is no span to form
            // and no block to read.  Without this the span would have no chunk and the loop no progress.
            if (entry >= n * 8) { failed = true; return bad(at(member_start, status_text(DN_INFLATE_E_INPUT))); }
            // the span: from the entry's chunk
            const int64_t c0 = entry >> shift, base = c0 * chunk;
            const int64_t want = grown ? grown : window;
            const int64_t end = n - base < want ? n : base + want, n_span = end - base, n_chunks = (n_span + chunk - 1) / chunk;
            if (n_span > (1 << 30)) { failed = true; return bad(at(member_start, "a deflate block or a run of unguessed chunks beyond 1 GiB of compressed bytes")); }
            const int64_t n_fix = n_chunks > 64 ? n_chunks : 64;
            int rc = be->scan(comp + base, n_span, n_chunks, shift, n_chunks + n_fix, guess, res);
            if (rc != DN_OK) { failed = true; return rc; }
            for (int64_t k = 0; k < n_chunks; k++) guess_abs[(size_t) (c0 + k)] = guess[(size_t) k] < 0 ? -1 : guess[(size_t) k] + base * 8;
            chain.clear(); ends.clear();
            int64_t total = 0, fix_used = 0;
            bool cut = false;
            for (;;) {
                if (!in_member && (!header(err) || done)) break;
                if (entry >= n * 8) { err = at(member_start, status_text(DN_INFLATE_E_INPUT)); break; }
                const int64_t rel = entry - base * 8, k = rel >> shift;
                if (k >= n_chunks) break;
                Segment s;
                const bool confirmed = guess[(size_t) k] == rel;
                int64_t slot = k;
                if (confirmed) s = res[(size_t) k];
                else {
                    if (fix_used == n_fix) break;
                    slot = n_chunks + fix_used++;
                    rc = be->fixup(Unit{rel, slot}, s);
                    if (rc != DN_OK) { failed = true; return rc; }
                }
                if (s.status == DN_INFLATE_E_INPUT && end < n) { cut = true; break; }
                c[confirmed ? 3 : 5]++;
                if (s.status) { err = at(member_start, status_text(s.status)); break; }
                const int64_t have = member_out < kHist ? member_out : kHist;
                chain.push_back(Emit{rel, s.exit, total, s.out_len, (int32_t) have, (int32_t) slot, member_out == 0 ? 1 : 0, s.kind});
                total += s.out_len; member_out += s.out_len;
                c[6]++; c[7] += s.blocks;
                const int64_t over = (s.exit >> shift) - k - 1;
                if (over > 0) c[4] += over;
                entry = s.exit + base * 8;
                segments.insert(segments.end(), {rel + base * 8, entry, s.out_len, (int64_t) s.kind});
                if (s.kind == DN_GZ_EXIT_MEMBER) {
                    const int64_t trailer = (entry + 7) >> 3;
                    ends.push_back(MemberEnd{chain.size() - 1, member_start, trailer, member_out});
                    in_member = false;
                    pos = trailer + 8;
                    if (pos > n) break;                      // reported below, in its turn
                }
            }
            // emit what the span confirmed, then the checks in stream order
            const uint8_t *bytes = nullptr;
            if (emit_on) {
                rc = be->emit(chain, hist.data(), total, verify, &bytes, eres);
                if (rc != DN_OK) { failed = true; return rc; }
            }
            size_t e = 0;
            for (size_t s = 0; s < chain.size(); s++) {
                const int64_t member_of = e < ends.size() ? ends[e].start : member_start;
                if (emit_on) {
                    if (eres[s].status) { failed = true; return bad(at(member_of, status_text(eres[s].status))); }
                    crc_reg = crc_shift64(chain[s].reset ? 0xffffffffu : crc_reg, chain[s].out_len) ^ eres[s].crc;
                }
                if (e < ends.size() && ends[e].seg == s) {
                    const MemberEnd &m = ends[e++];
                    if (m.trailer + 8 > n) { failed = true; return bad(at(m.start, "truncated trailer")); }
                    const uint8_t *t = comp + m.trailer;
                    const uint32_t crc = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t) t[3] << 24);
                    const uint32_t isize = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t) t[7] << 24);
                    if (emit_on && verify && (crc_reg ^ 0xffffffffu) != crc) { failed = true; return bad(at(m.start, "CRC32 mismatch")); }
                    if (isize != (uint32_t) (m.out_len & 0xffffffff)) { failed = true; return bad(at(m.start, "ISIZE mismatch")); }
                }
            }
            if (!err.empty()) { failed = true; return bad(err); }
            // the history the next span starts with
            if (emit_on)
                for (const Emit &E : chain) {
                    if (E.out_len >= kHist) memcpy(hist.data(), bytes + E.out_off + E.out_len - kHist, (size_t) kHist);
                    else if (E.out_len > 0) {
                        memmove(hist.data(), hist.data() + E.out_len, (size_t) (kHist - E.out_len));
                        memcpy(hist.data() + kHist - E.out_len, bytes + E.out_off, (size_t) E.out_len);
                    }
                }
            grown = chain.empty() && cut ? 2 * want : 0;
            c[9] += total;
            if (total > 0 && emit_on) { *out = bytes; *n_out = total; return DN_OK; }
        }
    }
};

extern "C" int dn_gz_open(const uint8_t *comp, int64_t n_comp, int32_t device, int64_t chunk_bytes, int64_t window_bytes, int32_t verify, int32_t emit,
                          dn_gz *out)
{
    dn::clear_error();
    if (!out) return bad("dn_gz_open: bad argument");
    *out = nullptr;
    if (n_comp < 0 || (n_comp > 0 && !comp) || device < -1) return bad("dn_gz_open: bad argument");
    if (chunk_bytes < 4096 || chunk_bytes > (16 << 20) || (chunk_bytes & (chunk_bytes - 1)))
        return bad("dn_gz_open: chunk_bytes must be a power of two, 4 KiB .. 16 MiB");
    if (window_bytes < 1) return bad("dn_gz_open: window_bytes must be positive");
    std::unique_ptr<dn_gz_> h(new dn_gz_);
    h->comp = comp; h->n = n_comp; h->chunk = chunk_bytes;
    h->window = (window_bytes + chunk_bytes - 1) / chunk_bytes * chunk_bytes;
    if (h->window > (1 << 30)) h->window = 1 << 30;
    for (h->shift = 3; (int64_t) 1 << (h->shift - 3) < chunk_bytes;) h->shift++;
    h->verify = verify != 0; h->emit_on = emit != 0;
    h->c[1] = (n_comp + chunk_bytes - 1) / chunk_bytes;
    h->c[8] = n_comp;
    h->guess_abs.assign((size_t) h->c[1], -1);
    if (device < 0) h->be.reset(new HostBackend);
    else {
        int n_dev = 0;
        DN_TRY(hipGetDeviceCount(&n_dev));
        if (device >= n_dev) return bad("dn_gz_open: device " + std::to_string(device) + " of " + std::to_string(n_dev));
        std::unique_ptr<DeviceBackend> d(new DeviceBackend(device));
        const int rc = d->init();
        if (rc != DN_OK) return rc;
        h->be = std::move(d);
    }
    *out = h.release();
    return DN_OK;
}

extern "C" int dn_gz_next(dn_gz h, const uint8_t **out, int64_t *n_out, int32_t *done)
{
    dn::clear_error();
    if (!h || !out || !n_out || !done) return bad("dn_gz_next: bad argument");
    return h->next(out, n_out, done);
}

extern "C" int dn_gz_counters(dn_gz h, int64_t *counters, double *ms)
{
    dn::clear_error();
    if (!h || !counters) return bad("dn_gz_counters: bad argument");
    h->c[2] = 0;
    for (int64_t g : h->guess_abs) h->c[2] += g >= 0;
    for (int k = 0; k < DN_GZ_N_COUNTERS; k++) counters[k] = h->c[k];
    if (ms)
        for (int k = 0; k < 6; k++) ms[k] = h->be->ms[k];
    return DN_OK;
}

extern "C" int dn_gz_tables(dn_gz h, int64_t *n_chunks, const int64_t **guess, int64_t *n_segments, const int64_t **segments)
{
    dn::clear_error();
    if (!h || !n_chunks || !guess || !n_segments || !segments) return bad("dn_gz_tables: bad argument");
    *n_chunks = (int64_t) h->guess_abs.size(); *guess = h->guess_abs.data();
    *n_segments = (int64_t) h->segments.size() / 4; *segments = h->segments.data();
    return DN_OK;
}

extern "C" void dn_gz_close(dn_gz h) { delete h; }
