// dn_crc.hpp -- the CRC-32 of BGZF blocks, sliced so that the lanes of a wavefront share one block: what the decoder
// (dn_inflate.hip) checks and the encoder (dn_deflate.hip) writes.  __host__ __device__ code; every unit that includes this
// header gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef DN_HD
#define DN_HD __host__ __device__ __forceinline__
#endif

namespace {

// --- CRC-32 (RFC 1952), reflected: bit 31 of a register is the coefficient of x^0 ------------------------------------------

constexpr uint32_t kCrcPoly = 0xEDB88320u;

// the register after `nbits` more bits whose data was xor-ed into its low end
DN_HD uint32_t crc_bits(uint32_t c, int nbits)
{
    for (int k = 0; k < nbits; k++) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
    return c;
}

// a * b mod P
constexpr __host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int k = 0; k < 32; k++) {
        r ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));               // b * x
    }
    return r;
}

struct CrcPowers { uint32_t v[32]; };                               // v[k] = x^(8 * 2^k) mod P
constexpr __host__ __device__ inline CrcPowers crc_powers()
{
    CrcPowers t{};
    uint32_t p = 0x00800000u;                                       // x^8
    for (int k = 0; k < 32; k++) { t.v[k] = p; p = crc_mul(p, p); }
    return t;
}

// c * x^(8 n) mod P: what n zero bytes make of a register that started from c (without the xor-in of an initial value)
DN_HD uint32_t crc_shift(uint32_t c, uint32_t n)
{
    constexpr CrcPowers t = crc_powers();
    for (int k = 0; n != 0; k++, n >>= 1)
        if (n & 1u) c = crc_mul(c, t.v[k]);
    return c;
}

// The part of lane `lane` of `lanes` in the CRC of bytes [a, b) (0 <= a <= b): the span is cut at dword boundaries into
// `lanes` slices of an odd number of dwords each (lanes that read LDS a power-of-two stride apart would share a bank; an
// odd stride spreads 64 lanes over all 64), the lane runs its slice from register 0 and shifts the result by the bytes
// behind the slice.  The xor of all lanes' parts is raw([a, b), 0).  rd.dword(p): the four bytes at p, a multiple of 4;
// bytes outside [a, b) may hold anything.
template <class R> DN_HD uint32_t crc_slice(const R &rd, int32_t a, int32_t b, int lane, int lanes)
{
    const int32_t a4 = a & ~3;
    const int32_t per = ((((b - a4 + 3) >> 2) + lanes - 1) / lanes) | 1;
    int32_t lo = a4 + 4 * per * lane, hi = lo + 4 * per;
    if (lo < a) lo = a;
    if (hi > b) hi = b;
    if (lo >= hi) return 0;
    uint32_t c = 0;
    for (int32_t p = lo & ~3; p < hi; p += 4) {
        const int32_t s = p < lo ? lo : p, e = p + 4 < hi ? p + 4 : hi;
        uint32_t w = rd.dword(p) >> (8 * (s - p));
        if (e - s == 4) c = crc_bits(c ^ w, 32);
        else c = crc_bits(c ^ (w & ((1u << (8 * (e - s))) - 1u)), 8 * (e - s));
    }
    return crc_shift(c, (uint32_t) (b - hi));
}

// the register reg after the bytes [a, b) too, from the xor of every lane's crc_slice
DN_HD uint32_t crc_join(uint32_t reg, uint32_t slices, int32_t a, int32_t b) { return crc_shift(reg, (uint32_t) (b - a)) ^ slices; }

struct ArrayReader {                                                // plain memory of n bytes
    const uint8_t *base;
    int64_t n;
    uint32_t dword(int64_t p) const
    {
        uint32_t w = 0;
        for (int k = 0; k < 4; k++)
            if (p + k >= 0 && p + k < n) w |= (uint32_t) base[p + k] << (8 * k);
        return w;
    }
};

// the register reg after data[0 .. n), cut into spans of `flush` bytes and every span into `lanes` slices
uint32_t crc_host(uint32_t reg, const uint8_t *data, int64_t n, int lanes, int32_t flush)
{
    for (int64_t o = 0; o < n; o += flush) {
        const int32_t len = (int32_t) (n - o < flush ? n - o : flush);
        const ArrayReader rd{data + o, len};
        uint32_t x = 0;
        for (int l = 0; l < lanes; l++) x ^= crc_slice(rd, 0, len, l, lanes);
        reg = crc_join(reg, x, 0, len);
    }
    return reg;
}

}  // namespace
