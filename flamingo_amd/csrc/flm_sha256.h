// flm_sha256.h -- SHA-256 for the P-256 kernels, one message per lane: the compression function, a
// byte-fed front end (hash to curve) and the fixed 64-byte x||y digest (seed recovery).
// Included by flm_p256.hip only; everything is in the anonymous namespace.
#pragma once
#include "flm_fe256.h"

namespace flm {
namespace {

__device__ constexpr uint32_t kK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ constexpr uint32_t kShaIv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                           0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

__device__ void sha256_block(uint32_t (&h)[8], const uint32_t (&m)[16]) {
    uint32_t w[64];
#pragma unroll
    for (int t = 0; t < 16; ++t) w[t] = m[t];
#pragma unroll
    for (int t = 16; t < 64; ++t) {
        uint32_t s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
        uint32_t s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
        w[t] = w[t - 16] + s0 + w[t - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int t = 0; t < 64; ++t) {
        uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
        uint32_t ch = (e & f) ^ (~e & g);
        uint32_t t1 = hh + S1 + ch + kK[t] + w[t];
        uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
        uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
        uint32_t t2 = S0 + mj;
        hh = g;
        g = f;
        f = e;
        e = d + t1;
        d = c;
        c = b;
        b = a;
        a = t1 + t2;
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
    h[5] += f;
    h[6] += g;
    h[7] += hh;
}

// SHA-256 fed byte by byte (the messages are short and their layout depends on the message length)
struct Sha256 {
    uint32_t h[8];
    uint32_t w[16];
    uint32_t n;      // bytes in w
    uint32_t total;  // bytes hashed
};

__device__ __forceinline__ void sha_init(Sha256 &s) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s.h[i] = kShaIv[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) s.w[i] = 0;
    s.n = 0;
    s.total = 0;
}

__device__ void sha_put(Sha256 &s, uint32_t b) {
    s.w[s.n >> 2] |= (b & 0xffu) << (24 - 8 * (s.n & 3));
    ++s.total;
    if (++s.n == 64) {
        sha256_block(s.h, s.w);
#pragma unroll
        for (int i = 0; i < 16; ++i) s.w[i] = 0;
        s.n = 0;
    }
}

// the digest as 8 big-endian words (word k = bytes 4k..4k+3)
__device__ void sha_final(Sha256 &s, uint32_t (&out)[8]) {
    const uint64_t bits = (uint64_t)s.total * 8;
    sha_put(s, 0x80);
#pragma unroll 1
    while (s.n != 56) sha_put(s, 0);
#pragma unroll 1
    for (int i = 7; i >= 0; --i) sha_put(s, (uint32_t)(bits >> (8 * i)));
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = s.h[i];
}

// SHA-256 of the 64-byte big-endian x||y; digest written as 32 bytes
__device__ void sha256_point(const Fe &x, const Fe &y, uint8_t *out) {
    uint32_t h[8], m[16];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        h[t] = kShaIv[t];
        m[t] = x.v[7 - t];
        m[8 + t] = y.v[7 - t];
    }
    sha256_block(h, m);
#pragma unroll
    for (int t = 0; t < 16; ++t) m[t] = 0;
    m[0] = 0x80000000u;
    m[15] = 512;
    sha256_block(h, m);
    uint4 *q = reinterpret_cast<uint4 *>(out);
    q[0] = make_uint4(bswap32(h[0]), bswap32(h[1]), bswap32(h[2]), bswap32(h[3]));
    q[1] = make_uint4(bswap32(h[4]), bswap32(h[5]), bswap32(h[6]), bswap32(h[7]));
}

}  // namespace
}  // namespace flm
