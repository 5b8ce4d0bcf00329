// flm_aes128.h -- AES-128 and GCM's field multiplication as block functions, one message per lane
// (gfx950); aes_gcm_xor_kernel and aes_gcm_auth_kernel in flm_p256.hip stage the S-box in LDS and
// drive them.
// Included by flm_p256.hip only; everything is in the anonymous namespace.
// State columns are big-endian words (row 0 in the top byte).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace flm {
namespace {

__device__ constexpr uint8_t kAesSbox[256] = {
    0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b, 0xfe, 0xd7, 0xab, 0x76,
    0xca, 0x82, 0xc9, 0x7d, 0xfa, 0x59, 0x47, 0xf0, 0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0,
    0xb7, 0xfd, 0x93, 0x26, 0x36, 0x3f, 0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15,
    0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07, 0x12, 0x80, 0xe2, 0xeb, 0x27, 0xb2, 0x75,
    0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0, 0x52, 0x3b, 0xd6, 0xb3, 0x29, 0xe3, 0x2f, 0x84,
    0x53, 0xd1, 0x00, 0xed, 0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58, 0xcf,
    0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f, 0x50, 0x3c, 0x9f, 0xa8,
    0x51, 0xa3, 0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5, 0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2,
    0xcd, 0x0c, 0x13, 0xec, 0x5f, 0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73,
    0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88, 0x46, 0xee, 0xb8, 0x14, 0xde, 0x5e, 0x0b, 0xdb,
    0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c, 0xc2, 0xd3, 0xac, 0x62, 0x91, 0x95, 0xe4, 0x79,
    0xe7, 0xc8, 0x37, 0x6d, 0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a, 0xae, 0x08,
    0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f, 0x4b, 0xbd, 0x8b, 0x8a,
    0x70, 0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e, 0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e,
    0xe1, 0xf8, 0x98, 0x11, 0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf,
    0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42, 0x68, 0x41, 0x99, 0x2d, 0x0f, 0xb0, 0x54, 0xbb, 0x16,
};

__device__ __forceinline__ uint32_t rotl32(uint32_t w, int s) { return (w << s) | (w >> (32 - s)); }

__device__ __forceinline__ uint32_t aes_sub_word(const uint8_t *sb, uint32_t w) {
    return ((uint32_t)sb[w >> 24] << 24) | ((uint32_t)sb[(w >> 16) & 255u] << 16) | ((uint32_t)sb[(w >> 8) & 255u] << 8) |
           (uint32_t)sb[w & 255u];
}

// SubBytes + ShiftRows of column c: row r comes from column c + r
__device__ __forceinline__ uint32_t aes_sub_shift(const uint8_t *sb, const uint32_t (&s)[4], int c) {
    return ((uint32_t)sb[s[c] >> 24] << 24) | ((uint32_t)sb[(s[(c + 1) & 3] >> 16) & 255u] << 16) |
           ((uint32_t)sb[(s[(c + 2) & 3] >> 8) & 255u] << 8) | (uint32_t)sb[s[(c + 3) & 3] & 255u];
}

// MixColumns of one column: 2 b_r ^ 3 b_{r+1} ^ b_{r+2} ^ b_{r+3} in row r, four bytes at once
__device__ __forceinline__ uint32_t aes_mix(uint32_t w) {
    const uint32_t x2 = ((w & 0x7f7f7f7fu) << 1) ^ (((w >> 7) & 0x01010101u) * 0x1bu);
    return x2 ^ rotl32(x2 ^ w, 8) ^ rotl32(w, 16) ^ rotl32(w, 24);
}

__device__ __forceinline__ void aes128_encrypt(const uint8_t *sb, const uint32_t (&rk)[44], uint32_t (&s)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] ^= rk[c];
#pragma unroll
    for (int r = 1; r < 10; ++r) {
        uint32_t t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) t[c] = aes_mix(aes_sub_shift(sb, s, c)) ^ rk[4 * r + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = t[c];
    }
    uint32_t t[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] = aes_sub_shift(sb, s, c) ^ rk[40 + c];
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] = t[c];
}

// x = x * h in GF(2^128) as GCM orders its bits (bit 0 = top bit of byte 0; R = 0xe1 || 0^120):
// shift-and-xor over the 128 bits of x, words big endian, no data-dependent branch
__device__ __forceinline__ void gcm_mul(uint32_t (&x)[4], const uint32_t (&h)[4]) {
    uint32_t z[4] = {0, 0, 0, 0}, v[4] = {h[0], h[1], h[2], h[3]};
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        const uint32_t xw = x[w];
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            const uint32_t take = 0u - ((xw >> b) & 1u), lsb = 0u - (v[3] & 1u);
            z[0] ^= v[0] & take;
            z[1] ^= v[1] & take;
            z[2] ^= v[2] & take;
            z[3] ^= v[3] & take;
            v[3] = (v[3] >> 1) | (v[2] << 31);
            v[2] = (v[2] >> 1) | (v[1] << 31);
            v[1] = (v[1] >> 1) | (v[0] << 31);
            v[0] = (v[0] >> 1) ^ (0xe1000000u & lsb);
        }
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) x[w] = z[w];
}

// byte loads, not bswap32 of a word load: keys and nonces come from the caller's device pointers
// (flm_aes_gcm_xor_dev), and a 12-byte nonce row promises no word alignment
__device__ __forceinline__ uint32_t load_be32(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// the 44 round-key words of the 16-byte key at `key` (aes_gcm_xor_kernel keeps its own, older copy of
// these lines, so that its machine code stays what §6 of DESIGN.md measured)
__device__ __forceinline__ void aes128_expand_key(const uint8_t *sb, const uint8_t *key, uint32_t (&rk)[44]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) rk[w] = load_be32(key + 4 * w);
#pragma unroll
    for (int w = 4; w < 44; ++w) {
        uint32_t t = rk[w - 1];
        if (w % 4 == 0) {
            constexpr uint32_t rcon[10] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1b, 0x36};
            t = aes_sub_word(sb, rotl32(t, 8)) ^ (rcon[w / 4 - 1] << 24);
        }
        rk[w] = rk[w - 4] ^ t;
    }
}

// the first cnt (1..16) bytes at p as a block of big-endian words, zero behind them (GHASH's padding)
__device__ __forceinline__ void load_block_be(const uint8_t *p, uint32_t cnt, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k)
        if (k < cnt) w[k >> 2] |= (uint32_t)p[k] << (24u - 8u * (k & 3u));
}

// the first cnt (1..16) bytes of a block of big-endian words to p
__device__ __forceinline__ void store_block_be(uint8_t *p, uint32_t cnt, const uint32_t (&w)[4]) {
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k)
        if (k < cnt) p[k] = (uint8_t)(w[k >> 2] >> (24u - 8u * (k & 3u)));
}

// word w of a block whose first cnt bytes are ones and the rest zero
__device__ __forceinline__ uint32_t head_mask(uint32_t cnt, uint32_t w) {
    const uint32_t nb = cnt > 4u * w ? (cnt - 4u * w < 4u ? cnt - 4u * w : 4u) : 0u;
    return nb ? 0xffffffffu << (32u - 8u * nb) : 0u;
}

// y = GHASH_h continued over len bytes at p, the last block zero padded (SP 800-38D, 6.4)
__device__ __forceinline__ void ghash_absorb(uint32_t (&y)[4], const uint32_t (&h)[4], const uint8_t *p, uint32_t len) {
#pragma unroll 1
    for (uint32_t o = 0; o < len; o += 16u) {
        uint32_t b[4];
        load_block_be(p + o, len - o < 16u ? len - o : 16u, b);
#pragma unroll
        for (int w = 0; w < 4; ++w) y[w] ^= b[w];
        gcm_mul(y, h);
    }
}

}  // namespace
}  // namespace flm
