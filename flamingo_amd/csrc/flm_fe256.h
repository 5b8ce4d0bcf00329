// flm_fe256.h -- 256-bit modular arithmetic for the P-256 kernels, one element per lane (gfx950).
// Included by flm_p256.hip only; everything is in the anonymous namespace.
//
// Field: p = 2^256 - 2^224 + 2^192 + 2^96 - 1, eight 32-bit limbs little
// endian, Montgomery form with R = 2^256 (-p^-1 mod 2^32 = 1, so the CIOS
// quotient digit is the low limb itself).  The group order n has no special form: generic CIOS.
// Wire format (host <-> device): field elements and scalars are 32-byte big-endian integers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace flm {
namespace {

struct Fe {
    uint32_t v[8];
};

__device__ constexpr uint32_t kP[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 1u, 0xffffffffu};
__device__ constexpr uint32_t kOne[8] = {0x00000001u, 0x00000000u, 0x00000000u, 0xffffffffu,
                                         0xffffffffu, 0xffffffffu, 0xfffffffeu, 0x00000000u};  // R mod p
__device__ constexpr uint32_t kR2[8] = {0x00000003u, 0x00000000u, 0xffffffffu, 0xfffffffbu,
                                        0xfffffffeu, 0xffffffffu, 0xfffffffdu, 0x00000004u};  // R^2 mod p
__device__ constexpr uint32_t kBm[8] = {0x29c4bddfu, 0xd89cdf62u, 0x78843090u, 0xacf005cdu,
                                        0xf7212ed6u, 0xe5a220abu, 0x04874834u, 0xdc30061du};  // b*R mod p

__device__ __forceinline__ Fe fe_const(const uint32_t (&c)[8]) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = c[i];
    return r;
}

__device__ __forceinline__ bool fe_is_zero(const Fe &a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.v[i];
    return o == 0;
}

__device__ __forceinline__ bool fe_eq(const Fe &a, const Fe &b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.v[i] ^ b.v[i];
    return o == 0;
}

// ---- helpers over the modulus MOD (p or the group order n), written once
// a < MOD for a canonical (non-Montgomery) input
template <const uint32_t (&MOD)[8]>
__device__ __forceinline__ bool mod_lt(const Fe &a) {
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) (void)__builtin_subc(a.v[i], MOD[i], b, &b);
    return b != 0;
}

// Carry chains go through __builtin_addc / __builtin_subc, which lower to v_add_co / v_addc_co
// (v_sub_co / v_subb_co) with the carry in VCC: 8 instructions per 256-bit add.  The earlier
// 64-bit C form compiled to 64-bit shift-adds plus register moves: fe_add 95 VALU -> 28, fe_sub
// 75 -> 24 (gfx950 ISA count); a lone wave of the EC chain issues one VALU per ~8 cycles, so the
// instruction count is its latency.
// r = (t8:t) - MOD if that does not borrow (or t8 set), else t; requires t < 2 MOD
template <const uint32_t (&MOD)[8]>
__device__ __forceinline__ void mod_reduce_once(Fe &r, const uint32_t (&t)[8], uint32_t t8) {
    uint32_t d[8], b = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = __builtin_subc(t[i], MOD[i], b, &b);
    const bool take = t8 || !b;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = take ? d[i] : t[i];
}

template <const uint32_t (&MOD)[8]>
__device__ __forceinline__ Fe mod_add(const Fe &a, const Fe &b) {
    uint32_t s[8], c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = __builtin_addc(a.v[i], b.v[i], c, &c);
    Fe r;
    mod_reduce_once<MOD>(r, s, c);
    return r;
}

__device__ __forceinline__ bool fe_lt_p(const Fe &a) { return mod_lt<kP>(a); }
__device__ __forceinline__ Fe fe_add(const Fe &a, const Fe &b) { return mod_add<kP>(a, b); }

__device__ __forceinline__ Fe fe_sub(const Fe &a, const Fe &b) {
    uint32_t d[8], br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = __builtin_subc(a.v[i], b.v[i], br, &br);
    // borrow -> add p back (mask instead of branch)
    const uint32_t m = 0u - br;
    Fe r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = __builtin_addc(d[i], kP[i] & m, c, &c);
    return r;
}

// Montgomery reduction of a 512-bit product t by p = 2^256 - 2^224 + 2^192 + 2^96 - 1 in one
// signed column pass: the quotient digit m_i is the running limb i itself (-p^-1 = 1 mod
// 2^32) and adding m_i*p touches limbs i (-m, clears it), i+3 (+m), i+6 (+m), i+7 (-m), i+8 (+m).
__device__ __forceinline__ Fe mont_reduce(uint32_t (&t)[16]) {
    uint32_t m[8];
    int64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        int64_t s = (int64_t)t[i] + carry;
        if (i >= 3 && i - 3 < 8) s += m[i - 3];
        if (i >= 6 && i - 6 < 8) s += m[i - 6];
        if (i >= 7 && i - 7 < 8) s -= m[i - 7];
        if (i >= 8 && i - 8 < 8) s += m[i - 8];
        if (i < 8) m[i] = (uint32_t)s; else t[i - 8] = (uint32_t)s;
        carry = s >> 32;
    }
    uint32_t r8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r8[i] = t[i];
    Fe r;
    mod_reduce_once<kP>(r, r8, (uint32_t)carry);
    return r;
}

// A whole product column in ONE asm statement: NP mad/addc pairs, acc (64-bit) += a[q]*b[q]
// with every carry-out of the 64-bit accumulator counted in hi (v_mad_u64_u32's own carry-out
// feeds one v_addc).  The compiler pads each inline-asm boundary with s_nop (it cannot see
// through asm): one statement per product pair measured 543 ns per single-wave multiply,
// against 669 ns with mad and addc in separate statements and 860 ns for a plain 64-bit C CIOS
// (tools/probes/ec_probe.hip); one statement per column drops most of the remaining pads.
#define FLM_MC(n) "v_mad_u64_u32 %[acc], %[c], %[a" #n "], %[b" #n "], %[acc]\n\t" \
                  "v_addc_co_u32_e64 %[hi], %[c], 0, %[hi], %[c]\n\t"
// first product of a column whose carry counter starts at zero: hi = carry, written fresh (no
// zeroing move before the statement)
#define FLM_MC_H "v_mad_u64_u32 %[acc], %[c], %[a0], %[b0], %[acc]\n\t" \
                 "v_addc_co_u32_e64 %[hi], %[c], 0, 0, %[c]\n\t"
// first product of a column whose accumulator starts at zero: acc = a*b (cannot carry), hi = 0
#define FLM_MC_Z "v_mad_u64_u32 %[acc], %[c], %[a0], %[b0], 0\n\t" \
                 "v_mov_b32 %[hi], 0\n\t"
#define FLM_R1
#define FLM_R2 FLM_R1 FLM_MC(1)
#define FLM_R3 FLM_R2 FLM_MC(2)
#define FLM_R4 FLM_R3 FLM_MC(3)
#define FLM_R5 FLM_R4 FLM_MC(4)
#define FLM_R6 FLM_R5 FLM_MC(5)
#define FLM_R7 FLM_R6 FLM_MC(6)
#define FLM_R8 FLM_R7 FLM_MC(7)
#define FLM_MI(n) [a##n] "v"(a[n]), [b##n] "v"(b[n])
#define FLM_I1 FLM_MI(0)
#define FLM_I2 FLM_I1, FLM_MI(1)
#define FLM_I3 FLM_I2, FLM_MI(2)
#define FLM_I4 FLM_I3, FLM_MI(3)
#define FLM_I5 FLM_I4, FLM_MI(4)
#define FLM_I6 FLM_I5, FLM_MI(5)
#define FLM_I7 FLM_I6, FLM_MI(6)
#define FLM_I8 FLM_I7, FLM_MI(7)
// acc/hi are early-clobber: later products read inputs after the first mad/addc wrote them,
// so no input may share their registers (the compiler otherwise reuses one holding the same
// value, e.g. a zero limb of the constant 1 against hi's initial 0)
#define FLM_MOUT0 [acc] "+&v"(acc), [hi] "+&v"(hi), [c] "=&s"(c)
#define FLM_MOUT1 [acc] "+&v"(acc), [hi] "=&v"(hi), [c] "=&s"(c)
#define FLM_MOUT2 [acc] "=&v"(acc), [hi] "=&v"(hi), [c] "=&s"(c)
#define FLM_MCASE(N)                                                                \
    if constexpr (NP == N) {                                                        \
        if constexpr (MODE == 0) asm(FLM_MC(0) FLM_R##N : FLM_MOUT0 : FLM_I##N);    \
        else if constexpr (MODE == 1) asm(FLM_MC_H FLM_R##N : FLM_MOUT1 : FLM_I##N); \
        else asm(FLM_MC_Z FLM_R##N : FLM_MOUT2 : FLM_I##N);                          \
    }
// MODE 0: acc and hi carry in; 1: acc carries in, hi starts at zero; 2: both start at zero
// (modes 1/2 write the fresh words in the statement instead of zeroing registers before it:
// the per-column moves were ~45 of fe_mul's VALU instructions)
template <int NP, int MODE = 0>
__device__ __forceinline__ void mad_col(uint64_t &acc, uint32_t &hi, const uint32_t (&a)[NP], const uint32_t (&b)[NP]) {
    uint64_t c;
    FLM_MCASE(1) FLM_MCASE(2) FLM_MCASE(3) FLM_MCASE(4) FLM_MCASE(5) FLM_MCASE(6) FLM_MCASE(7) FLM_MCASE(8)
}
#undef FLM_MCASE
#undef FLM_MC
#undef FLM_MC_H
#undef FLM_MC_Z
#undef FLM_MI
#undef FLM_MOUT0
#undef FLM_MOUT1
#undef FLM_MOUT2

// column K of a*b (products a_i b_{K-i}) into acc/hi
template <int K>
__device__ __forceinline__ void mul_col(uint64_t &acc, uint32_t &hi, const Fe &a, const Fe &b) {
    constexpr int lo = K < 8 ? 0 : K - 7, top = K < 8 ? K : 7, n = top - lo + 1;
    uint32_t av[n], bv[n];
#pragma unroll
    for (int q = 0; q < n; ++q) {
        av[q] = a.v[lo + q];
        bv[q] = b.v[K - lo - q];
    }
    mad_col<n, K == 0 ? 2 : 1>(acc, hi, av, bv);  // hi (and at K = 0 acc) start at zero
}

// column K of the doubled cross products of a^2 (a_i a_j, i < j, i + j = K)
template <int K>
__device__ __forceinline__ void sqr_col(uint64_t &x, uint32_t &xh, const Fe &a) {
    constexpr int lo = K < 8 ? 0 : K - 7, top = K >= 1 ? (K - 1) / 2 : -1, n = top - lo + 1;
    if constexpr (n > 0) {
        uint32_t av[n], bv[n];
#pragma unroll
        for (int q = 0; q < n; ++q) {
            av[q] = a.v[lo + q];
            bv[q] = a.v[K - lo - q];
        }
        mad_col<n, 2>(x, xh, av, bv);  // x and xh start at zero
    } else {
        x = 0;
        xh = 0;
    }
}

template <int K>
__device__ __forceinline__ void mul_cols(uint64_t &acc, uint32_t &hi, uint32_t (&t)[16], const Fe &a, const Fe &b) {
    if constexpr (K < 15) {
        mul_col<K>(acc, hi, a, b);
        t[K] = (uint32_t)acc;
        acc = (acc >> 32) | ((uint64_t)hi << 32);
        mul_cols<K + 1>(acc, hi, t, a, b);
    }
}

// Montgomery product a*b*R^-1 mod p: product scanning with a 96-bit column accumulator
__device__ __forceinline__ Fe fe_mul(const Fe &a, const Fe &b) {
    uint32_t t[16];
    uint64_t acc;  // written by column 0
    uint32_t hi;
    mul_cols<0>(acc, hi, t, a, b);
    t[15] = (uint32_t)acc;
    return mont_reduce(t);
}

template <int K>
__device__ __forceinline__ void sqr_cols(uint64_t &c, uint32_t (&t)[16], const Fe &a) {
    if constexpr (K < 15) {
        uint64_t x;
        uint32_t xh;
        sqr_col<K>(x, xh, a);
        xh = (xh << 1) | (uint32_t)(x >> 63);
        x <<= 1;
        uint64_t n = x + c;
        xh += (n < x);
        x = n;
        if constexpr ((K & 1) == 0) {
            const uint32_t av[1] = {a.v[K / 2]};
            mad_col<1>(x, xh, av, av);
        }
        t[K] = (uint32_t)x;
        c = (x >> 32) | ((uint64_t)xh << 32);
        sqr_cols<K + 1>(c, t, a);
    }
}

// a^2 R^-1: 28 cross products summed once and doubled, plus 8 squares (36 mads instead of 64)
__device__ __forceinline__ Fe fe_sqr(const Fe &a) {
    uint32_t t[16];
    uint64_t c = 0;
    sqr_cols<0>(c, t, a);
    t[15] = (uint32_t)c;
    return mont_reduce(t);
}

__device__ __forceinline__ Fe fe_neg(const Fe &a) {
    Fe z = {};
    return fe_sub(z, a);
}

__device__ __forceinline__ Fe to_mont(const Fe &a) { return fe_mul(a, fe_const(kR2)); }
__device__ __forceinline__ Fe from_mont(const Fe &a) {
    Fe one = {};
    one.v[0] = 1;
    return fe_mul(a, one);
}

// The per-lane field as a policy object, for formulas written once over a field (jac_dbl in
// flm_jac256.h; LaneField in flm_p256.hip adds the cooperative kernels' LDS exchange to it).
struct FeField {
    using E = Fe;
    __device__ __forceinline__ E mul(const E &a, const E &b) const { return fe_mul(a, b); }
    __device__ __forceinline__ E sqr(const E &a) const { return fe_sqr(a); }
    __device__ __forceinline__ E add(const E &a, const E &b) const { return fe_add(a, b); }
    __device__ __forceinline__ E sub(const E &a, const E &b) const { return fe_sub(a, b); }
    __device__ __forceinline__ E neg(const E &a) const { return fe_neg(a); }
    __device__ __forceinline__ bool is_zero(const E &a) const { return fe_is_zero(a); }
};

// ec_finish inverts by binary GCD (fe_inv_bingcd below), not Fermat's a^(p-2) (round 3)

// ---- inversion by binary GCD (ec_finish_kernel's one-lane chain)
// Pornin, "Optimized Binary GCD for Modular Inversion" (eprint 2020/972), Algorithm 2, with
// k - 1 = 30 inner steps per outer step so the update factors fit int32: 18 outer steps, i.e.
// 540 >= 2 * 256 - 1 inner steps, the algorithm's bound (tools/bingcd_model.py runs exactly this
// schedule in Python and traces it).  Random inputs reach a = 0 after 12 to 14 outer steps; all 18
// are needed by 2^255 and a handful of c << k, k in 243..255 (mod p: 13 << 252, 71 << 249,
// 923 << 246, ...; mod n: 21 << 251, 31 << 251, 57 << 250, ...).  The result v is final once
// b == 1, at least one inner step earlier: every known input has it after 17 outer steps, so the
// 18th is margin (the known inputs tell 16 steps from 18, none tells 17).  The two negation
// branches below fire when the approximations order a and b wrongly (tied 34-bit top windows): the
// family m - c 2^j + off reaches them on purpose, mod n at outer step 1, mod p also at steps 3 to 9;
// mod p about 1 random input in 20,000 takes one as well.  A structured search (c << k,
// m - (c << k), m - c 2^j + off and their inverses, ~24k inputs per modulus) found no input that
// needs a 19th step: a search, not a proof.  tests/inv_cases.py lists these inputs;
// tests/test_inv_edges_gpu.py runs them through this code.
// An outer step runs 30 binary-GCD steps on 64-bit approximations of a and b (the low 30 bits
// exact, above them the top 34 bits of the longer one's window), then applies the 2 x 2 update
// matrix to the 256-bit a, b and to the Bezout coefficients u, v mod p (with a Montgomery
// division by 2^30; -p^-1 = 1 mod 2^30, so the quotient digit is the low 30 bits).  No
// data-dependent branches, so a wave's lanes never diverge.  ~25k VALU instructions against
// Fermat's ~73k (266 squarings, 11 multiplications).
__device__ constexpr uint32_t kR3[8] = {0x0000000au, 0xfffffffdu, 0xfffffff7u, 0xffffffedu,
                                        0xfffffffcu, 0x00000005u, 0x00000001u, 0x00000018u};  // R^3 mod p

// r (9 limbs, two's complement) = a * f for a unsigned 256-bit and f signed 32-bit
__device__ __forceinline__ void bg_mul_s32(uint32_t (&r)[9], const uint32_t (&a)[8], int32_t f) {
    const uint32_t F = (uint32_t)f;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c = (uint64_t)a[i] * F + (c >> 32);
        r[i] = (uint32_t)c;
    }
    r[8] = (uint32_t)(c >> 32);
    // f < 0: F = f + 2^32, so a * f = a * F - a * 2^32
    const uint32_t m = f < 0 ? 0xffffffffu : 0u;
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i + 1] = __builtin_subc(r[i + 1], a[i] & m, br, &br);
}

// r = (a * f + b * g) >> 30 (arithmetic; exact for the matrix's products), 9 limbs
__device__ __forceinline__ void bg_lin(uint32_t (&r)[9], const uint32_t (&a)[8], int32_t f, const uint32_t (&b)[8],
                                       int32_t g) {
    uint32_t x[9], y[9], c = 0;
    bg_mul_s32(x, a, f);
    bg_mul_s32(y, b, g);
#pragma unroll
    for (int i = 0; i < 9; ++i) x[i] = __builtin_addc(x[i], y[i], c, &c);
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = __builtin_amdgcn_alignbit(x[i + 1], x[i], 30);
    r[8] = (uint32_t)((int32_t)x[8] >> 30);
}

// (u * f + v * g) / 2^30 mod m, into [0, m), for the modulus m = MOD (p, or the group order n): the
// sum plus q m with q its low 30 bits times NINV30 = -m^-1 mod 2^30 (1 for p) is divisible by 2^30;
// |u f + v g| <= m 2^30 (|f| + |g| <= 2^30), so the quotient lies in [-m, 2m]
template <const uint32_t (&MOD)[8], uint32_t NINV30>
__device__ __forceinline__ void bg_lin_modp(uint32_t (&r)[8], const uint32_t (&u)[8], int32_t f,
                                            const uint32_t (&v)[8], int32_t g) {
    uint32_t x[9], y[9], c = 0;
    bg_mul_s32(x, u, f);
    bg_mul_s32(y, v, g);
#pragma unroll
    for (int i = 0; i < 9; ++i) x[i] = __builtin_addc(x[i], y[i], c, &c);
    const uint32_t q = (x[0] * NINV30) & 0x3fffffffu;
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        m = (uint64_t)MOD[i] * q + (m >> 32);
        y[i] = (uint32_t)m;
    }
    y[8] = (uint32_t)(m >> 32);
    c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) x[i] = __builtin_addc(x[i], y[i], c, &c);
    uint32_t w[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbit(x[i + 1], x[i], 30);
    w[8] = (uint32_t)((int32_t)x[8] >> 30);
    // [-p, 0) -> + p
    const uint32_t neg = (int32_t)w[8] < 0 ? 0xffffffffu : 0u;
    c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = __builtin_addc(w[i], MOD[i] & neg, c, &c);
    w[8] = __builtin_addc(w[8], 0u, c, &c);  // the sign word wraps to 0 when p was added
    // [p, 2p] -> - p
    uint32_t d[8], br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = __builtin_subc(w[i], MOD[i], br, &br);
    const bool take = w[8] != 0 || !br;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = take ? d[i] : w[i];
}

// x^-1 mod m for 0 < x < m (plain integers: the caller's Montgomery form is just an integer here).
// MOD is the odd 256-bit modulus and NINV30 = -m^-1 mod 2^30 (1 for p); the 18 x 30 steps cover any
// modulus below 2^256 (tools/bingcd_model.py runs the schedule for both p and the group order n).
template <const uint32_t (&MOD)[8], uint32_t NINV30>
__device__ Fe inv_bingcd(const Fe &x) {
    uint32_t a[8], b[8], u[8], v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = x.v[i];
        b[i] = MOD[i];
        u[i] = i == 0 ? 1u : 0u;
        v[i] = 0u;
    }
#pragma unroll 1
    for (int it = 0; it < 18; ++it) {
        // n = max(bitlen(a), bitlen(b), 64): the approximations take bits [n - 64, n) and the low 30
        uint32_t top = a[0] | b[0];
        int t = 0;
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            const uint32_t ck = a[k] | b[k];
            if (ck) {
                t = k;
                top = ck;
            }
        }
        const int bl = 32 * t + 32 - (int)__clz(top);  // b >= 1 throughout
        const int sh = (bl > 64 ? bl : 64) - 64;
        const int q = sh >> 5, r = sh & 31;            // q <= 6
        uint32_t a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
#pragma unroll
        for (int k = 1; k <= 6; ++k) {
            if (q == k) {
                a0 = a[k]; a1 = a[k + 1]; a2 = k + 2 < 8 ? a[(k + 2) & 7] : 0u;
                b0 = b[k]; b1 = b[k + 1]; b2 = k + 2 < 8 ? b[(k + 2) & 7] : 0u;
            }
        }
        uint64_t ab = ((uint64_t)__builtin_amdgcn_alignbit(a2, a1, r) << 32) |
                      ((__builtin_amdgcn_alignbit(a1, a0, r) & 0xc0000000u) | (a[0] & 0x3fffffffu));
        uint64_t bb = ((uint64_t)__builtin_amdgcn_alignbit(b2, b1, r) << 32) |
                      ((__builtin_amdgcn_alignbit(b1, b0, r) & 0xc0000000u) | (b[0] & 0x3fffffffu));
        int32_t f0 = 1, g0 = 0, f1 = 0, g1 = 1;
#pragma unroll
        for (int j = 0; j < 30; ++j) {
            const bool odd = (uint32_t)ab & 1u;
            const bool sw = odd && ab < bb;
            const uint64_t xa = sw ? bb : ab, xb = sw ? ab : bb;
            const int32_t xf0 = sw ? f1 : f0, xg0 = sw ? g1 : g0, xf1 = sw ? f0 : f1, xg1 = sw ? g0 : g1;
            ab = (xa - (odd ? xb : 0ull)) >> 1;
            bb = xb;
            f0 = xf0 - (odd ? xf1 : 0);
            g0 = xg0 - (odd ? xg1 : 0);
            f1 = xf1 * 2;
            g1 = xg1 * 2;
        }
        uint32_t na[9], nb[9];
        bg_lin(na, a, f0, b, g0);
        bg_lin(nb, a, f1, b, g1);
        // a negative result: negate it and its row of the matrix
        const bool nga = (int32_t)na[8] < 0, ngb = (int32_t)nb[8] < 0;
        {
            const uint32_t ma = nga ? 0xffffffffu : 0u, mb = ngb ? 0xffffffffu : 0u;
            uint32_t ca = nga ? 1u : 0u, cb = ngb ? 1u : 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                a[i] = __builtin_addc(na[i] ^ ma, 0u, ca, &ca);
                b[i] = __builtin_addc(nb[i] ^ mb, 0u, cb, &cb);
            }
        }
        if (nga) { f0 = -f0; g0 = -g0; }
        if (ngb) { f1 = -f1; g1 = -g1; }
        uint32_t nu[8], nv[8];
        bg_lin_modp<MOD, NINV30>(nu, u, f0, v, g0);
        bg_lin_modp<MOD, NINV30>(nv, u, f1, v, g1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            u[i] = nu[i];
            v[i] = nv[i];
        }
    }
    Fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = v[i];  // b = 1 = v x (mod m)
    return r;
}

__device__ Fe fe_inv_bingcd(const Fe &x) { return inv_bingcd<kP, 1u>(x); }

// ------------------------------------------------- scalar field (mod n)
// n is the P-256 group order (the reference's `prime`, ecchash.n).  Generic
// CIOS Montgomery (n has no special form).
__device__ constexpr uint32_t kN[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu,
                                       0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu};
__device__ constexpr uint32_t kR2N[8] = {0xbe79eea2u, 0x83244c95u, 0x49bd6fa6u, 0x4699799cu,
                                         0x2b6bec59u, 0x2845b239u, 0xf3d95620u, 0x66e12d94u};  // R^2 mod n
constexpr uint32_t kN0 = 0xee00bc4fu;                                                             // -n^-1 mod 2^32
constexpr uint32_t kNInv30 = kN0 & 0x3fffffffu;  // -n^-1 mod 2^30

__device__ __forceinline__ Fe sc_mul(const Fe &a, const Fe &b) {
    uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t t8 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            c = (uint64_t)a.v[j] * b.v[i] + t[j] + (c >> 32);
            t[j] = (uint32_t)c;
        }
        uint64_t s = (uint64_t)t8 + (c >> 32);
        uint32_t hi0 = (uint32_t)s, hi1 = (uint32_t)(s >> 32);
        uint32_t m = t[0] * kN0;
        c = (uint64_t)m * kN[0] + t[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            c = (uint64_t)m * kN[j] + t[j] + (c >> 32);
            t[j - 1] = (uint32_t)c;
        }
        s = (uint64_t)hi0 + (c >> 32);
        t[7] = (uint32_t)s;
        t8 = hi1 + (uint32_t)(s >> 32);
    }
    Fe r;
    mod_reduce_once<kN>(r, t, t8);
    return r;
}

__device__ __forceinline__ bool sc_lt_n(const Fe &a) { return mod_lt<kN>(a); }
__device__ __forceinline__ Fe sc_add(const Fe &a, const Fe &b) { return mod_add<kN>(a, b); }
// any a < 2^256 < 2n brought below n: one subtraction
__device__ __forceinline__ Fe sc_below_n(const Fe &a) {
    Fe r;
    mod_reduce_once<kN>(r, a.v, 0u);
    return r;
}

// ---- wire format
__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// 32-byte big endian -> limbs
__device__ __forceinline__ Fe load_be(const uint8_t *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    uint4 a = q[0], b = q[1];
    uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    Fe r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r.v[k] = bswap32(w[7 - k]);
    return r;
}

__device__ __forceinline__ void store_be(uint8_t *p, const Fe &a) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(bswap32(a.v[7]), bswap32(a.v[6]), bswap32(a.v[5]), bswap32(a.v[4]));
    q[1] = make_uint4(bswap32(a.v[3]), bswap32(a.v[2]), bswap32(a.v[1]), bswap32(a.v[0]));
}

}  // namespace
}  // namespace flm
