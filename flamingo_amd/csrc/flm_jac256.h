// flm_jac256.h -- P-256 points over the per-lane field of flm_fe256.h (gfx950).
// Included by flm_p256.hip only; everything is in the anonymous namespace.
//
// Points: Jacobian (X, Y, Z), Z = 0 is the point at infinity; curve a = -3.
// Wire format (host <-> device): points are 64 bytes x||y, each a 32-byte
// big-endian integer (SEC1 uncompressed without the 0x04 prefix; the same
// bytes the reference hashes at :584-585).
#pragma once
#include "flm_fe256.h"

namespace flm {
namespace {

template <class E>
struct JacT {
    E X, Y, Z;
};
using Jac = JacT<Fe>;

// -------------------------------------------------------------- points (a = -3)
__device__ __forceinline__ Jac jac_inf() {
    // X, Y, Z are assigned in this order here, in jac_dbl and in the additions: where their early returns
    // meet, the compiler then merges the last stores of every path by value.  With Z before Y on one path
    // it merged them by address instead and kept two 7-word arrays in scratch (ecdsa_verify_kernel 832 ->
    // 784 bytes a lane, feldman_verify_kernel 60 -> 0).
    Jac r;
    r.X = fe_const(kOne);
    r.Y = fe_const(kOne);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.Z.v[i] = 0;
    return r;
}

// dbl-2001-b, written once over a field policy F (mul, sqr, add, sub): the per-lane kernels use it
// with FeField, the row kernel's rare acc == Q path with RowField (flm_p256.hip)
template <class F>
__device__ __forceinline__ JacT<typename F::E> jac_dbl(const JacT<typename F::E> &P, const F &f) {
    using E = typename F::E;
    const E delta = f.sqr(P.Z), gamma = f.sqr(P.Y), beta = f.mul(P.X, gamma);
    const E t = f.mul(f.sub(P.X, delta), f.add(P.X, delta));
    const E alpha = f.add(f.add(t, t), t);
    const E beta2 = f.add(beta, beta), beta4 = f.add(beta2, beta2), beta8 = f.add(beta4, beta4);
    JacT<E> R;
    R.X = f.sub(f.sqr(alpha), beta8);
    const E yz = f.add(P.Y, P.Z);
    const E z3 = f.sub(f.sub(f.sqr(yz), gamma), delta);
    const E g1 = f.sqr(gamma), g2 = f.add(g1, g1), g4 = f.add(g2, g2), g8 = f.add(g4, g4);  // 8 gamma^2
    R.Y = f.sub(f.mul(alpha, f.sub(beta4, R.X)), g8);
    R.Z = z3;  // after Y: jac_inf says why
    return R;
}
__device__ __forceinline__ Jac jac_dbl(const Jac &P) { return jac_dbl(P, FeField{}); }

// add-2007-bl with the exceptional cases (P == Q, P == -Q, infinity) handled
__device__ __forceinline__ Jac jac_add(const Jac &P, const Jac &Q) {
    if (fe_is_zero(P.Z)) return Q;
    if (fe_is_zero(Q.Z)) return P;
    Fe z1z1 = fe_sqr(P.Z);
    Fe z2z2 = fe_sqr(Q.Z);
    Fe u1 = fe_mul(P.X, z2z2);
    Fe u2 = fe_mul(Q.X, z1z1);
    Fe s1 = fe_mul(fe_mul(P.Y, Q.Z), z2z2);
    Fe s2 = fe_mul(fe_mul(Q.Y, P.Z), z1z1);
    Fe h = fe_sub(u2, u1);
    Fe r = fe_sub(s2, s1);
    if (fe_is_zero(h)) {
        if (fe_is_zero(r)) return jac_dbl(P);
        return jac_inf();
    }
    r = fe_add(r, r);
    Fe h2 = fe_add(h, h);
    Fe i = fe_sqr(h2);
    Fe j = fe_mul(h, i);
    Fe v = fe_mul(u1, i);
    Jac R;
    R.X = fe_sub(fe_sub(fe_sqr(r), j), fe_add(v, v));
    Fe s1j = fe_mul(s1, j);
    R.Y = fe_sub(fe_mul(r, fe_sub(v, R.X)), fe_add(s1j, s1j));
    Fe zz = fe_add(P.Z, Q.Z);
    R.Z = fe_mul(fe_sub(fe_sub(fe_sqr(zz), z1z1), z2z2), h);
    return R;
}

// madd-2007-bl: P + (x2, y2) for an affine second point (Z2 = 1), exceptional cases as jac_add
__device__ __forceinline__ Jac jac_add_affine(const Jac &P, const Fe &x2, const Fe &y2) {
    Jac Q;
    Q.X = x2;
    Q.Y = y2;
    Q.Z = fe_const(kOne);
    if (fe_is_zero(P.Z)) return Q;
    Fe z1z1 = fe_sqr(P.Z);
    Fe u2 = fe_mul(x2, z1z1);
    Fe s2 = fe_mul(fe_mul(y2, P.Z), z1z1);
    Fe h = fe_sub(u2, P.X);
    Fe r = fe_sub(s2, P.Y);
    if (fe_is_zero(h)) {
        if (fe_is_zero(r)) return jac_dbl(Q);
        return jac_inf();
    }
    r = fe_add(r, r);
    Fe hh = fe_sqr(h);
    Fe i = fe_add(hh, hh);
    i = fe_add(i, i);
    Fe j = fe_mul(h, i);
    Fe v = fe_mul(P.X, i);
    Jac R;
    R.X = fe_sub(fe_sub(fe_sqr(r), j), fe_add(v, v));
    Fe y1j = fe_mul(P.Y, j);
    R.Y = fe_sub(fe_mul(r, fe_sub(v, R.X)), fe_add(y1j, y1j));
    R.Z = fe_sub(fe_sub(fe_sqr(fe_add(P.Z, h)), z1z1), hh);
    return R;
}

// tab[t] = (2t+1) P, the wNAF / regular-recoding table of odd multiples
__device__ __forceinline__ void jac_odd_multiples(Jac (&tab)[8], const Jac &P) {
    tab[0] = P;
    const Jac P2 = jac_dbl(P);
#pragma unroll 1
    for (int t = 1; t < 8; ++t) tab[t] = jac_add(tab[t - 1], P2);
}

// Load an affine wire point; false if a coordinate is >= p or the point is off the curve.
__device__ __forceinline__ bool load_point(const uint8_t *p, Jac &out) {
    Fe x = load_be(p), y = load_be(p + 32);
    bool ok = fe_lt_p(x) && fe_lt_p(y);
    x = to_mont(x);
    y = to_mont(y);
    // y^2 == x^3 - 3x + b
    Fe rhs = fe_mul(fe_sqr(x), x);
    Fe x3 = fe_add(fe_add(x, x), x);
    rhs = fe_add(fe_sub(rhs, x3), fe_const(kBm));
    ok = ok && fe_eq(fe_sqr(y), rhs);
    out.X = x;
    out.Y = y;
    out.Z = fe_const(kOne);
    return ok;
}

__device__ __forceinline__ void store_jac(uint32_t *jac, size_t plane_stride, const Jac &R) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        jac[(size_t)k * plane_stride] = R.X.v[k];
        jac[(size_t)(8 + k) * plane_stride] = R.Y.v[k];
        jac[(size_t)(16 + k) * plane_stride] = R.Z.v[k];
    }
}

__device__ __forceinline__ Jac load_jac(const uint32_t *jac, size_t plane_stride) {
    Jac R;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        R.X.v[k] = jac[(size_t)k * plane_stride];
        R.Y.v[k] = jac[(size_t)(8 + k) * plane_stride];
        R.Z.v[k] = jac[(size_t)(16 + k) * plane_stride];
    }
    return R;
}

// Width-5 NAF of a 256-bit scalar (32-byte big endian) into d[0..kNafLen), least significant
// digit first: digits are 0 or odd in [-15, 15] and every non-zero digit is followed by at
// least four zeros, so a scalar multiplication costs ~256/6 additions instead of 64 (4-bit
// windows).  A ninth limb absorbs k + 15 for scalars near 2^256.
constexpr int kNafLen = 258;

__device__ __forceinline__ void wnaf5(const uint8_t *k_be, int8_t (&d)[kNafLen]) {
    uint32_t k[9];
    {
        const Fe f = load_be(k_be);
#pragma unroll
        for (int i = 0; i < 8; ++i) k[i] = f.v[i];
        k[8] = 0;
    }
#pragma unroll 1
    for (int i = 0; i < kNafLen; ++i) {
        int v = 0;
        if (k[0] & 1u) {
            v = (int)(k[0] & 31u);
            if (v >= 16) v -= 32;
            // k -= v  (v odd, |v| <= 15)
            uint64_t c;
            if (v > 0) {
                c = (uint64_t)k[0] - (uint32_t)v;
                k[0] = (uint32_t)c;
#pragma unroll
                for (int l = 1; l < 9; ++l) {
                    c = (uint64_t)k[l] - (c >> 63);
                    k[l] = (uint32_t)c;
                }
            } else {
                c = (uint64_t)k[0] + (uint32_t)(-v);
                k[0] = (uint32_t)c;
#pragma unroll
                for (int l = 1; l < 9; ++l) {
                    c = (uint64_t)k[l] + (c >> 32);
                    k[l] = (uint32_t)c;
                }
            }
        }
        d[i] = (int8_t)v;
#pragma unroll
        for (int l = 0; l < 8; ++l) k[l] = (k[l] >> 1) | (k[l + 1] << 31);
        k[8] >>= 1;
    }
}

}  // namespace
}  // namespace flm
