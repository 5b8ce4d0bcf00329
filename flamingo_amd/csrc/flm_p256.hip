// flm_p256.hip -- P-256 batch kernels for Flamingo's seed recovery (gfx950).
//
// The server recovers every dropped pair's seed from the committee's threshold
// ElGamal decryption shares (SA_ServiceAgent.py:542-585):
//     point_i = c1_i - sum_j lambda_j * share_{j,i}          (share = sk_j * c0_i)
//     seed_i  = SHA-256(x(point_i) || y(point_i))            (32-byte big endian)
// and the clients/committee do single scalar multiplications (ECDH :256-263,
// ElGamal :434-447, decryption shares :397-400).  All of it is 256-bit modular
// arithmetic on independent points -- one lane per (term, pair) scalar
// multiplication (or four cooperating waves per 64 of them, exchanging field
// elements through LDS), a few lanes per pair for the combine -- so this is
// VALU integer work: no MFMA.  A small batch is one latency chain, bound by the
// quarter-rate v_mad_u64_u32 on its critical path.
//
// This file holds the kernels, the cooperative formulas with their field policies, the ECDSA recoding
// with the fixed-base ladder it shares with the Feldman share check, the hash-to-curve map and the
// launchers.  The device libraries under them are headers that only this translation unit includes:
// flm_fe256.h (the fields mod p and mod n, inversion, wire format), flm_jac256.h (points, wNAF, odd
// multiples), flm_sha256.h, flm_aes128.h and flm_fe_row.h (16-lane rows).

#include <hip/hip_runtime.h>

#include "flm_aes128.h"
#include "flm_fe_row.h"
#include "flm_internal.h"
#include "flm_jac256.h"
#include "flm_sha256.h"

namespace flm {
namespace {

// ------------------------------------------------------------------ kernels
constexpr int kEcThreads = 64;

// Scalar multiplication scalar * point for T x D (term, element) pairs, flattened to one lane
// per pair g = j*D + i (1-D grid; the workgroup size is a launch parameter).
// points: [T][D][64] wire bytes; scalars: [T][32] (one per term) or [T][D][32] when
// per_element; jac out: SoA planes [T][24][D].
// wNAF (w = 5) with a table of the odd multiples P, 3P, ..., 15P: ~256 doublings and ~43
// additions from the most significant digit (was: fixed 4-bit windows, 252 + 63 + 13 table).
// The combine's scalars are one per term, so a wave's digits (and branches) are uniform.
template <int TPB, int WPE>
__global__ __launch_bounds__(TPB, WPE) void ec_mul_kernel(const uint8_t *__restrict__ points,
                                                     const uint8_t *__restrict__ scalars, int per_element, int T,
                                                     int D, uint32_t *__restrict__ jac,
                                                     uint32_t *__restrict__ flags) {
    // Latency-bound (one wave's issue chain sets the time): when the unmask runs beside it on
    // another stream (flamingo_amd/reconstruct.py), let these waves issue first; the
    // throughput-bound unmask waves fill the remaining slots.
    __builtin_amdgcn_s_setprio(3);
    const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (g >= (size_t)T * D) return;
    const int j = (int)(g / D);
    const int i = (int)(g - (size_t)j * D);
    const size_t e = g;
    Jac P;
    bool ok = load_point(points + e * 64, P);
    if (!ok) atomicOr(&flags[i], 2u);
    int8_t dig[kNafLen];
    wnaf5(scalars + (per_element ? e : (size_t)j) * 32, dig);

    // jac_odd_multiples written out: through the helper the <*, 4> instantiations spill 16 bytes more
    // per lane (profiles/p256_layers_resources.txt)
    Jac tab[8];  // tab[t] = (2t+1) P
    tab[0] = P;
    const Jac P2 = jac_dbl(P);
#pragma unroll 1
    for (int t = 1; t < 8; ++t) tab[t] = jac_add(tab[t - 1], P2);

    Jac acc = jac_inf();
    bool started = false;
#pragma unroll 1
    for (int w = kNafLen - 1; w >= 0; --w) {
        if (started) acc = jac_dbl(acc);
        const int v = dig[w];
        if (v) {
            Jac Q = tab[(v < 0 ? -v : v) >> 1];
            if (v < 0) Q.Y = fe_neg(Q.Y);
            acc = started ? jac_add(acc, Q) : Q;
            started = true;
        }
    }
    if (!ok) acc = jac_inf();
    store_jac(jac + (size_t)j * 24 * D + i, (size_t)D, acc);
}

// ------------------------------------------------ Straus: NT terms per lane
// The combine's sum_j lambda_j share_{j,i} with NT consecutive terms per lane sharing ONE chain
// of doublings (Straus / Shamir's trick): ~256 doublings + NT x ~43 additions + NT tables per lane
// instead of NT x (256 + 43 + 8) -- 35 % less work at NT = 2, for a longer chain per lane.  Worth it
// where the combine is throughput-bound (ServerReconstruction's 32 EC CUs).  Output: the per-lane
// partial sums as SoA planes [ceil(T/NT)][24][D] for ec_finish_kernel.  Off-curve points count as
// infinity and set flag bit 1, as in ec_mul_kernel.
template <int NT>
__global__ __launch_bounds__(kEcThreads) void ec_mul_straus_kernel(const uint8_t *__restrict__ points,
                                                                  const uint8_t *__restrict__ scalars, int T, int D,
                                                                  uint32_t *__restrict__ jac,
                                                                  uint32_t *__restrict__ flags) {
    __builtin_amdgcn_s_setprio(3);
    const int Tg = (T + NT - 1) / NT;
    const size_t g = (size_t)blockIdx.x * kEcThreads + threadIdx.x;
    if (g >= (size_t)Tg * D) return;
    const int jg = (int)(g / D);
    const int i = (int)(g - (size_t)jg * D);
    int8_t dig[NT][kNafLen];
    Jac tab[NT][8];
#pragma unroll 1
    for (int u = 0; u < NT; ++u) {
        const int j = jg * NT + u;
        Jac P = jac_inf();
        if (j < T) {
            if (!load_point(points + ((size_t)j * D + i) * 64, P)) {
                atomicOr(&flags[i], 2u);
                P = jac_inf();
            }
            wnaf5(scalars + (size_t)j * 32, dig[u]);
        } else {
#pragma unroll 1
            for (int k = 0; k < kNafLen; ++k) dig[u][k] = 0;
        }
        jac_odd_multiples(tab[u], P);
    }
    Jac acc = jac_inf();
#pragma unroll 1
    for (int w = kNafLen - 1; w >= 0; --w) {
        acc = jac_dbl(acc);  // doubling infinity keeps Z = 0
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int v = dig[u][w];
            if (v) {
                Jac Q = tab[u][(v < 0 ? -v : v) >> 1];
                if (v < 0) Q.Y = fe_neg(Q.Y);
                acc = jac_add(acc, Q);
            }
        }
    }
    store_jac(jac + (size_t)jg * 24 * D + i, (size_t)D, acc);
}

// ------------------------------------------------ cooperative scalar multiplication
// The same product as ec_mul_kernel, with FOUR waves (on the CU's four SIMDs) per 64 scalar
// multiplications: lane l of every wave works on item g = blockIdx.x * 64 + l, and the field
// multiplications of each point doubling are spread over the waves, exchanging field elements
// through LDS between three barriers:
//   L1  w0: delta = Z^2          w1: gamma = Y^2          w2: s = (Y+Z)^2
//   L2  w0: t = (X-delta)(X+delta), 3t   w1: beta = X gamma, 4 beta, 8 beta   w2: 8 gamma^2
//       w3: Z3 = s - gamma - delta
//   L3  w0: X3 = (3t)^2 - 8 beta, Y3 = 3t (4 beta - X3) - 8 gamma^2
// so a doubling costs 4 multiplications of latency instead of 8 (dbl-2001-b, a = -3).  Additions
// (~43 per scalar) run on wave 0 with the table of odd multiples in LDS.  A scalar multiplication is
// one lane's latency chain (~2,850 field multiplications), so where the batch leaves most SIMDs
// idle -- seed recovery on the whole chip, one rank's share of the pairs on G GPUs, the agents'
// ECDH/ElGamal batches -- this halves it; where the batch already fills its CUs (the CU-split
// reconstruction) the per-lane kernel issues fewer instructions.  Exceptional cases as jac_add.
constexpr int kCoopWaves = 4;
constexpr int kCoopSlots = 11;
// The cooperative kernels carry W = Z^4 (modified Jacobian, coop_dbl_w / coop_add_w below).

// lane-major slots: a lane's 8 words are 32 contiguous bytes, moved with two 16-byte LDS ops
// (0.5-1 % faster than word-major single-dword ops, profiles/r02_ab_coop_b128.log)
__device__ __forceinline__ void xput(uint32_t *slot, const Fe &a, int lane) {
    uint4 *q = reinterpret_cast<uint4 *>(slot + lane * 8);
    q[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
    q[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
__device__ __forceinline__ Fe xget(const uint32_t *slot, int lane) {
    const uint4 *q = reinterpret_cast<const uint4 *>(slot + lane * 8);
    const uint4 x = q[0], y = q[1];
    Fe a;
    a.v[0] = x.x; a.v[1] = x.y; a.v[2] = x.z; a.v[3] = x.w;
    a.v[4] = y.x; a.v[5] = y.y; a.v[6] = y.z; a.v[7] = y.w;
    return a;
}

// ---- modified Jacobian (X, Y, Z, W = Z^4) for the cooperative kernels 
// Carrying W takes the doubling's a Z^4 term off the critical path: alpha = 3 (X^2 - W) needs one
// squaring, so alpha^2 lands one level earlier and a doubling is 3 multiplications of latency and
// two barriers instead of 4 and three.  Same outputs as dbl-2001-b (X3, Y3, Z3 are identical), so
// the Jacobian result and everything after it are bit-identical.
//
// The formulas are written once over a field policy F: LaneField (one element per lane, the
// Montgomery limbs of flm_fe256.h, exchange slots of 512 words) for ec_mul_coop_kernel, and
// RowField (one element per 16-lane row, flm_fe_row.h, slots of 64 words) for ec_mul_row_kernel.
template <class E>
struct JacWT {
    E X, Y, Z, W;
};
using JacW = JacWT<Fe>;

struct LaneField : FeField {
    static constexpr int kSlot = 512;       // words per exchange slot: 64 lanes x 8 limbs
    static constexpr int kCoord = 8 * 64;   // words per coordinate of a table entry
    static constexpr int kEntry = 24 * 64;  // words per table entry (X, Y, Z)
    __device__ __forceinline__ void put(uint32_t *slot, const E &a, int lane) const { xput(slot, a, lane); }
    __device__ __forceinline__ E get(const uint32_t *slot, int lane) const { return xget(slot, lane); }
    __device__ __forceinline__ JacT<E> inf() const { return jac_inf(); }
    __device__ __forceinline__ JacT<E> dbl(const JacT<E> &P) const { return jac_dbl(P); }
};

struct RowField {
    using E = uint32_t;
    static constexpr int kSlot = 64;  // one word per lane: 4 elements x 16 lanes
    static constexpr int kCoord = 64;
    static constexpr int kEntry = 3 * 64;
    row::Ctx K;
    __device__ __forceinline__ E mul(E a, E b) const { return row::mul(a, b, K); }
    __device__ __forceinline__ E sqr(E a) const { return row::sqr(a, K); }
    __device__ __forceinline__ E add(E a, E b) const { return row::add(a, b, K); }
    __device__ __forceinline__ E sub(E a, E b) const { return row::sub(a, b, K); }
    __device__ __forceinline__ E neg(E a) const { return row::neg(a, K); }
    __device__ __forceinline__ bool is_zero(E a) const { return row::is_zero(a, K); }
    __device__ __forceinline__ void put(uint32_t *slot, E a, int lane) const { slot[lane] = a; }
    __device__ __forceinline__ E get(const uint32_t *slot, int lane) const { return slot[lane]; }
    __device__ __forceinline__ E one() const { return (threadIdx.x & 15) == 0 ? 1u : 0u; }
    __device__ __forceinline__ JacT<E> inf() const {  // (1, 1, 0), normal form
        JacT<E> r;
        r.X = r.Y = one();
        r.Z = 0u;
        return r;
    }
    // the rare acc == Q path of an addition: out of line (the kernel is sized by its hot loop)
    __device__ JacT<E> dbl(const JacT<E> &P) const { return jac_dbl(P, *this); }
};

// entry e of the LDS table of odd multiples: X, Y, Z, each coordinate laid out as an exchange slot
template <class F, class J>
__device__ __forceinline__ void tab_put(uint32_t *tab, int e, const J &P, int lane, const F &f) {
    uint32_t *q = tab + (size_t)e * F::kEntry;
    f.put(q, P.X, lane);
    f.put(q + F::kCoord, P.Y, lane);
    f.put(q + 2 * F::kCoord, P.Z, lane);
}
template <class F>
__device__ __forceinline__ JacT<typename F::E> tab_get(const uint32_t *tab, int e, int lane, const F &f) {
    const uint32_t *q = tab + (size_t)e * F::kEntry;
    return {f.get(q, lane), f.get(q + F::kCoord, lane), f.get(q + 2 * F::kCoord, lane)};
}

//   before barrier 1  w0: XX = X^2, alpha = 3 (XX - W), alpha^2
//                     w1: beta = X Y^2 -> 4 beta (slot 0), 8 beta (slot 1)
//                     w2: gamma^2 -> 8 gamma^2 (slot 2)            w3: Z3 = 2 Y Z
//   between barriers  w0: X3 = alpha^2 - 8 beta, Y3 = alpha (4 beta - X3) - 8 gamma^2 (slots 6, 7)
//                     w2: W3 = 16 gamma^2 W (slot 9)                w3: Z3 (slot 8)
// Slots 0..2 are read by w0 before barrier 2; the results (6..9) are written only between the two
// barriers, so the next operation's writes before its first barrier (slots 0..2 for a doubling,
// A/B = 0/1 for an addition) never land on a slot another wave is still reading.
template <class F>
__device__ __forceinline__ void coop_dbl_w(JacWT<typename F::E> &acc, int w, int lane, uint32_t *S, const F &f) {
    using E = typename F::E;
    constexpr int Q = F::kSlot;
    E alpha, a2, g8, z3;
    if (w == 0) {
        const E t = f.sub(f.sqr(acc.X), acc.W);
        alpha = f.add(f.add(t, t), t);
        a2 = f.sqr(alpha);
    } else if (w == 1) {
        const E beta = f.mul(acc.X, f.sqr(acc.Y));
        const E b2 = f.add(beta, beta);
        const E b4 = f.add(b2, b2);
        f.put(S + 0 * Q, b4, lane);
        f.put(S + 1 * Q, f.add(b4, b4), lane);
    } else if (w == 2) {
        E g = f.sqr(f.sqr(acc.Y));
        g = f.add(g, g);
        g = f.add(g, g);
        g8 = f.add(g, g);
        f.put(S + 2 * Q, g8, lane);
    } else {
        const E yz = f.mul(acc.Y, acc.Z);
        z3 = f.add(yz, yz);
    }
    __syncthreads();
    if (w == 0) {
        const E x3 = f.sub(a2, f.get(S + 1 * Q, lane));
        f.put(S + 6 * Q, x3, lane);
        f.put(S + 7 * Q, f.sub(f.mul(alpha, f.sub(f.get(S + 0 * Q, lane), x3)), f.get(S + 2 * Q, lane)), lane);
    } else if (w == 2) {
        f.put(S + 9 * Q, f.mul(f.add(g8, g8), acc.W), lane);
    } else if (w == 3) {
        f.put(S + 8 * Q, z3, lane);
    }
    __syncthreads();
    acc.X = f.get(S + 6 * Q, lane);
    acc.Y = f.get(S + 7 * Q, lane);
    acc.Z = f.get(S + 8 * Q, lane);
    acc.W = f.get(S + 9 * Q, lane);
}

// coop_add with W carried: the same six levels; w3, idle after L3, squares its Z3 twice (L4, L5)
// into slot H, and L6 picks W for the exceptional cases (Q or a doubling: two squarings of the new
// Z on that rare path; infinity: 0; acc: its own W).  Result slots D, E, F and K (W).
template <class F>
__device__ __forceinline__ void coop_add_w(JacWT<typename F::E> &acc, bool sel, int tab_idx, bool neg, int w, int lane,
                                           uint32_t *S, const uint32_t *tab, const F &f) {
    using E = typename F::E;
    constexpr int Q_ = F::kSlot;
    JacT<E> Q = tab_get(tab, tab_idx, lane, f);
    if (neg) Q.Y = f.neg(Q.Y);
    uint32_t *A = S, *B = S + Q_, *C = S + 2 * Q_, *Dd = S + 3 * Q_, *Ee = S + 4 * Q_, *Fs = S + 5 * Q_,
             *G = S + 6 * Q_, *H = S + 7 * Q_, *I = S + 8 * Q_, *J = S + 9 * Q_, *K = S + 10 * Q_;
    E z1z1, z2z2, zz, s2a, s1a, u1, u2, s2, s1, h, i, j, v, x3, y3a, z3;
    // L1
    if (w == 0) {
        z1z1 = f.sqr(acc.Z);
        f.put(A, z1z1, lane);
    } else if (w == 1) {
        z2z2 = f.sqr(Q.Z);
        f.put(B, z2z2, lane);
    } else if (w == 2) {
        zz = f.sqr(f.add(acc.Z, Q.Z));
    } else {
        s1a = f.mul(acc.Y, Q.Z);
    }
    __syncthreads();
    // L2
    if (w == 0) {
        f.put(Dd, f.mul(Q.X, z1z1), lane);  // u2
    } else if (w == 1) {
        u1 = f.mul(acc.X, z2z2);
        f.put(Ee, u1, lane);
    } else if (w == 2) {
        z1z1 = f.get(A, lane);
        z2z2 = f.get(B, lane);
        f.put(Fs, f.sub(f.sub(zz, z1z1), z2z2), lane);  // Z3'
        s2a = f.mul(Q.Y, acc.Z);
    } else {
        z2z2 = f.get(B, lane);
        f.put(G, f.mul(s1a, z2z2), lane);  // s1
    }
    __syncthreads();
    // L3
    if (w == 0) {
        u2 = f.get(Dd, lane);
        u1 = f.get(Ee, lane);
        h = f.sub(u2, u1);
        const E h2 = f.add(h, h);
        i = f.sqr(h2);
        f.put(H, i, lane);
    } else if (w == 2) {
        s2 = f.mul(s2a, z1z1);
    } else if (w == 3) {
        u2 = f.get(Dd, lane);
        u1 = f.get(Ee, lane);
        z3 = f.mul(f.get(Fs, lane), f.sub(u2, u1));  // Z3 = Z3' h
        f.put(I, z3, lane);
    }
    __syncthreads();
    // L4
    if (w == 0) {
        j = f.mul(h, i);
        f.put(J, j, lane);
    } else if (w == 1) {
        i = f.get(H, lane);
        v = f.mul(u1, i);
        f.put(K, v, lane);
        f.put(Dd, f.add(v, v), lane);
    } else if (w == 2) {
        s1 = f.get(G, lane);
        E r = f.sub(s2, s1);
        r = f.add(r, r);
        f.put(A, r, lane);
        f.put(B, f.sqr(r), lane);
    } else {
        z3 = f.sqr(z3);
    }
    __syncthreads();
    // L5
    E r;
    if (w == 0) {
        v = f.get(K, lane);
        r = f.get(A, lane);
        const E rr = f.get(B, lane);
        x3 = f.sub(f.sub(rr, j), f.get(Dd, lane));
        y3a = f.mul(r, f.sub(v, x3));
    } else if (w == 1) {
        s1 = f.get(G, lane);
        j = f.get(J, lane);
        const E s1j = f.mul(s1, j);
        f.put(C, f.add(s1j, s1j), lane);
    } else if (w == 3) {
        f.put(H, f.sqr(z3), lane);  // W3 = Z3^4 (H's i was read at L4)
    }
    __syncthreads();
    // L6
    if (w == 0) {
        JacWT<E> R;
        R.X = x3;
        R.Y = f.sub(y3a, f.get(C, lane));
        R.Z = f.get(I, lane);
        R.W = f.get(H, lane);
        if (f.is_zero(acc.Z)) {
            R.X = Q.X; R.Y = Q.Y; R.Z = Q.Z;
            R.W = f.sqr(f.sqr(Q.Z));
        } else if (f.is_zero(Q.Z)) {
            R = acc;
        } else if (f.is_zero(h)) {
            JacT<E> a;
            a.X = acc.X; a.Y = acc.Y; a.Z = acc.Z;
            const JacT<E> d = f.is_zero(r) ? f.dbl(a) : f.inf();  // acc == Q / acc == -Q (rare: one lane)
            R.X = d.X; R.Y = d.Y; R.Z = d.Z;
            R.W = f.sqr(f.sqr(d.Z));
        }
        if (!sel) R = acc;
        f.put(Dd, R.X, lane);
        f.put(Ee, R.Y, lane);
        f.put(Fs, R.Z, lane);
        f.put(K, R.W, lane);
    }
    __syncthreads();
    acc.X = f.get(Dd, lane);
    acc.Y = f.get(Ee, lane);
    acc.Z = f.get(Fs, lane);
    acc.W = f.get(K, lane);
}

// The body ec_mul_coop_kernel and ec_mul_row_kernel share: acc = dig * PW for the block's lanes, all
// four waves in step.  S: kCoopSlots slots of F::kSlot words; tab: 9 entries of F::kEntry words.
// acc is the kernel's own object, PW and f come by value: with acc returned and PW, f by reference
// ec_mul_coop_kernel's combine took 1.51 ms against 1.48 (profiles/p256_layers_ladder_shapes.txt).
template <class F>
__device__ __forceinline__ void coop_ladder(JacWT<typename F::E> &acc, const JacWT<typename F::E> PW,
                                            const int8_t (&dig)[kNafLen], int w, int lane, uint32_t *S,
                                            uint32_t *tab, const F f) {
    using E = typename F::E;
    // table of odd multiples (2k+1) P (X, Y, Z only: an addend's W is needed on the rare path only): 2P
    // into entry 1 as the addend, then entry k = entry k-1 + 2P; 3P waits in the spare entry 8 meanwhile
    JacWT<E> P2 = PW;
    coop_dbl_w(P2, w, lane, S, f);
    if (w == 0) {
        tab_put(tab, 0, PW, lane, f);
        tab_put(tab, 1, P2, lane, f);
    }
    __syncthreads();
    JacWT<E> t = PW;
#pragma unroll 1
    for (int k = 1; k < 8; ++k) {
        coop_add_w(t, true, 1, false, w, lane, S, tab, f);
        if (w == 0) tab_put(tab, k == 1 ? 8 : k, t, lane, f);
        __syncthreads();
    }
    if (w == 0) tab_put(tab, 1, tab_get(tab, 8, lane, f), lane, f);
    __syncthreads();
    const JacT<E> inf = f.inf();
    acc.X = inf.X; acc.Y = inf.Y; acc.Z = inf.Z; acc.W = inf.Z;  // W = Z^4 = 0
    // the next digit is read from scratch before the doubling, so its latency hides under it (read
    // after the doubling, every step waited for the scratch load: tools/probes/ec_row_split.py)
    int v_next = dig[kNafLen - 1];
#pragma unroll 1
    for (int k = kNafLen - 1; k >= 0; --k) {
        const int v = v_next;
        if (k > 0) v_next = dig[k - 1];
        coop_dbl_w(acc, w, lane, S, f);
        if (__any(v != 0)) coop_add_w(acc, v != 0, (v < 0 ? -v : v) >> 1, v < 0, w, lane, S, tab, f);
    }
}

__global__ __launch_bounds__(64 * kCoopWaves) void ec_mul_coop_kernel(const uint8_t *__restrict__ points,
                                                                   const uint8_t *__restrict__ scalars,
                                                                   int per_element, int T, int D,
                                                                   uint32_t *__restrict__ jac,
                                                                   uint32_t *__restrict__ flags) {
    // latency-bound like ec_mul_kernel: beside the unmask on another stream (the unpartitioned
    // overlap, every rank of a sharded reconstruction) these waves issue first
    __builtin_amdgcn_s_setprio(3);
    __shared__ __attribute__((aligned(16))) uint32_t S[kCoopSlots * LaneField::kSlot];  // exchange slots, 512 words each
    __shared__ __attribute__((aligned(16))) uint32_t tab[9 * LaneField::kEntry];  // (2t+1) P, t = 0..7, + a spare row
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t g = (size_t)blockIdx.x * 64 + lane;
    const bool valid = g < (size_t)T * D;
    const int j = valid ? (int)(g / D) : 0;
    const int i = valid ? (int)(g - (size_t)j * D) : 0;
    // every wave loads the point and recodes the scalar itself (no exchange needed for either)
    Jac P = jac_inf();
    bool ok = true;
    int8_t dig[kNafLen];
    if (valid) {
        ok = load_point(points + g * 64, P);
        if (!ok) P = jac_inf();
        wnaf5(scalars + (per_element ? g : (size_t)j) * 32, dig);
    } else {
#pragma unroll 1
        for (int k = 0; k < kNafLen; ++k) dig[k] = 0;
    }
    if (w == 0 && valid && !ok) atomicOr(&flags[i], 2u);
    JacW PW;
    PW.X = P.X; PW.Y = P.Y; PW.Z = P.Z;
    PW.W = fe_sqr(fe_sqr(P.Z));
    JacW accw;
    coop_ladder(accw, PW, dig, w, lane, S, tab, LaneField{});
    if (w == 0 && valid) {
        Jac acc;
        acc.X = accw.X; acc.Y = accw.Y; acc.Z = accw.Z;
        if (!ok) acc = jac_inf();
        store_jac(jac + (size_t)j * 24 * D + i, (size_t)D, acc);
    }
}

// The cooperative kernel with every field element spread over a 16-lane row (flm_fe_row.h): a
// workgroup is the same four waves (formula roles w0..w3 as coop_dbl_w / coop_add_w), each wave
// holding four scalar multiplications, one per row.  A row multiplication is ~93 instructions per
// lane against ~258 for the per-lane Montgomery one, so each level of the formulas is that much
// shorter; in exchange the batch takes 16x the lanes.  For batches that leave most SIMDs idle --
// one G = 8 rank's share of the c5 pairs (ceil(962/8) x 20 products), the agents' ECDH batches --
// that is the trade to make (tools/ec_row_model.py).  Values stay in normal
// form inside; the result is converted to the Montgomery Jacobian planes ec_finish_kernel reads.
__device__ constexpr uint32_t kBn[8] = {0x27d2604bu, 0x3bce3c3eu, 0xcc53b0f6u, 0x651d06b0u,
                                        0x769886bcu, 0xb3ebbd55u, 0xaa3a93e7u, 0x5ac635d8u};  // b

__global__ __launch_bounds__(64 * kCoopWaves) void ec_mul_row_kernel(const uint8_t *__restrict__ points,
                                                                  const uint8_t *__restrict__ scalars,
                                                                  int per_element, int T, int D,
                                                                  uint32_t *__restrict__ jac,
                                                                  uint32_t *__restrict__ flags) {
    __builtin_amdgcn_s_setprio(3);
    __shared__ uint32_t S[kCoopSlots * RowField::kSlot];  // exchange slots, one word per lane
    __shared__ uint32_t tab[9 * RowField::kEntry];        // (2t+1) P, t = 0..7, + a spare entry
    const int lane = threadIdx.x & 63, r = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    RowField f;
    f.K = row::make_ctx();
    const size_t g = (size_t)blockIdx.x * 4 + (lane >> 4);
    const bool valid = g < (size_t)T * D;
    const int j = valid ? (int)(g / D) : 0;
    const int i = valid ? (int)(g - (size_t)j * D) : 0;
    // the point: lane r < 8 holds limb r of x and of y (the wire is big endian)
    uint32_t x = 0, y = 0;
    if (valid && r < 8) {
        const uint32_t *pw = reinterpret_cast<const uint32_t *>(points + g * 64);
        x = __builtin_bswap32(pw[7 - r]);
        y = __builtin_bswap32(pw[15 - r]);
    }
    // x, y < p and y^2 == x^3 - 3x + b (every lane runs every row operation: no divergence around
    // the carry loops' wave-wide votes)
    const uint32_t rhs = f.add(f.sub(f.mul(f.sqr(x), x), f.add(f.add(x, x), x)), r < 8 ? kBn[r & 7] : 0u);
    const bool in_x = row::row_all8(row::canon(x, f.K) == x, f.K);
    const bool in_y = row::row_all8(row::canon(y, f.K) == y, f.K);
    const bool on_c = row::row_all8(row::canon(f.sqr(y), f.K) == row::canon(rhs, f.K), f.K);
    const bool ok = in_x && in_y && on_c;
    if (w == 0 && valid && !ok && r == 0) atomicOr(&flags[i], 2u);
    JacWT<uint32_t> PW;
    PW.X = ok ? x : f.one();
    PW.Y = ok ? y : f.one();
    PW.Z = ok ? f.one() : 0u;
    PW.W = PW.Z;  // Z^4 of Z = 1 or 0
    int8_t dig[kNafLen];
    if (valid) {
        wnaf5(scalars + (per_element ? g : (size_t)j) * 32, dig);
    } else {
#pragma unroll 1
        for (int k = 0; k < kNafLen; ++k) dig[k] = 0;
    }
    JacWT<uint32_t> acc;
    coop_ladder(acc, PW, dig, w, lane, S, tab, f);
    if (w == 0) {
        // to the Montgomery form of ec_finish_kernel (x R mod p; R mod p = kOne as a normal value),
        // canonical; an invalid point went in as infinity (1, 1, 0) and comes out as (R, R, 0)
        const uint32_t rm = r < 8 ? kOne[r & 7] : 0u;
        const uint32_t X = row::canon(f.mul(acc.X, rm), f.K);
        const uint32_t Y = row::canon(f.mul(acc.Y, rm), f.K);
        const uint32_t Z = row::canon(f.mul(acc.Z, rm), f.K);
        if (valid && r < 8) {
            uint32_t *o = jac + (size_t)j * 24 * D + i;
            o[(size_t)r * D] = X;
            o[(size_t)(8 + r) * D] = Y;
            o[(size_t)(16 + r) * D] = Z;
        }
    }
}

// Per element i: acc = base_i (c1, or infinity when base == nullptr) + sign * sum_j R_{j,i};
// write the affine wire point and optionally SHA-256(x||y).
// flags bit 0: base off-curve, bit 1: an input share was off-curve (ec_mul), bit 2: result at infinity.
// kFinishLanes lanes per element split the T terms (lane q adds j = q, q + kFinishLanes, ...), then
// log2(kFinishLanes) LDS tree levels add the partials.  At T = 20: 8 lanes make it 3 + 3 sequential
// additions (lane 0 adds c1 first), 4 lanes 5 + 2 (round 3: 8).
// Lane 0 of each element then inverts Z and hashes (the inversion is one lane's chain either way).
constexpr int kFinishLanes = 8;
static_assert(kFinishLanes >= 1 && (kFinishLanes & (kFinishLanes - 1)) == 0 && kFinishLanes <= 64,
              "kFinishLanes: a power of two dividing the workgroup");
__global__ __launch_bounds__(kEcThreads) void ec_finish_kernel(const uint8_t *__restrict__ base,
                                                               const uint32_t *__restrict__ jac, int T, int D,
                                                               int negate, uint8_t *__restrict__ points_out,
                                                               uint8_t *__restrict__ digests_out,
                                                               uint32_t *__restrict__ flags) {
    __builtin_amdgcn_s_setprio(3);
    __shared__ uint32_t part[kEcThreads * 24];
    const int q = threadIdx.x % kFinishLanes;
    const int i = blockIdx.x * (kEcThreads / kFinishLanes) + threadIdx.x / kFinishLanes;
    const bool valid = i < D;
    uint32_t fl = 0;
    Jac acc = jac_inf();
    if (valid && q == 0 && base) {
        if (!load_point(base + (size_t)i * 64, acc)) {
            fl |= 1u;
            acc = jac_inf();
        }
    }
    if (valid) {
#pragma unroll 1
        for (int j = q; j < T; j += kFinishLanes) {
            Jac R = load_jac(jac + (size_t)j * 24 * D + i, (size_t)D);
            if (negate) R.Y = fe_neg(R.Y);
            acc = jac_add(acc, R);
        }
    }
    // tree over the element's 4 lanes (adjacent threads): level 1 lanes 0,2 add lanes 1,3;
    // level 2 lane 0 adds lane 2
    uint32_t *mine = part + threadIdx.x * 24;
#pragma unroll 1
    for (int step = 1; step < kFinishLanes; step *= 2) {
        store_jac(mine, 1, acc);
        __syncthreads();
        if (valid && (q % (2 * step)) == 0) acc = jac_add(acc, load_jac(mine + step * 24, 1));
        __syncthreads();
    }
    if (!valid || q != 0) return;
    Fe x = {}, y = {};
    if (fe_is_zero(acc.Z)) {
        fl |= 4u;
    } else {
        // acc.Z is Z R mod p as an integer: (Z R)^-1 R^3 R^-1 = Z^-1 R, the Montgomery form of Z^-1
        Fe zi = fe_mul(fe_inv_bingcd(acc.Z), fe_const(kR3));
        Fe zi2 = fe_sqr(zi);
        x = from_mont(fe_mul(acc.X, zi2));
        y = from_mont(fe_mul(acc.Y, fe_mul(zi2, zi)));
    }
    if (points_out) {
        store_be(points_out + (size_t)i * 64, x);
        store_be(points_out + (size_t)i * 64 + 32, y);
    }
    if (digests_out) sha256_point(x, y, digests_out + (size_t)i * 32);
    if (fl) atomicOr(&flags[i], fl);
}

// ------------------------------------------------- Shamir over the scalar field (mod n)
// Shamir recovery of the self-mask seeds (SA_ServiceAgent.py:506-526):
//     m_i = sum_j lambda_j * y_{j,i} mod n,   seed_i = m_i.to_bytes(32, 'big')
// with n the P-256 group order; T multiplications per lane (sc_mul, flm_fe256.h).
// shares: [T][M][32] big endian; lambdas: [T][32]; out: [M][32] big endian
__global__ __launch_bounds__(kEcThreads) void shamir_combine_kernel(const uint8_t *__restrict__ shares,
                                                                    const uint8_t *__restrict__ lambdas, int T,
                                                                    int M, uint8_t *__restrict__ out) {
    const int i = blockIdx.x * kEcThreads + threadIdx.x;
    if (i >= M) return;
    Fe acc = {};
    const Fe r2 = fe_const(kR2N);
#pragma unroll 1
    for (int j = 0; j < T; ++j) {
        const Fe y = sc_below_n(load_be(shares + ((size_t)j * M + i) * 32));
        Fe lm = sc_mul(load_be(lambdas + (size_t)j * 32), r2);   // lambda * R mod n
        acc = sc_add(acc, sc_mul(lm, y));                   // lambda * y mod n
    }
    store_be(out + (size_t)i * 32, acc);
}

// Shamir dealing of the self-mask seeds (SA_ClientAgent.py:218-220), one lane per share:
//     y[c][i] = sum_{j<T} coeffs[j][i] * xs[c]^j mod n        (Horner, top coefficient first)
// coeffs: [T][M][32] big endian, term 0 the secret, any value < 2^256 (reduced on load);
// xs: [C] non-zero; out: [C][M][32] big endian, every value < n -- row c is a `shares[j]` of
// shamir_combine_kernel.  x goes into Montgomery form once, so each sc_mul(acc, x R) leaves
// acc * x in plain form: T - 1 multiplications per lane.  A 256 x 32-bit multiply-and-reduce
// would be cheaper; unmeasured against the launch, so not done.
__global__ __launch_bounds__(kEcThreads) void shamir_deal_kernel(const uint8_t *__restrict__ coeffs, int T, int M,
                                                                 const uint32_t *__restrict__ xs, int C,
                                                                 uint8_t *__restrict__ out) {
    const size_t g = (size_t)blockIdx.x * kEcThreads + threadIdx.x;
    if (g >= (size_t)C * (size_t)M) return;
    const size_t c = g / (size_t)M, i = g % (size_t)M;
    Fe x = {};
    x.v[0] = xs[c];
    const Fe xm = sc_mul(x, fe_const(kR2N));  // x * R mod n
    Fe acc = sc_below_n(load_be(coeffs + ((size_t)(T - 1) * M + i) * 32));
#pragma unroll 1
    for (int j = T - 2; j >= 0; --j)
        acc = sc_add(sc_mul(acc, xm), sc_below_n(load_be(coeffs + ((size_t)j * M + i) * 32)));
    store_be(out + g * 32, acc);
}

// ------------------------------------------------------------- ECDSA verification
// The signatures a committee member must check before it releases decryption shares: the
// server's over the offline set and the other members' over the same labels, forwarded in DEC
// (SA_ServiceAgent.py:382-386; the reference leaves the check as the comment
// `# CHECK SIGNATURES`, SA_ClientAgent.py:387).  One lane per signature, the verdict of FIPS 186-4
// section 6.4.2 and of OpenSSL's ECDSA_do_verify:
//     r, s in [1, n-1];  Q a point of the curve, not infinity;
//     w = s^-1 mod n,  u1 = (e mod n) w,  u2 = r w,  R = u1 G + u2 Q != infinity,  x(R) mod n == r.
//
// u1 and u2 differ from row to row, so a wNAF's sparse digits would send the lanes of a wave down
// different branches and every step would run both additions anyway.  The scalars are recoded
// regularly instead: an odd k < 2^256 is 2^256 + sum_{i<64} d_i 16^i with
//     d_i = 2 ((k >> (4 i + 1)) & 15) - 15,   odd, in [-15, 15], never zero
// (every bit b_j of k written as the digit 2 b_{j+1} - 1 of weight 2^j, a top digit of +1), and an
// even k is taken as n - k with the point negated.  Every lane then runs the same schedule: one
// chain of 256 doublings shared by both scalars (Straus) and 65 x (one mixed addition from the
// constant affine table of G's odd multiples + one addition from the lane's Jacobian table of
// Q's), about 3,800 field multiplications with no divergence.  jac_add's exceptional cases stay:
// u1 G = +-u2 Q and keys that are small multiples of G reach them.
// (2t+1) G, t = 0..7, affine x then y, Montgomery form (oracle/ec_oracle.py mul(2t+1) times 2^256 mod
// p; tests/test_ecdsa_cpu.py recomputes the table)
__device__ constexpr uint32_t kGOdd[8][16] = {
    {0x18a9143cu, 0x79e730d4u, 0x5fedb601u, 0x75ba95fcu, 0x77622510u, 0x79fb732bu, 0xa53755c6u, 0x18905f76u,
     0xce95560au, 0xddf25357u, 0xba19e45cu, 0x8b4ab8e4u, 0xdd21f325u, 0xd2e88688u, 0x25885d85u, 0x8571ff18u},  // 1G
    {0x4eebc127u, 0xffac3f90u, 0x087d81fbu, 0xb027f84au, 0x87cbbc98u, 0x66ad77ddu, 0xb6ff747eu, 0x26936a3fu,
     0xc983a7ebu, 0xb04c5c1fu, 0x0861fe1au, 0x583e47adu, 0x1a2ee98eu, 0x78820831u, 0xe587cc07u, 0xd5f06a29u},  // 3G
    {0xc45c61f5u, 0xbe1b8aaeu, 0x94b9537du, 0x90ec649au, 0xd076c20cu, 0x941cb5aau, 0x890523c8u, 0xc9079605u,
     0xe7ba4f10u, 0xeb309b4au, 0xe5eb882bu, 0x73c568efu, 0x7e7a1f68u, 0x3540a987u, 0x2dd1e916u, 0x73a076bbu},  // 5G
    {0xa0173b4fu, 0x0746354eu, 0xd23c00f7u, 0x2bd20213u, 0x0c23bb08u, 0xf43eaab5u, 0xc3123e03u, 0x13ba5119u,
     0x3f5b9d4du, 0x2847d030u, 0x5da67bddu, 0x6742f2f2u, 0x77c94195u, 0xef933bdcu, 0x6e240867u, 0xeaedd915u},  // 7G
    {0x264e20e8u, 0x75c96e8fu, 0x59a7a841u, 0xabe6bfedu, 0x44c8eb00u, 0x2cc09c04u, 0xf0c4e16bu, 0xe05b3080u,
     0xa45f3314u, 0x1eb7777au, 0xce5d45e3u, 0x56af7bedu, 0x88b12f1au, 0x2b6e019au, 0xfd835f9bu, 0x086659cdu},  // 9G
    {0x6245e404u, 0xea7d260au, 0x6e7fdfe0u, 0x9de40795u, 0x8dac1ab5u, 0x1ff3a415u, 0x649c9073u, 0x3e7090f1u,
     0x2b944e88u, 0x1a768561u, 0xe57f61c8u, 0x250f939eu, 0x1ead643du, 0x0c0daa89u, 0xe125b88eu, 0x68930023u},  // 11G
    {0x4b2ed709u, 0xccc42563u, 0x856fd30du, 0x0e356769u, 0x559e9811u, 0xbcbcd43fu, 0x5395b759u, 0x738477acu,
     0xc00ee17fu, 0x35752b90u, 0x742ed2e3u, 0x68748390u, 0xbd1f5bc1u, 0x7cd06422u, 0xc9e7b797u, 0xfbc08769u},  // 13G
    {0xbc60055bu, 0x72bcd8b7u, 0x56e27e4bu, 0x03cc23eeu, 0xe4819370u, 0xee337424u, 0x0ad3da09u, 0xe2aa0e43u,
     0x6383c45du, 0x40b8524fu, 0x42a41b25u, 0xd7663554u, 0x778a4797u, 0x64efa6deu, 0x7079adf4u, 0x2042170au},  // 15G
};

// A scalar k < n under the regular recoding above: odd |k| stored as k >> 1 with the digits taken
// from the top nibble, neg = the point's sign.
struct Regular {
    uint32_t k[8];
    bool neg;
};

__device__ __forceinline__ Regular regular_recode(const Fe &k) {
    Regular r;
    r.neg = (k.v[0] & 1u) == 0;  // even (0 included): n - k is odd, and (n - k)(-P) = k P
    uint32_t d[8], b = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = __builtin_subc(kN[i], k.v[i], b, &b);
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = r.neg ? d[i] : k.v[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) r.k[i] = (d[i] >> 1) | (i < 7 ? d[i + 1] << 31 : 0u);
    return r;
}

// the next digit from the top, as (table index t, negative): digit = +-(2t + 1), sign already
// folded with the scalar's
__device__ __forceinline__ void regular_next(Regular &r, int &t, bool &negative) {
    const int d = 2 * (int)(r.k[7] >> 28) - 15;
#pragma unroll
    for (int i = 7; i > 0; --i) r.k[i] = (r.k[i] << 4) | (r.k[i - 1] >> 28);
    r.k[0] <<= 4;
    t = (d < 0 ? -d : d) >> 1;
    negative = (d < 0) != r.neg;
}

// The fixed-base half of a regular ladder, shared by ecdsa_verify_kernel (u1 G, beside u2 Q on the same
// doublings) and feldman_verify_kernel (s G alone): acc +- (2t+1) G as a mixed addition from kGOdd ...
__device__ __forceinline__ Jac fixed_base_add(const Jac &acc, int t, bool negative) {
    Fe gx, gy;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        gx.v[k] = kGOdd[t][k];
        gy.v[k] = kGOdd[t][8 + k];
    }
    if (negative) gy = fe_neg(gy);
    return jac_add_affine(acc, gx, gy);
}
// ... and one window's step after its four doublings: the scalar's next digit, added.  The top digit
// (+1, weight 2^256) is fixed_base_add(acc, 0, k.neg) before the first window.
__device__ __forceinline__ Jac fixed_base_step(const Jac &acc, Regular &k) {
    int t;
    bool negative;
    regular_next(k, t, negative);
    return fixed_base_add(acc, t, negative);
}

// pubkeys n x 64 wire bytes, digests n x 32, sigs n x 64 (r || s), all big endian.
// ok[i] = 1 accept / 0 reject; flags[i] (may be NULL): bit 0 r or s outside [1, n-1], bit 1 Q not a
// valid point, bit 2 u1 G + u2 Q at infinity.
__global__ __launch_bounds__(kEcThreads) void ecdsa_verify_kernel(const uint8_t *__restrict__ pubkeys,
                                                                  const uint8_t *__restrict__ digests,
                                                                  const uint8_t *__restrict__ sigs, int n,
                                                                  uint8_t *__restrict__ ok_out,
                                                                  uint32_t *__restrict__ flags) {
    __builtin_amdgcn_s_setprio(3);  // one wave's issue chain sets the time, as the other EC kernels
    const size_t g = (size_t)blockIdx.x * kEcThreads + threadIdx.x;
    if (g >= (size_t)n) return;
    const Fe r = load_be(sigs + g * 64), s = load_be(sigs + g * 64 + 32);
    uint32_t fl = 0;
    if (fe_is_zero(r) || fe_is_zero(s) || !sc_lt_n(r) || !sc_lt_n(s)) fl |= 1u;
    Jac Q;
    bool q_ok = load_point(pubkeys + g * 64, Q);  // (0, 0), the wire form of infinity, is off the curve
    {
        const uint4 *qw = reinterpret_cast<const uint4 *>(pubkeys + g * 64);
        uint32_t any = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) any |= qw[k].x | qw[k].y | qw[k].z | qw[k].w;
        if (any == 0) q_ok = false;  // infinity, rejected explicitly
    }
    if (!q_ok) fl |= 2u;
    bool accept = false;
    if (fl == 0) {
        const Fe e = sc_below_n(load_be(digests + g * 32));
        const Fe w = inv_bingcd<kN, kNInv30>(s);
        const Fe wm = sc_mul(w, fe_const(kR2N));  // w R mod n, so sc_mul(x, wm) = x w
        Regular k1 = regular_recode(sc_mul(e, wm));
        Regular k2 = regular_recode(sc_mul(r, wm));

        Jac tab[8];  // tab[t] = (2t+1) Q
        jac_odd_multiples(tab, Q);

        // top digits (+1 each, weight 2^256): acc = +-G +- Q
        Jac acc = Q;
        if (k2.neg) acc.Y = fe_neg(acc.Y);
        acc = fixed_base_add(acc, 0, k1.neg);
#pragma unroll 1
        for (int wnd = 0; wnd < 64; ++wnd) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) acc = jac_dbl(acc);  // doubling infinity keeps Z = 0
            acc = fixed_base_step(acc, k1);
            int t;
            bool negative;
            regular_next(k2, t, negative);
            Jac A = tab[t];
            if (negative) A.Y = fe_neg(A.Y);
            acc = jac_add(acc, A);
        }
        if (fe_is_zero(acc.Z)) {
            fl |= 4u;
        } else {
            // x(R) = X / Z^2 mod p, and x(R) mod n == r iff x(R) is r, or r + n where that is below p
            const Fe z2 = fe_sqr(acc.Z);
            accept = fe_eq(fe_mul(to_mont(r), z2), acc.X);
            uint32_t rn[8], c = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) rn[k] = __builtin_addc(r.v[k], kN[k], c, &c);
            Fe r2;
#pragma unroll
            for (int k = 0; k < 8; ++k) r2.v[k] = rn[k];
            if (!accept && c == 0 && fe_lt_p(r2)) accept = fe_eq(fe_mul(to_mont(r2), z2), acc.X);
        }
    }
    ok_out[g] = accept ? 1 : 0;
    if (flags) flags[g] = fl;
}

// ------------------------------------------------------------- Feldman share checks (the DKG)
// The check a committee member runs on every share a dealer sends it in the joint-Feldman key
// generation (agent/dkg/SA_ClientAgent.py:219-228, verify_commitment):
//     s G == F_d(x) = sum_{k<T} x^k C_{d,k}
// with C_{d,k} = c_{d,k} G the dealer's commitments to its polynomial's coefficients.  The reference
// evaluates the right-hand side as T full scalar multiplications by the unreduced integer x ** k; here
// it is Horner's rule in the exponent, one lane per (dealer, x, share) row:
//     acc = C_{d,T-1};   acc = x acc + C_{d,k}   for k = T-2 .. 0
// where x acc is left-to-right double-and-add over exactly x_bits bits (a launch parameter, so every
// lane runs the same number of steps): (T-1) (x_bits doublings + at most x_bits + 1 additions), 21 x
// (6 + 7) point operations at the protocol's T = 22, x <= 60, against 22 x ~300 for the reference's form.
// The per-bit addition is taken by branch: the lanes of a wave hold different x, so a mixed wave runs
// the addition masked at the cost computing and selecting would have every time, and a wave whose
// lanes all have the bit clear (the upper bits of small x under a wide x_bits, x = 0) skips it.
// The left-hand side is the fixed-base half of the ECDSA ladder (fixed_base_step) and runs after the
// right-hand side, whose temporaries are dead by then: the lane carries F (24 words) through it.
// Commitments: [T][M][64] wire bytes, term-major; 64 zero bytes are the point at infinity, a valid
// term (a zero coefficient).  A commitment with a coordinate >= p or off the curve sets flag bit 1,
// counts as infinity in F (as ec_mul_kernel's inputs do) and fails the row.  An x >= 2^x_bits sets bit 3
// and fails the row; F is then evaluated at its low x_bits bits.  The verdict compares projectively
// (no inversion); points_out, when given, costs one inversion for the affine F.
__device__ __forceinline__ bool load_commitment(const uint8_t *p, Jac &out) {
    const uint4 *w = reinterpret_cast<const uint4 *>(p);
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) any |= w[k].x | w[k].y | w[k].z | w[k].w;
    const bool ok = load_point(p, out);
    if (any == 0 || !ok) out = jac_inf();
    return any == 0 || ok;
}

__global__ __launch_bounds__(kEcThreads) void feldman_verify_kernel(const uint8_t *__restrict__ commitments, int T,
                                                                    int M, const uint32_t *__restrict__ dealer,
                                                                    const uint32_t *__restrict__ xs, int x_bits,
                                                                    const uint8_t *__restrict__ shares, int n,
                                                                    uint8_t *__restrict__ ok_out,
                                                                    uint8_t *__restrict__ points_out,
                                                                    uint32_t *__restrict__ flags) {
    __builtin_amdgcn_s_setprio(3);  // one wave's issue chain sets the time, as the other EC kernels
    const size_t g = (size_t)blockIdx.x * kEcThreads + threadIdx.x;
    if (g >= (size_t)n) return;
    const uint32_t d = dealer ? dealer[g] : (uint32_t)(g % (size_t)M);
    const uint32_t x = xs[g];
    uint32_t fl = 0;
    if (x_bits < 32 && (x >> x_bits) != 0) fl |= 8u;
    const uint8_t *col = commitments + (size_t)d * 64;  // term k at col + k M 64

    // right-hand side: Horner from the top term
    Jac acc;
    if (!load_commitment(col + (size_t)(T - 1) * M * 64, acc)) fl |= 2u;
#pragma unroll 1
    for (int k = T - 2; k >= 0; --k) {
        Jac R = jac_inf();
#pragma unroll 1
        for (int b = x_bits - 1; b >= 0; --b) {
            R = jac_dbl(R);  // doubling infinity keeps Z = 0
            if ((x >> b) & 1u) R = jac_add(R, acc);
        }
        Jac C;
        if (!load_commitment(col + (size_t)k * M * 64, C)) fl |= 2u;
        acc = jac_add(R, C);
    }
    const bool f_inf = fe_is_zero(acc.Z);
    if (f_inf) fl |= 4u;
    if (points_out) {
        Fe px = {}, py = {};
        if (!f_inf) {
            // (Z R)^-1 R^3 R^-1 = Z^-1 R, the Montgomery form of Z^-1 (ec_finish_kernel)
            const Fe zi = fe_mul(fe_inv_bingcd(acc.Z), fe_const(kR3));
            const Fe zi2 = fe_sqr(zi);
            px = from_mont(fe_mul(acc.X, zi2));
            py = from_mont(fe_mul(acc.Y, fe_mul(zi2, zi)));
        }
        store_be(points_out + g * 64, px);
        store_be(points_out + g * 64 + 32, py);
    }

    // left-hand side: s G by the regular ladder's fixed-base half
    const Fe s = load_be(shares + g * 32);
    if (!sc_lt_n(s)) fl |= 1u;
    bool accept = false;
    if (fl == 0 || fl == 4u) {
        Regular ks = regular_recode(s);
        Jac L = fixed_base_add(jac_inf(), 0, ks.neg);  // the top digit: +-G
#pragma unroll 1
        for (int wnd = 0; wnd < 64; ++wnd) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) L = jac_dbl(L);
            L = fixed_base_step(L, ks);
        }
        // L == F without leaving Jacobian form: X1 Z2^2 == X2 Z1^2 and Y1 Z2^3 == Y2 Z1^3; infinity
        // equals only infinity
        const bool l_inf = fe_is_zero(L.Z);
        if (l_inf || f_inf) {
            accept = l_inf && f_inf;
        } else {
            const Fe z1 = fe_sqr(L.Z), z2 = fe_sqr(acc.Z);
            accept = fe_eq(fe_mul(L.X, z2), fe_mul(acc.X, z1)) &&
                     fe_eq(fe_mul(L.Y, fe_mul(z2, acc.Z)), fe_mul(acc.Y, fe_mul(z1, L.Z)));
        }
    }
    ok_out[g] = accept ? 1 : 0;
    if (flags) flags[g] = fl;
}

// ------------------------------------------------------------- AES-128-GCM keystream
// The m_i shares travel AES-128-GCM encrypted with the tag dropped (SA_ClientAgent.py:227-244,
// opened at :402-425 without a tag check), so both directions are data XOR keystream:
//     H = E_k(0^128);  J0 = nonce || 0x00000001 (12-byte nonce)
//                      J0 = GHASH_H(nonce || 0^64 || [128]_64) (16-byte nonce, pycryptodome's default)
//     out[16 m - 16 .. 16 m) = in ^ E_k(inc32^m(J0)),  m = 1, 2, ...    (NIST SP 800-38D, 7.1)
// One lane per message: its own key schedule (44 words in registers), S-box lookups in LDS.
// State columns are big-endian words (row 0 in the top byte).
constexpr int kAesThreads = 256;  // one S-box entry staged per lane

// keys: [n][16]; nonces: [n][nonce_len], nonce_len 12 or 16; in, out: [n][len], in == out allowed
__global__ __launch_bounds__(kAesThreads) void aes_gcm_xor_kernel(const uint8_t *__restrict__ keys,
                                                                  const uint8_t *__restrict__ nonces, int nonce_len,
                                                                  const uint8_t *in, uint8_t *out, uint32_t len, int n) {
    __shared__ uint8_t sb[256];
    sb[threadIdx.x] = kAesSbox[threadIdx.x];
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * kAesThreads + threadIdx.x;
    if (i >= (size_t)n) return;
    uint32_t rk[44];
#pragma unroll
    for (int w = 0; w < 4; ++w) rk[w] = load_be32(keys + i * 16 + 4 * w);
#pragma unroll
    for (int w = 4; w < 44; ++w) {
        uint32_t t = rk[w - 1];
        if (w % 4 == 0) {
            constexpr uint32_t rcon[10] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1b, 0x36};
            t = aes_sub_word(sb, rotl32(t, 8)) ^ (rcon[w / 4 - 1] << 24);
        }
        rk[w] = rk[w - 4] ^ t;
    }
    const uint8_t *nc = nonces + i * (size_t)nonce_len;
    uint32_t j0[4] = {load_be32(nc), load_be32(nc + 4), load_be32(nc + 8), 1u};
    const uint8_t *src = in + i * (size_t)len;
    uint8_t *dst = out + i * (size_t)len;
    const uint32_t blocks = (len + 15u) / 16u;
    // pass 0 encrypts the zero block (H, which a 16-byte nonce's J0 needs); pass m >= 1 is
    // keystream block m: one copy of the cipher's code for both
#pragma unroll 1
    for (uint32_t m = 0; m <= blocks; ++m) {
        uint32_t s[4] = {0, 0, 0, 0};
        if (m > 0) {
            s[0] = j0[0], s[1] = j0[1], s[2] = j0[2];
            s[3] = j0[3] + m;  // inc32: the low word wraps, nothing carries out of it
        }
        aes128_encrypt(sb, rk, s);
        if (m == 0) {
            if (nonce_len == 16) {
                j0[3] = load_be32(nc + 12);
                gcm_mul(j0, s);
                j0[3] ^= 128u;  // 0^64 || [128]_64
                gcm_mul(j0, s);
            }
            continue;
        }
        const uint32_t o = 16u * (m - 1u), cnt = len - o < 16u ? len - o : 16u;
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k)
            if (k < cnt) dst[o + k] = src[o + k] ^ (uint8_t)(s[k >> 2] >> (24u - 8u * (k & 3u)));
    }
}

// ------------------------------------------------------------- AES-128-GCM with its tag
// The whole of NIST SP 800-38D for AES-128, one lane per message like aes_gcm_xor_kernel:
//     H, J0 and C as above;  S = GHASH_H(A || 0* || C || 0* || [8 aad_len]_64 || [8 len]_64);
//     T = S ^ E_k(J0)        (J0 itself: the keystream starts at inc32(J0))
// Seal writes C and T.  Open recomputes T over the ciphertext it was given, compares all 16 bytes
// (OR of XORs, no early exit), writes ok[i] and then the plaintext -- or zero bytes where the tag
// is wrong, never unauthenticated plaintext.  in == out is allowed: seal reads a block before it
// writes it, open has hashed every block before it writes the first.
// One copy of the cipher's code per kernel: pass 0 encrypts the zero block, one pass J0 (the tag's
// mask; last for seal, which hashes C as it produces it, second for open, which needs the verdict
// before it writes), the others a keystream block each.  The lane holds the 44 round keys, H, J0
// and the GHASH accumulator; gcm_mul's loops stay rolled.
// keys: [n][16]; nonces: [n][nonce_len]; aad: [n][aad_len] (unread when aad_len is 0); in, out:
// [n][len] (unread when len is 0); tags: [n][16], written by seal and read by open; ok: [n], open only
template <bool kOpen>
__global__ __launch_bounds__(kAesThreads) void aes_gcm_auth_kernel(const uint8_t *__restrict__ keys,
                                                                   const uint8_t *__restrict__ nonces, int nonce_len,
                                                                   const uint8_t *__restrict__ aad, uint32_t aad_len,
                                                                   const uint8_t *in, uint8_t *out, uint32_t len,
                                                                   const uint8_t *tags_in, uint8_t *tags_out,
                                                                   uint8_t *ok_out, int n) {
    __shared__ uint8_t sb[256];
    sb[threadIdx.x] = kAesSbox[threadIdx.x];
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * kAesThreads + threadIdx.x;
    if (i >= (size_t)n) return;
    uint32_t rk[44];
    aes128_expand_key(sb, keys + i * 16, rk);
    const uint8_t *nc = nonces + i * (size_t)nonce_len;
    uint32_t j0[4] = {load_be32(nc), load_be32(nc + 4), load_be32(nc + 8), 1u};
    const uint8_t *src = in + i * (size_t)len;
    uint8_t *dst = out + i * (size_t)len;
    const uint32_t blocks = (len + 15u) / 16u;
    uint32_t h[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0};
    uint32_t open_mask = 0;  // all ones once open has found the tag right
#pragma unroll 1
    for (uint32_t t = 0; t <= blocks + 1u; ++t) {
        const bool tag_pass = kOpen ? t == 1u : t == blocks + 1u;
        const uint32_t m = kOpen ? t - 1u : t;  // the keystream block of a pass that is neither
        uint32_t s[4] = {0, 0, 0, 0};
        if (t > 0) {
            s[0] = j0[0], s[1] = j0[1], s[2] = j0[2];
            s[3] = j0[3] + (tag_pass ? 0u : m);  // inc32: the low word wraps, nothing carries out of it
        }
        aes128_encrypt(sb, rk, s);
        if (t == 0) {
#pragma unroll
            for (int w = 0; w < 4; ++w) h[w] = s[w];
            if (nonce_len == 16) {
                j0[3] = load_be32(nc + 12);
                gcm_mul(j0, h);
                j0[3] ^= 128u;  // 0^64 || [128]_64
                gcm_mul(j0, h);
            }
            ghash_absorb(y, h, aad + i * (size_t)aad_len, aad_len);
            if (kOpen) ghash_absorb(y, h, src, len);
            continue;
        }
        if (tag_pass) {
            y[1] ^= aad_len << 3;  // [8 aad_len]_64 || [8 len]_64: both far below 2^32
            y[3] ^= len << 3;
            gcm_mul(y, h);
#pragma unroll
            for (int w = 0; w < 4; ++w) s[w] ^= y[w];
            if (kOpen) {
                uint32_t diff = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) diff |= s[w] ^ load_be32(tags_in + i * 16 + 4 * w);
                open_mask = diff ? 0u : 0xffffffffu;
                ok_out[i] = (uint8_t)(open_mask & 1u);
            } else {
                store_block_be(tags_out + i * 16, 16u, s);
            }
            continue;
        }
        const uint32_t o = 16u * (m - 1u), cnt = len - o < 16u ? len - o : 16u;
        uint32_t b[4];
        load_block_be(src + o, cnt, b);
        if (kOpen) {
#pragma unroll
            for (int w = 0; w < 4; ++w) b[w] = (b[w] ^ s[w]) & open_mask;
        } else {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                b[w] = (b[w] ^ s[w]) & head_mask(cnt, w);  // the keystream behind the message is no ciphertext
                y[w] ^= b[w];
            }
            gcm_mul(y, h);
        }
        store_block_be(dst + o, cnt, b);
    }
}

// ------------------------------------------------------------- hash to curve
// The client's pairwise seed group element (SA_ClientAgent.py:275-286): h_ijt, a decimal string
// below 2^16, goes through util/crypto/ecchash.hash_str_to_curve(msg, count=2, modulus=n, degree=1,
// blen=48, XMDExpander(DST, sha256, 128)) (:277-283):
//   uniform = expand_message_xmd(msg, DST, 96)                                   (:90-133)
//   u_k     = OS2IP(uniform[48k : 48k + 48]) mod n      (the client passes n, not p: :285)  (:50-61)
//   Q_k     = map_to_curve(u_k)                                                   (:233-275)
//   H       = Q_0 + Q_1                                                           (:282)
// One lane per message, Montgomery field of the scalar-multiplication kernels.  map_to_curve is the
// reference's own simplified-SWU variant with Z = -10: tv1 = (100 u^4 - 10 u^2)^-1, x1 = -b/a (1 + tv1),
// x2 = -10 u^2 x1, y = the first square root of g(x1) else of g(x2).  Where the denominator is 0 (u = 0
// and u = +-sqrt(1/10), which no message reaches) the reference's libnum.invmod raises and its x1 =
// b/30 branch (:247-248) is dead; here the inverse is RFC 9380's inv0 (0 -> 0) and that branch is
// taken -- this project's choice.
// Square roots are a^((p+1)/4) (p = 3 mod 4): the root the host restatement (flamingo_amd/crypto.py)
// takes first for libnum's sqrtmod -- the one convention that stays "parity unpinned" (DESIGN.md).
// The sgn0 step (:271-272) flips y only when exactly one of u, y is zero.  The whole table of the
// protocol's 2^16 inputs is one launch (flm_hash_to_curve_decimal).
constexpr int kH2cMaxMsg = 64;
__device__ constexpr uint32_t kAm[8] = {0xfffffffcu, 0xffffffffu, 0xffffffffu, 0x00000003u,
                                        0x00000000u, 0x00000000u, 0x00000004u, 0xfffffffcu};  // a R (a = -3)
__device__ constexpr uint32_t kC1m[8] = {0x6341949fu, 0x9d899fcbu, 0x7d816585u, 0x8efaac9au,
                                         0xa7b5ba47u, 0xa1e0b58eu, 0x01826d67u, 0xf4100209u};  // (-b/a) R
__device__ constexpr uint32_t kC2m[8] = {0xf0535ba9u, 0x5c8dc32du, 0x8c8cf08du, 0xc17f77a9u,
                                         0x43f892a0u, 0x7696788eu, 0x99c03e24u, 0x98680033u};  // (b/30) R
__device__ constexpr uint32_t k10m[8] = {0x0000000au, 0x00000000u, 0x00000000u, 0xfffffff6u,
                                         0xffffffffu, 0xffffffffu, 0xfffffff5u, 0x00000009u};  // 10 R
__device__ constexpr uint32_t k100m[8] = {0x00000064u, 0x00000000u, 0x00000000u, 0xffffff9cu,
                                          0xffffffffu, 0xffffffffu, 0xffffff9bu, 0x00000063u};  // 100 R
__device__ constexpr uint32_t kNeg10m[8] = {0xfffffff5u, 0xffffffffu, 0xffffffffu, 0x0000000au,
                                            0x00000000u, 0x00000000u, 0x0000000bu, 0xfffffff5u};  // -10 R
__device__ constexpr uint32_t kNc[7] = {0x039cdaafu, 0x0c46353du, 0x58e8617bu, 0x43190552u,
                                        0x00000000u, 0x00000000u, 0xffffffffu};  // 2^256 - n (< 2^224)
// ecchash.test_dst("P256_XMD:SHA-256_SSWU_RO_") || I2OSP(44, 1): DST_prime of :104
__device__ constexpr uint8_t kDstPrime[45] = {'Q', 'U', 'U', 'X', '-', 'V', '0', '1', '-', 'C', 'S', '0', '2', '-', 'w',
                                              'i', 't', 'h', '-', 'P', '2', '5', '6', '_', 'X', 'M', 'D', ':', 'S', 'H',
                                              'A', '-', '2', '5', '6', '_', 'S', 'S', 'W', 'U', '_', 'R', 'O', '_', 44};

__device__ void sha_put_dst(Sha256 &s) {
#pragma unroll 1
    for (int i = 0; i < 45; ++i) sha_put(s, kDstPrime[i]);
}

// 384-bit big-endian words u[0..11] mod n: fold t = lo + hi (2^256 mod n) until t < 2^256, then one
// subtraction.  2^256 mod n < 2^224, so hi goes from 128 bits to at most 96, 64, 32, 1 and 0: five
// folds can meet a non-zero hi (random inputs need four or five, about half each) and the last two of
// the seven iterations always see hi = 0 and add nothing.  tools/h2c_reduce_model.py replays these
// limbs and carries in Python and proves the bound (fold_bound); the loop count is left as it was.
__device__ Fe mod_n_384(const uint32_t *u) {
    uint32_t t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = u[11 - i];
#pragma unroll 1
    for (int it = 0; it < 7; ++it) {
        uint32_t hi[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            hi[i] = t[8 + i];
            t[8 + i] = 0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint64_t c = 0;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                c = (uint64_t)hi[i] * kNc[j] + t[i + j] + (c >> 32);
                t[i + j] = (uint32_t)c;
            }
            c >>= 32;
#pragma unroll
            for (int k = i + 7; k < 12; ++k) {
                c += t[k];
                t[k] = (uint32_t)c;
                c >>= 32;
            }
        }
    }
    Fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = t[i];
    return sc_below_n(r);
}

// Montgomery-form inverse by binary GCD (ec_finish_kernel's: ~25k VALU instructions against Fermat's
// ~73k): (a R)^-1 R^3 R^-1 = a^-1 R; 0 -> 0 (RFC 9380's inv0: h2c_map's x1 = b/30 branch)
__device__ __forceinline__ Fe fe_inv_mont(const Fe &a) {
    if (fe_is_zero(a)) return a;
    return fe_mul(fe_inv_bingcd(a), fe_const(kR3));
}

__device__ __forceinline__ Fe fe_sqr_n(Fe a, int n) {
#pragma unroll 1
    for (int i = 0; i < n; ++i) a = fe_sqr(a);
    return a;
}

// a^((p+1)/4), (p+1)/4 = (2^32 - 1) 2^222 + 2^190 + 2^94: 253 squarings, 7 multiplications
__device__ Fe fe_sqrt_cand(const Fe &a) {
    const Fe x2 = fe_mul(fe_sqr(a), a);
    const Fe x4 = fe_mul(fe_sqr_n(x2, 2), x2);
    const Fe x8 = fe_mul(fe_sqr_n(x4, 4), x4);
    const Fe x16 = fe_mul(fe_sqr_n(x8, 8), x8);
    const Fe x32 = fe_mul(fe_sqr_n(x16, 16), x16);
    Fe r = fe_mul(fe_sqr_n(x32, 32), a);
    r = fe_mul(fe_sqr_n(r, 96), a);
    return fe_sqr_n(r, 94);
}

// map_to_curve (ecchash.py:233-275) of u (canonical, < n < p), affine Montgomery (x, y); bad = neither
// g(x1) nor g(x2) had a root (cannot happen for this map; flagged rather than assumed)
__device__ void h2c_map(const Fe &u_plain, Fe &x, Fe &y, bool &bad) {
    const Fe u = to_mont(u_plain);
    const Fe u2 = fe_sqr(u);
    const Fe u4 = fe_sqr(u2);
    const Fe den = fe_sub(fe_mul(fe_const(k100m), u4), fe_mul(fe_const(k10m), u2));
    const Fe tv1 = fe_inv_mont(den);                              // inv0: 0 -> 0, then x1 = b/30
    Fe x1 = fe_mul(fe_const(kC1m), fe_add(fe_const(kOne), tv1));
    if (fe_is_zero(tv1)) x1 = fe_const(kC2m);
    const Fe gx1 = fe_add(fe_mul(x1, fe_add(fe_sqr(x1), fe_const(kAm))), fe_const(kBm));
    const Fe x2 = fe_mul(fe_const(kNeg10m), fe_mul(u2, x1));
    const Fe gx2 = fe_add(fe_mul(x2, fe_add(fe_sqr(x2), fe_const(kAm))), fe_const(kBm));
    const Fe y1 = fe_sqrt_cand(gx1);
    const bool sq1 = fe_eq(fe_sqr(y1), gx1);
    const Fe y2 = fe_sqrt_cand(gx2);
    bad = !sq1 && !fe_eq(fe_sqr(y2), gx2);
    x = sq1 ? x1 : x2;
    y = sq1 ? y1 : y2;
    if (fe_is_zero(u_plain) != fe_is_zero(y)) y = fe_neg(y);    // sgn0(u) != sgn0(y), :271-272
}

// Everything after expand_message_xmd, for both kernels below: uni is the lane's 24 big-endian words
// of uniform bytes (of message i; lane `half` of its pair takes words 12 half .. 12 half + 11).  Lane
// 2m maps u_0 and lane 2m+1 maps u_1, then the odd lane hands its point to the even one (a lane
// swap, no LDS), which adds, inverts and stores out row i and flags[i].  Lanes with !valid (i >= n)
// compute on whatever uni holds and store nothing: both lanes of a pair stay to the swap.
// Inlined into each kernel: as a shared out-of-line function it took hash_to_curve_kernel from 152 to
// 200 VGPRs (3 -> 2 waves per SIMD); inlined, that kernel's code is what it was with the tail written
// in place.
__device__ __forceinline__ void h2c_tail(const uint32_t *uni, bool valid, int half, int i, uint8_t *__restrict__ out,
                                         uint32_t *__restrict__ flags) {
    Fe x, y;
    bool bad;
    h2c_map(mod_n_384(half ? uni + 12 : uni), x, y, bad);   // Q_half = map_to_curve(u_half)
    Fe x1, y1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        x1.v[k] = (uint32_t)__shfl_xor((int)x.v[k], 1);
        y1.v[k] = (uint32_t)__shfl_xor((int)y.v[k], 1);
    }
    const bool bad1 = __shfl_xor((int)bad, 1) != 0;
    if (!valid || half) return;
    Jac Q0, Q1;
    Q0.X = x;
    Q0.Y = y;
    Q0.Z = fe_const(kOne);
    Q1.X = x1;
    Q1.Y = y1;
    Q1.Z = fe_const(kOne);
    const Jac R = jac_add(Q0, Q1);                                 // Q0 + Q1 (:282), P == +-Q handled
    uint32_t fl = (bad || bad1) ? 8u : 0u;
    Fe ax = {}, ay = {};
    if (fe_is_zero(R.Z)) {
        fl |= 4u;
    } else {
        const Fe zi = fe_inv_mont(R.Z);
        const Fe zi2 = fe_sqr(zi);
        ax = from_mont(fe_mul(R.X, zi2));
        ay = from_mont(fe_mul(R.Y, fe_mul(zi2, zi)));
    }
    store_be(out + (size_t)i * 64, ax);
    store_be(out + (size_t)i * 64 + 32, ay);
    flags[i] = fl;
}

// msgs: n x kH2cMaxMsg bytes (message i in its first lens[i] bytes), or NULL for the decimal
// strings of v0 + i (str(h_ijt), SA_ClientAgent.py:280).  out: n x 64 wire bytes (infinity: zeros,
// flags bit 2); flags bit 3: no square root (not expected).
// Two adjacent lanes per message: both expand it (9 SHA-256 compressions, cheap next to the field
// work), lane 2m maps u_0 and lane 2m+1 maps u_1 -- the two map_to_curve calls are independent, so
// the chain a lane runs is one inversion + two square roots instead of two of each -- then the odd
// lane hands its point to the even one (a lane swap, no LDS), which adds, inverts and stores.
__global__ __launch_bounds__(kEcThreads) void hash_to_curve_kernel(const uint8_t *__restrict__ msgs,
                                                                   const uint32_t *__restrict__ lens, uint32_t v0,
                                                                   int n, uint8_t *__restrict__ out,
                                                                   uint32_t *__restrict__ flags) {
    const int t = blockIdx.x * kEcThreads + threadIdx.x;
    const int i = t >> 1, half = t & 1;
    const bool valid = i < n;  // both lanes of a pair stay to the swap: no early return
    uint8_t msg[kH2cMaxMsg];
    int m = 0;
    if (valid && msgs) {
        m = (int)lens[i];
#pragma unroll 1
        for (int k = 0; k < m; ++k) msg[k] = msgs[(size_t)i * kH2cMaxMsg + k];
    } else if (valid) {
        uint32_t v = v0 + (uint32_t)i;
        uint8_t dig[10];
        int nd = 0;
#pragma unroll 1
        do {
            dig[nd++] = (uint8_t)('0' + v % 10);
            v /= 10;
        } while (v);
#pragma unroll 1
        for (int k = 0; k < nd; ++k) msg[k] = dig[nd - 1 - k];
        m = nd;
    }
    // b_0 = H(Z_pad || msg || I2OSP(96, 2) || I2OSP(0, 1) || DST_prime)   (:113-114)
    Sha256 s;
    sha_init(s);
    sha256_block(s.h, s.w);  // Z_pad: one all-zero block (s.w is zero)
    s.total = 64;
#pragma unroll 1
    for (int k = 0; k < m; ++k) sha_put(s, msg[k]);
    sha_put(s, 0);
    sha_put(s, 96);
    sha_put(s, 0);
    sha_put_dst(s);
    uint32_t b0[8], bi[8], uni[24];
    sha_final(s, b0);
    // b_1 = H(b_0 || 1 || DST_prime), b_i = H((b_0 ^ b_{i-1}) || i || DST_prime)   (:115-117)
#pragma unroll
    for (int k = 0; k < 8; ++k) bi[k] = 0;
#pragma unroll 1
    for (int blk = 1; blk <= 3; ++blk) {
        sha_init(s);
#pragma unroll 1
        for (int k = 0; k < 32; ++k) sha_put(s, (b0[k >> 2] ^ bi[k >> 2]) >> (24 - 8 * (k & 3)));
        sha_put(s, (uint32_t)blk);
        sha_put_dst(s);
        sha_final(s, bi);
#pragma unroll
        for (int k = 0; k < 8; ++k) uni[(blk - 1) * 8 + k] = bi[k];
    }
    h2c_tail(uni, valid, half, i, out, flags);
}

// The same tail on uniform bytes the caller chose (flm_h2c_from_uniform, for the tests: no message
// reaches u = 0, the roots of 1/10, Q0 = +-Q1 or a late fold of mod_n_384).  uniform: n x 96 bytes,
// what expand_message_xmd(msg, DST, 96) would give; out and flags as above.  Lanes with i >= n read
// nothing and stay for the swap.
__global__ __launch_bounds__(kEcThreads) void h2c_from_uniform_kernel(const uint8_t *__restrict__ uniform, int n,
                                                                      uint8_t *__restrict__ out,
                                                                      uint32_t *__restrict__ flags) {
    const int t = blockIdx.x * kEcThreads + threadIdx.x;
    const int i = t >> 1, half = t & 1;
    const bool valid = i < n;
    uint32_t uni[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) uni[k] = 0;
    if (valid) {
        const uint8_t *row = uniform + (size_t)i * 96;
#pragma unroll 1
        for (int k = 0; k < 24; ++k)
            uni[k] = (uint32_t)row[4 * k] << 24 | (uint32_t)row[4 * k + 1] << 16 | (uint32_t)row[4 * k + 2] << 8 |
                     (uint32_t)row[4 * k + 3];
    }
    h2c_tail(uni, valid, half, i, out, flags);
}

}  // namespace

template <int TPB, int WPE>
static void launch_ec_mul_t(const uint8_t *d_points, const uint8_t *d_scalars, int per_element, int T, int D,
                            uint32_t *d_jac, uint32_t *d_flags, hipStream_t stream, unsigned lds_pad) {
    const size_t n = (size_t)T * D;
    hipLaunchKernelGGL((ec_mul_kernel<TPB, WPE>), dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), lds_pad, stream,
                       d_points, d_scalars, per_element, T, D, d_jac, d_flags);
}

// threads: lanes per workgroup (64/128/256); waves: register budget, as minimum waves per SIMD
// (2: no cap, 172 VGPRs; 4: 128 VGPRs; 8: 64 VGPRs, both with spills)
int ec_mul_groups(int T, int terms) { return terms > 1 ? (T + terms - 1) / terms : T; }

hipError_t launch_ec_mul(const uint8_t *d_points, const uint8_t *d_scalars, int per_element, int T, int D,
                         uint32_t *d_jac, uint32_t *d_flags, hipStream_t stream, int threads, int waves, int coop,
                         int terms, unsigned lds_pad) {
    if (T <= 0 || D <= 0) return hipSuccess;
    if (terms > 1 && !per_element) {
        const size_t n = (size_t)ec_mul_groups(T, terms) * D;
        const dim3 grid((unsigned)((n + kEcThreads - 1) / kEcThreads));
        if (terms == 2)
            hipLaunchKernelGGL(ec_mul_straus_kernel<2>, grid, dim3(kEcThreads), lds_pad, stream, d_points, d_scalars, T, D,
                               d_jac, d_flags);
        else if (terms == 4)
            hipLaunchKernelGGL(ec_mul_straus_kernel<4>, grid, dim3(kEcThreads), lds_pad, stream, d_points, d_scalars, T, D,
                               d_jac, d_flags);
        else
            return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (coop == 2) {  // one element per 16-lane row: four scalar multiplications per workgroup
        const size_t n = (size_t)T * D;
        hipLaunchKernelGGL(ec_mul_row_kernel, dim3((unsigned)((n + 3) / 4)), dim3(64 * kCoopWaves), 0, stream,
                           d_points, d_scalars, per_element, T, D, d_jac, d_flags);
        return hipGetLastError();
    }
    if (coop) {
        const size_t n = (size_t)T * D;
        hipLaunchKernelGGL(ec_mul_coop_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64 * kCoopWaves), 0, stream,
                           d_points, d_scalars, per_element, T, D, d_jac, d_flags);
        return hipGetLastError();
    }
#define FLM_EC(TPB)                                                                                          \
    switch (waves) {                                                                                         \
        case 4: launch_ec_mul_t<TPB, 4>(d_points, d_scalars, per_element, T, D, d_jac, d_flags, stream, lds_pad); break; \
        case 8: launch_ec_mul_t<TPB, 8>(d_points, d_scalars, per_element, T, D, d_jac, d_flags, stream, lds_pad); break; \
        default: launch_ec_mul_t<TPB, 1>(d_points, d_scalars, per_element, T, D, d_jac, d_flags, stream, lds_pad); break; \
    }
    switch (threads) {
        case 64: FLM_EC(64) break;
        case 128: FLM_EC(128) break;
        default: FLM_EC(256) break;
    }
#undef FLM_EC
    return hipGetLastError();
}

hipError_t launch_shamir_combine(const uint8_t *d_shares, const uint8_t *d_lambdas, int T, int M, uint8_t *d_out,
                                 hipStream_t stream) {
    if (M <= 0) return hipSuccess;
    dim3 grid((M + kEcThreads - 1) / kEcThreads);
    hipLaunchKernelGGL(shamir_combine_kernel, grid, dim3(kEcThreads), 0, stream, d_shares, d_lambdas, T, M, d_out);
    return hipGetLastError();
}

hipError_t launch_shamir_deal(const uint8_t *d_coeffs, int T, int M, const uint32_t *d_xs, int C, uint8_t *d_out,
                              hipStream_t stream) {
    if (T <= 0 || M <= 0 || C <= 0) return hipSuccess;
    const size_t lanes = (size_t)C * (size_t)M;
    hipLaunchKernelGGL(shamir_deal_kernel, dim3((unsigned)((lanes + kEcThreads - 1) / kEcThreads)), dim3(kEcThreads), 0,
                       stream, d_coeffs, T, M, d_xs, C, d_out);
    return hipGetLastError();
}

hipError_t launch_aes_gcm_xor(const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len, const uint8_t *d_in,
                              uint8_t *d_out, uint32_t len, int n, hipStream_t stream) {
    if (n <= 0 || len == 0) return hipSuccess;
    hipLaunchKernelGGL(aes_gcm_xor_kernel, dim3((unsigned)(((size_t)n + kAesThreads - 1) / kAesThreads)),
                       dim3(kAesThreads), 0, stream, d_keys, d_nonces, nonce_len, d_in, d_out, len, n);
    return hipGetLastError();
}

hipError_t launch_aes_gcm_seal(const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len, const uint8_t *d_aad,
                               uint32_t aad_len, const uint8_t *d_in, uint8_t *d_out, uint32_t len, uint8_t *d_tags,
                               int n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(aes_gcm_auth_kernel<false>, dim3((unsigned)(((size_t)n + kAesThreads - 1) / kAesThreads)),
                       dim3(kAesThreads), 0, stream, d_keys, d_nonces, nonce_len, d_aad, aad_len, d_in, d_out, len,
                       (const uint8_t *)nullptr, d_tags, (uint8_t *)nullptr, n);
    return hipGetLastError();
}

hipError_t launch_aes_gcm_open(const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len, const uint8_t *d_aad,
                               uint32_t aad_len, const uint8_t *d_in, const uint8_t *d_tags, uint8_t *d_out,
                               uint32_t len, uint8_t *d_ok, int n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(aes_gcm_auth_kernel<true>, dim3((unsigned)(((size_t)n + kAesThreads - 1) / kAesThreads)),
                       dim3(kAesThreads), 0, stream, d_keys, d_nonces, nonce_len, d_aad, aad_len, d_in, d_out, len, d_tags,
                       (uint8_t *)nullptr, d_ok, n);
    return hipGetLastError();
}

hipError_t launch_ecdsa_verify(const uint8_t *d_pubkeys, const uint8_t *d_digests, const uint8_t *d_sigs, int n,
                               uint8_t *d_ok, uint32_t *d_flags, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ecdsa_verify_kernel, dim3((unsigned)(((size_t)n + kEcThreads - 1) / kEcThreads)),
                       dim3(kEcThreads), 0, stream, d_pubkeys, d_digests, d_sigs, n, d_ok, d_flags);
    return hipGetLastError();
}

hipError_t launch_feldman_verify(const uint8_t *d_commitments, int T, int M, const uint32_t *d_dealer,
                                 const uint32_t *d_xs, int x_bits, const uint8_t *d_shares, int n, uint8_t *d_ok,
                                 uint8_t *d_points, uint32_t *d_flags, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(feldman_verify_kernel, dim3((unsigned)(((size_t)n + kEcThreads - 1) / kEcThreads)),
                       dim3(kEcThreads), 0, stream, d_commitments, T, M, d_dealer, d_xs, x_bits, d_shares, n, d_ok,
                       d_points, d_flags);
    return hipGetLastError();
}

hipError_t launch_ec_finish(const uint8_t *d_base, const uint32_t *d_jac, int T, int D, int negate,
                            uint8_t *d_points_out, uint8_t *d_digests_out, uint32_t *d_flags, hipStream_t stream) {
    if (D <= 0) return hipSuccess;
    constexpr int per_group = kEcThreads / kFinishLanes;
    dim3 grid((D + per_group - 1) / per_group);
    hipLaunchKernelGGL(ec_finish_kernel, grid, dim3(kEcThreads), 0, stream, d_base, d_jac, T, D, negate,
                       d_points_out, d_digests_out, d_flags);
    return hipGetLastError();
}

hipError_t launch_hash_to_curve(const uint8_t *d_msgs, const uint32_t *d_lens, uint32_t v0, int n, uint8_t *d_out,
                                uint32_t *d_flags, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const size_t lanes = 2 * (size_t)n;  // two lanes per message
    hipLaunchKernelGGL(hash_to_curve_kernel, dim3((unsigned)((lanes + kEcThreads - 1) / kEcThreads)), dim3(kEcThreads),
                       0, stream, d_msgs, d_lens, v0, n, d_out, d_flags);
    return hipGetLastError();
}

hipError_t launch_h2c_from_uniform(const uint8_t *d_uniform, int n, uint8_t *d_out, uint32_t *d_flags,
                                   hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const size_t lanes = 2 * (size_t)n;
    hipLaunchKernelGGL(h2c_from_uniform_kernel, dim3((unsigned)((lanes + kEcThreads - 1) / kEcThreads)),
                       dim3(kEcThreads), 0, stream, d_uniform, n, d_out, d_flags);
    return hipGetLastError();
}

}  // namespace flm
