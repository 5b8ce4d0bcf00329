// flm_kernels.hip -- gfx950 (CDNA4) kernels for Flamingo's mask-and-aggregate path.
//
// Reference behaviour (paths relative to the reference root):
//   PRG(seed)[l] = LE32(ChaCha20_DJB(seed, nonce 0^8) word l) ^ 0x64636261
//     -- ChaCha20.new(key=seed, nonce=param.nonce).encrypt(param.fixed_key*L)
//        + np.frombuffer(..,'uint32'): agent/flamingo/SA_ServiceAgent.py:533-536,
//        596-603; agent/flamingo/SA_ClientAgent.py:248-250, 296-298.
//   partial sum        S = sum_i y_i          SA_ServiceAgent.py:346-350
//   self-mask unmask   M = -sum_i PRG(m_i)    SA_ServiceAgent.py:529-536
//   dropout-pair unmask C = sum sigma PRG(s)  SA_ServiceAgent.py:587-603
//   final              out = S + C + M        SA_ServiceAgent.py:538-540, 605
//   client masking     y = x + PRG(m) +- PRG(s_ij)   SA_ClientAgent.py:304-324
//
// Design (MI355X-first):
//   * Integer elementwise work: VALU only, no MFMA.  ChaCha20 is ~59 VALU ops
//     per output word, so regenerating masks is VALU-bound; summing rows is
//     HBM-bound.  One kernel does both so the two overlap inside every wave.
//   * A wave owns a 1024-slot sub-tile.  Masks are generated in "block layout"
//     (lane t computes ChaCha block t: slots 16t..16t+15) and never written to
//     HBM; rows are streamed in "coalesced layout" (lane t loads 16 B at
//     slot 4t + 256j, j = 0..3: every load instruction is 1 KiB contiguous).
//     The two layouts meet once per work item, through LDS.
//   * Signs fold into the XOR constant: -(ks ^ C) = (ks ^ ~C) + 1 mod 2^32, so
//     every seed costs one v_xad_u32 per word and the "+1" per negative seed
//     is added once per slot as a bias (count kept on the device).
//   * Everything of ChaCha's first double round that does not depend on the
//     block counter is computed once per seed (SeedRec), not per block.
//   * 1024-thread workgroups: 16 waves split an item's rows/seeds, partial
//     sums are combined through LDS; tiles shared by several items are
//     combined with u32 atomics (exact: integer adds commute).
#include <cmath>
#include <cstring>

#include "flm_internal.h"

namespace flm {

#define FLM_ROTL(v, c) __builtin_rotateleft32((v), (c))
#define FLM_QR(a, b, c, d)                       \
    a += b; d ^= a; d = FLM_ROTL(d, 16);          \
    c += d; b ^= c; b = FLM_ROTL(b, 12);          \
    a += b; d ^= a; d = FLM_ROTL(d, 8);           \
    c += d; b ^= c; b = FLM_ROTL(b, 7);

// Rounds 2..10 as ONE inline-asm statement per half round: the four quarter rounds in lockstep
// (each of the QR's 12 steps issues for all four QRs back to back: 4 adds, 4 xors, 4 rotates,
// ...), and an s_nop after every rotate.  gfx950 issues v_add_u32 / v_xor_b32 in about 2 cycles
// and the v_alignbit_b32 rotate in about 4 (profiles/r01_isa_probe3.log); a wave that issues a
// rotate right behind another rotate, or right before the add that reads it, holds up the SIMD
// for the other waves.  Measured on the c4 mask-only launch (tools/ab/ab_variants.sh,
// profiles/r02_ab_nops.log; 1024 seeds x 2^20 slots, 8 waves/SIMD):
//   one asm statement per instruction (round 1: the compiler then pads each statement boundary
//   where the next reads what the previous wrote with an s_nop 0, i.e. after every group of 4)  1.426 ms
//   one statement, no s_nop                                                                      1.60
//   one statement, s_nop 0 after every group of 4                                                1.394
//   one statement, s_nop 0 after every rotate (and after every group)                            1.297
//   one statement, s_nop 1 after each of the first three rotates, s_nop 2 after the fourth,
//   nothing between the adds and xors (FLM_GAP_* defaults below)                                 1.176
// Gaps between simple ops cost time; gaps after rotates buy it.
#define FLM_GAP_A1 ""  // between the 2nd and 3rd add of a step
#define FLM_GAP_AX ""  // adds -> xors
#define FLM_GAP_X1 ""  // between the 2nd and 3rd xor
#define FLM_GAP_XR ""  // xors -> rotates
#define FLM_GAP_R0 "s_nop 1\n\t"  // after the 1st rotate
#define FLM_GAP_R1 "s_nop 1\n\t"  // after the 2nd rotate
#define FLM_GAP_R2 "s_nop 1\n\t"  // after the 3rd rotate
#define FLM_GAP_RA "s_nop 2\n\t"  // after the 4th rotate, before the adds that read them
#define FLM_S_A(a, b) "v_add_u32 %[" #a "], %[" #b "], %[" #a "]\n\t"
#define FLM_S_X(a, b) "v_xor_b32 %[" #a "], %[" #b "], %[" #a "]\n\t"
#define FLM_S_R(a, s) "v_alignbit_b32 %[" #a "], %[" #a "], %[" #a "], " #s "\n\t"  // rotl(a, 32 - s)
// one QR step for QRs 0..3: a += b; d ^= a; d = rotl(d, 32 - s)
#define FLM_S_STEP(a, b, c, d, s)                                                                       \
    FLM_S_A(a##0, b##0) FLM_S_A(a##1, b##1) FLM_GAP_A1 FLM_S_A(a##2, b##2) FLM_S_A(a##3, b##3) FLM_GAP_AX \
    FLM_S_X(d##0, a##0) FLM_S_X(d##1, a##1) FLM_GAP_X1 FLM_S_X(d##2, a##2) FLM_S_X(d##3, a##3) FLM_GAP_XR \
    FLM_S_R(d##0, s) FLM_GAP_R0 FLM_S_R(d##1, s) FLM_GAP_R1 FLM_S_R(d##2, s) FLM_GAP_R2 FLM_S_R(d##3, s)  \
    FLM_GAP_RA
// QR(a_i, b_i, c_i, d_i) for i = 0..3: steps (a,b,d,16) (c,d,b,12) (a,b,d,8) (c,d,b,7)
#define FLM_QR4(A0, B0, C0, D0, A1, B1, C1, D1, A2, B2, C2, D2, A3, B3, C3, D3)                   \
    asm volatile(FLM_S_STEP(a, b, c, d, 16) FLM_S_STEP(c, d, a, b, 20) FLM_S_STEP(a, b, c, d, 24)  \
                 FLM_S_STEP(c, d, a, b, 25)                                                     \
                 : [a0] "+v"(A0), [b0] "+v"(B0), [c0] "+v"(C0), [d0] "+v"(D0), [a1] "+v"(A1),   \
                   [b1] "+v"(B1), [c1] "+v"(C1), [d1] "+v"(D1), [a2] "+v"(A2), [b2] "+v"(B2),   \
                   [c2] "+v"(C2), [d2] "+v"(D2), [a3] "+v"(A3), [b3] "+v"(B3), [c3] "+v"(C3),   \
                   [d3] "+v"(D3))

// ------------------------------------------------------------------ seeds
// One thread per seed builds its SeedRec from the raw 32 seed bytes and sign.
// Workgroup p writes its count of negative / invalid signs to meta[2+2p],
// meta[3+2p] and meta[0] = number of workgroups, so no zeroing pass is needed.
// zero_out/zero_n: when the round's plan adds into its output with atomics, the same
// launch zero-fills it (grid-stride, 16-B stores) -- one submission fewer than a memset.
__global__ __launch_bounds__(256) void seed_schedule_kernel(const uint8_t *__restrict__ seeds,
                                                            const int8_t *__restrict__ signs, int K,
                                                            SeedRec *__restrict__ recs,
                                                            uint32_t *__restrict__ meta,
                                                            uint32_t *__restrict__ zero_out, uint64_t zero_n) {
    if (zero_out) {
        const uint64_t quads = zero_n / 4, stride = (uint64_t)gridDim.x * blockDim.x;
        for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride)
            reinterpret_cast<uint4 *>(zero_out)[q] = make_uint4(0u, 0u, 0u, 0u);
        const uint64_t t = 4 * quads + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (t < zero_n) zero_out[t] = 0u;
    }
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t neg = 0, bad = 0;
    if (k < K) {
        const uint8_t *p = seeds + 32 * (size_t)k;
        uint32_t key[8];
        if (((uintptr_t)seeds & 15) == 0) {
            const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
            key[0] = a.x; key[1] = a.y; key[2] = a.z; key[3] = a.w;
            key[4] = b.x; key[5] = b.y; key[6] = b.z; key[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                key[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
                         ((uint32_t)p[4 * i + 3] << 24);
        }
        const int sg = signs[k];
        neg = (sg < 0);
        bad = (sg != 1 && sg != -1);
        SeedRec r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r.k[i] = key[i];
        r.xorc = sg < 0 ? ~kAbcd : kAbcd;
        r.a0 = kSigma0 + key[0];
        uint32_t x1 = kSigma1, x5 = key[1], x9 = key[5], x13 = 0u;
        uint32_t x2 = kSigma2, x6 = key[2], x10 = key[6], x14 = 0u;
        uint32_t x3 = kSigma3, x7 = key[3], x11 = key[7], x15 = 0u;
        FLM_QR(x1, x5, x9, x13);
        FLM_QR(x2, x6, x10, x14);
        FLM_QR(x3, x7, x11, x15);
        r.col1[0] = x1; r.col1[1] = x5; r.col1[2] = x9; r.col1[3] = x13;
        r.col2[0] = x2; r.col2[1] = x6; r.col2[2] = x10; r.col2[3] = x14;
        r.col3[0] = x3; r.col3[1] = x7; r.col3[2] = x11; r.col3[3] = x15;
#pragma unroll
        for (int i = 0; i < 10; ++i) r.pad[i] = 0;
        recs[k] = r;
    }
    // workgroup totals (64-lane ballots, then 4 waves through LDS)
    __shared__ uint32_t s_cnt[2][4];
    const unsigned long long bn = __ballot(neg != 0), bb = __ballot(bad != 0);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_cnt[0][w] = __popcll(bn); s_cnt[1][w] = __popcll(bb); }
    __syncthreads();
    if (threadIdx.x == 0) {
        meta[2 + 2 * blockIdx.x] = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
        meta[3 + 2 * blockIdx.x] = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
        if (blockIdx.x == 0) meta[0] = gridDim.x;
    }
}

// Total negative signs of the current seed table (sum of the per-workgroup counts).
__device__ __forceinline__ uint32_t meta_nneg(const uint32_t *__restrict__ meta) {
    const uint32_t parts = meta[0];
    uint32_t n = 0;
    for (uint32_t p = 0; p < parts; ++p) n += meta[2 + 2 * p];
    return n;
}

// -------------------------------------------------------------- ChaCha core
// m[i] += ChaCha20_block(seed, ctr)[i] ^ xorc for the 16 words of block `ctr`.
// `rec` is wave-uniform (scalar loads); `ctr` is per lane.
__device__ __forceinline__ void chacha_mask_add(const SeedRec *__restrict__ rec, uint32_t ctr,
                                                uint32_t (&m)[16]) {
    const uint32_t k0 = rec->k[0], k1 = rec->k[1], k2 = rec->k[2], k3 = rec->k[3];
    const uint32_t k4 = rec->k[4], k5 = rec->k[5], k6 = rec->k[6], k7 = rec->k[7];
    const uint32_t xc = rec->xorc;
    uint32_t x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, x10, x11, x12, x13, x14, x15;
    // round 1, column QR(0,4,8,12): a = sigma0 + k0 precomputed
    x0 = rec->a0;
    x12 = FLM_ROTL(ctr ^ x0, 16);
    x8 = k4 + x12;
    x4 = FLM_ROTL(k0 ^ x8, 12);
    x0 += x4;
    x12 = FLM_ROTL(x12 ^ x0, 8);
    x8 += x12;
    x4 = FLM_ROTL(x4 ^ x8, 7);
    // round 1, columns 1..3: counter independent
    x1 = rec->col1[0]; x5 = rec->col1[1]; x9 = rec->col1[2]; x13 = rec->col1[3];
    x2 = rec->col2[0]; x6 = rec->col2[1]; x10 = rec->col2[2]; x14 = rec->col2[3];
    x3 = rec->col3[0]; x7 = rec->col3[1]; x11 = rec->col3[2]; x15 = rec->col3[3];
    // round 1, diagonals
    // the whole diagonal round in lockstep, like rounds 2..10: 0.8 % faster than the compiler's order
    // with the first steps of QR(1,6,11,12) and QR(2,7,8,13) hoisted into SeedRec
    // (profiles/r02_ab_round1.log)
    FLM_QR4(x0, x5, x10, x15, x1, x6, x11, x12, x2, x7, x8, x13, x3, x4, x9, x14);
    // rounds 2..10
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        FLM_QR4(x0, x4, x8, x12, x1, x5, x9, x13, x2, x6, x10, x14, x3, x7, x11, x15);
        FLM_QR4(x0, x5, x10, x15, x1, x6, x11, x12, x2, x7, x8, x13, x3, x4, x9, x14);
    }
    // feed-forward (input words 13..15 are zero), fold "abcd"/sign, accumulate
    m[0] += (x0 + kSigma0) ^ xc;
    m[1] += (x1 + kSigma1) ^ xc;
    m[2] += (x2 + kSigma2) ^ xc;
    m[3] += (x3 + kSigma3) ^ xc;
    m[4] += (x4 + k0) ^ xc;
    m[5] += (x5 + k1) ^ xc;
    m[6] += (x6 + k2) ^ xc;
    m[7] += (x7 + k3) ^ xc;
    m[8] += (x8 + k4) ^ xc;
    m[9] += (x9 + k5) ^ xc;
    m[10] += (x10 + k6) ^ xc;
    m[11] += (x11 + k7) ^ xc;
    m[12] += (x12 + ctr) ^ xc;
    m[13] += x13 ^ xc;
    m[14] += x14 ^ xc;
    m[15] += x15 ^ xc;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Load the wave's 4 KiB of one row in coalesced layout through a buffer
// descriptor whose range ends at the tile's last valid quad: quads past it
// (tail tile) come back as zero from the hardware range check, no branches.
// BL = block layout: lane t loads its own 64 B (slots 16t..16t+15), the layout
// the ChaCha block is generated in; otherwise coalesced layout (slot 4t + 256j).
// AUX = buffer cache-policy bits (0 default, 2 = nt: streamed once, MI355X_MICROARCH.md nt-weights).
template <bool BL, int AUX = 0>
__device__ __forceinline__ void load_row(const uint32_t *base, uint32_t bytes, int lane, u32x4 (&v)[4]) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(base), 0,
                                                                        (int)bytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        v[j] = __builtin_bit_cast(
            u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, BL ? 64 * lane + 16 * j : 16 * lane + 1024 * j, 0, AUX));
}

// Sum the Cw chunk partials of every sub-tile from LDS and write the tile.
template <int S>
__device__ __forceinline__ void reduce_out(const u32x4 *__restrict__ lds, uint32_t *__restrict__ out,
                                           uint64_t base, int valid, uint32_t bias, bool atomic) {
    constexpr int Cw = kWavesPerGroup / S;
    if (!atomic) {
        for (int q = threadIdx.x; q < S * 256; q += kThreads) {
            const int s = q >> 8, p = q & 255;
            u32x4 acc = u32x4(bias);
#pragma unroll
            for (int c = 0; c < Cw; ++c) acc = acc + lds[(s + S * c) * 256 + p];
            const int slot = s * kWaveSlots + 4 * p;
            uint32_t *dst = out + base + slot;
            if (slot + 3 < valid) {
                *reinterpret_cast<u32x4 *>(dst) = acc;
            } else {
                if (slot + 0 < valid) dst[0] = acc.x;
                if (slot + 1 < valid) dst[1] = acc.y;
                if (slot + 2 < valid) dst[2] = acc.z;
            }
        }
    } else {
        const uint32_t *l32 = reinterpret_cast<const uint32_t *>(lds);
        for (int d = threadIdx.x; d < S * kWaveSlots; d += kThreads) {
            const int s = d >> 10, o = d & 1023;
            uint32_t acc = bias;
#pragma unroll
            for (int c = 0; c < Cw; ++c) acc += l32[(s + S * c) * 1024 + o];
            const int slot = s * kWaveSlots + o;
            if (slot < valid) atomicAdd(out + base + slot, acc);
        }
    }
}

// --------------------------------------------------------------- main kernel
// One workgroup = one Item.  Wave w works on sub-tile s = w % S with chunk
// c = w / S of the item's rows and seeds (Cw = 16 / S chunks).
//   BL      rows are loaded in block layout (lane t: slots 16t..16t+15), the
//           layout the ChaCha blocks come out in; else coalesced layout.
//   MERGED  every item writes one tile (same-tile, rows-only or mask-only), so
//           rows are added straight into the mask accumulator (needs BL): one
//           16-register accumulator instead of two, no transpose.
//   WPE     minimum waves per SIMD requested from the register allocator.
template <int S, bool BL, bool MERGED, int WPE, int RUM = 2, int AUX = 0, bool SPREAD = false>
__global__ __launch_bounds__(kThreads, WPE) void items_kernel(const Item *__restrict__ items,
                                                              const uint32_t *__restrict__ rows,
                                                              uint64_t row_pitch,
                                                              const SeedRec *__restrict__ recs,
                                                              const uint32_t *__restrict__ meta,
                                                              uint32_t *__restrict__ out) {
    static_assert(!MERGED || BL, "merged accumulation needs block-layout rows");
    constexpr int Cw = kWavesPerGroup / S;
    constexpr int RU = MERGED ? RUM : 4;  // rows in flight per wave in the rows-only loop
    __shared__ u32x4 lds[kWavesPerGroup * 256];  // 64 KiB: one 4 KiB region per wave
    __shared__ uint32_t claim[S];                 // next unclaimed unit of each sub-tile

    const Item it = items[blockIdx.x];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = w % S, c = w / S;
    if constexpr (!SPREAD && Cw > 1) {
        if (threadIdx.x < S) claim[threadIdx.x] = 0u;
        __syncthreads();
    }
    const uint32_t flags = it.flags;
    const bool has_rows = flags & kHasRows, has_mask = flags & kHasMask;

    u32x4 racc[4] = {u32x4(0u), u32x4(0u), u32x4(0u), u32x4(0u)};  // unused when MERGED
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = 0;

    // this wave's share of rows and seeds
    uint32_t nr = 0, ns = 0, r0 = 0, q0 = 0;
    if (has_rows) {
        r0 = (uint32_t)(((uint64_t)it.nrows * c) / Cw);
        nr = (uint32_t)(((uint64_t)it.nrows * (c + 1)) / Cw) - r0;
    }
    if (has_mask) {
        q0 = it.k0 + (uint32_t)(((uint64_t)it.nseeds * c) / Cw);
        ns = it.k0 + (uint32_t)(((uint64_t)it.nseeds * (c + 1)) / Cw) - q0;
    }
    const int sub_slot = s * kWaveSlots;
    const int row_valid = (int)it.row_valid - sub_slot;   // may be <= 0: nothing valid
    // bytes of this sub-tile a row load may touch: whole quads up to the last valid slot
    const uint32_t row_bytes =
        row_valid >= kWaveSlots ? 4u * kWaveSlots : (row_valid > 0 ? 16u * (uint32_t)((row_valid + 3) / 4) : 0u);
    const uint32_t *rp = rows + it.row_in + (uint64_t)r0 * row_pitch + sub_slot;
    const uint32_t ctr = (uint32_t)(it.mask_ctr + (uint64_t)(sub_slot / 16) + (uint64_t)lane);
    const SeedRec *rec = recs + q0;
    if (row_valid <= 0) nr = 0;

    auto add_row = [&](const u32x4 (&v)[4]) {
        if constexpr (MERGED) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[4 * j + 0] += v[j].x; m[4 * j + 1] += v[j].y; m[4 * j + 2] += v[j].z; m[4 * j + 3] += v[j].w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) racc[j] = racc[j] + v[j];
        }
    };

    if constexpr (SPREAD) {
        // seeds spread evenly over the row stream (Bresenham): every row load is
        // issued before the ChaCha block that hides it, and seed-light items keep
        // HBM busy from the first row instead of front-loading the VALU work
        uint32_t q = 0;
        for (uint32_t r = 0; r < nr; ++r) {
            u32x4 v[4];
            load_row<BL, AUX>(rp, row_bytes, lane, v);
            if (q < ns && (uint64_t)q * nr <= (uint64_t)r * ns) {
                chacha_mask_add(rec, ctr, m);
                ++rec;
                ++q;
            }
            add_row(v);
            rp += row_pitch;
        }
        for (; q < ns; ++q) {
            chacha_mask_add(rec, ctr, m);
            ++rec;
        }
    } else if constexpr (Cw > 1) {
        // Units claimed from a per-sub-tile LDS counter: unit i = seed i of the item, plus row i
        // when there is one.  With a static split (64 seeds per wave at c4) the SIMD's arbiter
        // lets some waves run far ahead, and a workgroup waited at its barrier for its slowest
        // wave: 0.33-0.62 ms workgroup times, wave 0 idle ~0.2 ms of them, 87 % mean residency
        // (tools/probes/wg_trace.py, profiles/r02_wg_trace.log).  Claiming, a fast wave takes more
        // units and the waves of a workgroup finish within about one block of each other.
        // Any split gives the same bits: the partials are summed mod 2^32.
        const uint32_t NR = (has_rows && row_valid > 0) ? it.nrows : 0u;
        const uint32_t NS = has_mask ? it.nseeds : 0u;
        const uint32_t *rb = rows + it.row_in + sub_slot;
        // one lane adds 1 to the counter; in asm so that the compiler's atomic optimizer does not
        // wrap it in a wave reduction (mbcnt/bcnt/readfirstlane: ~8 VALU per unit)
        const uint32_t caddr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&claim[s];
        auto next = [&]() -> uint32_t {
            uint32_t v = 0;
            if (lane == 0)
                asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(caddr), "v"(1u) : "memory");
            return __builtin_amdgcn_readlane(v, 0);
        };
        // two loops, one body each: a single loop with a row / no-row branch made the compiler
        // copy the 16 accumulators at every unit
        const uint32_t NP = NR < NS ? NR : NS;
        uint32_t i = next();
        for (; i < NP; i = next()) {
            u32x4 v4[4];
            load_row<BL, AUX>(rb + (uint64_t)i * row_pitch, row_bytes, lane, v4);
            chacha_mask_add(recs + it.k0 + i, ctr, m);
            add_row(v4);
        }
        for (; i < NS; i = next()) chacha_mask_add(recs + it.k0 + i, ctr, m);
        // rows past the last seed (seed-light items): the static split, RU rows in flight
        if (NR > NS) {
            const uint32_t a = NS + (uint32_t)(((uint64_t)(NR - NS) * c) / Cw);
            const uint32_t b = NS + (uint32_t)(((uint64_t)(NR - NS) * (c + 1)) / Cw);
            const uint32_t *rq = rb + (uint64_t)a * row_pitch;
            uint32_t rr = b - a;
            for (; rr >= RU; rr -= RU) {
                u32x4 v4[RU][4];
#pragma unroll
                for (int u = 0; u < RU; ++u) load_row<BL, AUX>(rq + u * row_pitch, row_bytes, lane, v4[u]);
#pragma unroll
                for (int u = 0; u < RU; ++u) add_row(v4[u]);
                rq += RU * row_pitch;
            }
            for (; rr > 0; --rr) {
                u32x4 v4[4];
                load_row<BL, AUX>(rq, row_bytes, lane, v4);
                add_row(v4);
                rq += row_pitch;
            }
        }
    } else {
        // paired phase: one row load in flight under one ChaCha block per step
        const uint32_t np = nr < ns ? nr : ns;
        for (uint32_t q = 0; q < np; ++q) {
            u32x4 v[4];
            load_row<BL, AUX>(rp, row_bytes, lane, v);
            chacha_mask_add(rec, ctr, m);
            add_row(v);
            rp += row_pitch;
            ++rec;
        }
        // remaining rows: RU rows (RU x 4 KiB per wave) in flight
        uint32_t rr = nr - np;
        for (; rr >= RU; rr -= RU) {
            u32x4 v[RU][4];
#pragma unroll
            for (int u = 0; u < RU; ++u) load_row<BL, AUX>(rp + u * row_pitch, row_bytes, lane, v[u]);
#pragma unroll
            for (int u = 0; u < RU; ++u) add_row(v[u]);
            rp += RU * row_pitch;
        }
        for (; rr > 0; --rr) {
            u32x4 v[4];
            load_row<BL, AUX>(rp, row_bytes, lane, v);
            add_row(v);
            rp += row_pitch;
        }
        // remaining seeds
        for (uint32_t q = np; q < ns; ++q) {
            chacha_mask_add(rec, ctr, m);
            ++rec;
        }
    }

    // ---- combine through this wave's LDS region (natural slot order), then
    // sum the Cw chunk partials of every sub-tile and write the tile.
    u32x4 *R = lds + w * 256;
    const uint32_t mbias = it.mask_bias + ((flags & kMaskBiasNneg) ? meta_nneg(meta) : 0u);
    if constexpr (MERGED) {
        R[4 * lane + 0] = u32x4{m[0], m[1], m[2], m[3]};
        R[4 * lane + 1] = u32x4{m[4], m[5], m[6], m[7]};
        R[4 * lane + 2] = u32x4{m[8], m[9], m[10], m[11]};
        R[4 * lane + 3] = u32x4{m[12], m[13], m[14], m[15]};
        __syncthreads();
        const uint64_t base = has_mask ? it.mask_out : it.row_out;
        const int valid = has_mask ? (int)it.mask_valid : (int)it.row_valid;
        const uint32_t bias = (has_rows ? it.row_bias : 0u) + (has_mask ? mbias : 0u);
        reduce_out<S>(lds, out, base, valid, bias, (flags & (kRowAtomic | kMaskAtomic)) != 0);
    } else {
        const bool same = flags & kSameTile;
        u32x4 mq[4];
        if (has_mask) {
            if (BL) {
                mq[0] = u32x4{m[0], m[1], m[2], m[3]};
                mq[1] = u32x4{m[4], m[5], m[6], m[7]};
                mq[2] = u32x4{m[8], m[9], m[10], m[11]};
                mq[3] = u32x4{m[12], m[13], m[14], m[15]};
            } else {  // block layout -> coalesced layout
                R[4 * lane + 0] = u32x4{m[0], m[1], m[2], m[3]};
                R[4 * lane + 1] = u32x4{m[4], m[5], m[6], m[7]};
                R[4 * lane + 2] = u32x4{m[8], m[9], m[10], m[11]};
                R[4 * lane + 3] = u32x4{m[12], m[13], m[14], m[15]};
                __syncthreads();
#pragma unroll
                for (int j = 0; j < 4; ++j) mq[j] = R[lane + 64 * j];
            }
            if (same) {
#pragma unroll
                for (int j = 0; j < 4; ++j) racc[j] = racc[j] + mq[j];
            }
        }
        // LDS quad index of accumulator quad j of this lane (natural slot order)
#define FLM_RQ(j) (BL ? 4 * lane + (j) : lane + 64 * (j))
        if (has_rows || same) {
#pragma unroll
            for (int j = 0; j < 4; ++j) R[FLM_RQ(j)] = racc[j];
            __syncthreads();
            const uint64_t base = same ? it.mask_out : it.row_out;
            const int valid = same ? (int)it.mask_valid : (int)it.row_valid;
            const uint32_t bias = it.row_bias + (same ? mbias : 0u);
            const bool atom = same ? ((flags & (kRowAtomic | kMaskAtomic)) != 0) : ((flags & kRowAtomic) != 0);
            reduce_out<S>(lds, out, base, valid, bias, atom);
        }
        if (has_mask && !same) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) R[FLM_RQ(j)] = mq[j];
            __syncthreads();
            reduce_out<S>(lds, out, it.mask_out, (int)it.mask_valid, mbias, (flags & kMaskAtomic) != 0);
        }
#undef FLM_RQ
    }
}

// ------------------------------------------------------- small-round kernel
// The whole round in ONE launch for rounds too small to fill the chip through items_kernel
// (BASELINE c2: N=128 rows, K=128 seeds, L=16384).  There, items_kernel's 1024-thread
// workgroups land on half the CUs, and the seed-schedule launch before it adds its own gap
// (13 us per round measured; ~3 us of ChaCha work).  Here a 256-thread workgroup owns
// T = 16*B output slots outright.  It sums every row over them and adds every seed's mask,
// then stores the tile once: no atomics, no zero-fill, no seed table.
//   lane (b, sl) of wave w: ChaCha block b of the tile for seed s = pass*4*(64/B) + w*(64/B) + sl,
//   keys read straight from the raw 32-byte seeds (no SeedRec precompute: its saving is ~5 %
//   of a block and would cost the extra launch).
//   Rows: thread (quad q, group rg) sums rows rg, rg + RG, ... of quad q with 16-B loads,
//   issued before the ChaCha work so HBM latency hides under it.
//   Combine: lane accumulators and row partials through LDS, 16 entries per thread, then
//   one store per slot.
// Block 0 also writes the sign counts to meta (meta[0] = 1 part) as seed_schedule_kernel does,
// so flm_check_signs keeps working.
// SEG (client masking, SA_ClientAgent.py:304-324): blockIdx.y is output row i; its seeds are
// [seg[i], seg[i+1]), its input is row i of `rows` (none: the all-ones input, `bias` = 1), and
// the row is written at out + i*pitch.  No sign counts (the host validated the signs).
template <int B, bool SEG = false>
__global__ __launch_bounds__(256) void small_round_kernel(const uint32_t *__restrict__ rows, uint64_t pitch, int N,
                                                          const uint8_t *__restrict__ seeds,
                                                          const int8_t *__restrict__ signs, int K, uint64_t L,
                                                          uint64_t mask_lo, uint64_t mask_hi, uint32_t ctr0,
                                                          uint32_t *__restrict__ out, uint32_t *__restrict__ meta,
                                                          const int64_t *__restrict__ seg = nullptr,
                                                          uint32_t bias = 0u) {
    constexpr int T = 16 * B;     // slots per workgroup
    constexpr int SPW = 64 / B;   // seeds per wave per pass
    constexpr int SPP = 4 * SPW;  // seeds per pass
    constexpr int Q = T / 4;      // 16-B quads per row tile
    constexpr int RG = 256 / Q;   // row groups
    constexpr int G = 256 / T;    // slot groups of the combine
    constexpr int RB = 4;         // rows per thread in flight under the ChaCha work
    __shared__ __attribute__((aligned(16))) uint32_t lm[256 * 16];  // lane accumulators, 16 KiB
    __shared__ __attribute__((aligned(16))) uint32_t lr[RG * T];    // row partials
    __shared__ uint32_t lp[G * T];                                  // per-group slot partials (256 words)

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t slot0 = (uint64_t)blockIdx.x * T;
    int k_lo = 0, k_hi = K;
    if constexpr (SEG) {
        const uint64_t y = blockIdx.y;
        k_lo = (int)seg[y];
        k_hi = (int)seg[y + 1];
        N = rows ? 1 : 0;
        if (rows) rows += y * pitch;
        out += y * pitch;
    }

    // ---- rows: the first RB of this thread's rows are loaded before the masks
    const int q = tid % Q, rg = tid / Q;
    const uint64_t qslot = slot0 + 4 * (uint64_t)q;
    const bool qok = qslot < L;  // a quad straddling L stays inside the row (pitch >= round_up(L, 4))
    const uint32_t *rq = rows + qslot;
    u32x4 racc = u32x4(0u), rv[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
        const int r = rg + u * RG;
        rv[u] = (qok && r < N) ? *reinterpret_cast<const u32x4 *>(rq + (uint64_t)r * pitch) : u32x4(0u);
    }

    // ---- masks: one ChaCha block per lane per pass
    uint32_t acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
    uint32_t nneg = 0;
    const int b = lane % B, sl = lane / B;
    const uint64_t bslot = slot0 + 16 * (uint64_t)b;
    if (bslot >= mask_lo && bslot < mask_hi) {
        const uint32_t ctr = ctr0 + (uint32_t)(bslot / 16);
        const bool al16 = ((uintptr_t)seeds & 15) == 0;
        for (int s = k_lo + w * SPW + sl; s < k_hi; s += SPP) {
            const uint8_t *p = seeds + 32 * (size_t)s;
            uint32_t k[8];
            if (al16) {
                const uint4 a0 = reinterpret_cast<const uint4 *>(p)[0], a1 = reinterpret_cast<const uint4 *>(p)[1];
                k[0] = a0.x; k[1] = a0.y; k[2] = a0.z; k[3] = a0.w;
                k[4] = a1.x; k[5] = a1.y; k[6] = a1.z; k[7] = a1.w;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    k[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
                           ((uint32_t)p[4 * i + 3] << 24);
            }
            const bool neg = signs[s] < 0;
            const uint32_t xc = neg ? ~kAbcd : kAbcd;  // -(ks ^ C) = (ks ^ ~C) + 1
            nneg += neg ? 1u : 0u;
            uint32_t x0 = kSigma0, x1 = kSigma1, x2 = kSigma2, x3 = kSigma3;
            uint32_t x4 = k[0], x5 = k[1], x6 = k[2], x7 = k[3], x8 = k[4], x9 = k[5], x10 = k[6], x11 = k[7];
            uint32_t x12 = ctr, x13 = 0u, x14 = 0u, x15 = 0u;
            if constexpr (SEG) {
                // client masking: throughput-bound, the tuned lockstep rounds (FLM_QR4)
#pragma unroll
                for (int r = 0; r < 10; ++r) {
                    FLM_QR4(x0, x4, x8, x12, x1, x5, x9, x13, x2, x6, x10, x14, x3, x7, x11, x15);
                    FLM_QR4(x0, x5, x10, x15, x1, x6, x11, x12, x2, x7, x8, x13, x3, x4, x9, x14);
                }
            } else {
                // a small round (c2) is one block per lane on a latency path: the s_nop gaps of
                // FLM_QR4 only lengthen it (7.4 -> 9.4 us per c2 round), so the compiler's order
#pragma unroll
                for (int r = 0; r < 10; ++r) {
                    FLM_QR(x0, x4, x8, x12);
                    FLM_QR(x1, x5, x9, x13);
                    FLM_QR(x2, x6, x10, x14);
                    FLM_QR(x3, x7, x11, x15);
                    FLM_QR(x0, x5, x10, x15);
                    FLM_QR(x1, x6, x11, x12);
                    FLM_QR(x2, x7, x8, x13);
                    FLM_QR(x3, x4, x9, x14);
                }
            }
            acc[0] += (x0 + kSigma0) ^ xc;
            acc[1] += (x1 + kSigma1) ^ xc;
            acc[2] += (x2 + kSigma2) ^ xc;
            acc[3] += (x3 + kSigma3) ^ xc;
            acc[4] += (x4 + k[0]) ^ xc;
            acc[5] += (x5 + k[1]) ^ xc;
            acc[6] += (x6 + k[2]) ^ xc;
            acc[7] += (x7 + k[3]) ^ xc;
            acc[8] += (x8 + k[4]) ^ xc;
            acc[9] += (x9 + k[5]) ^ xc;
            acc[10] += (x10 + k[6]) ^ xc;
            acc[11] += (x11 + k[7]) ^ xc;
            acc[12] += (x12 + ctr) ^ xc;
            acc[13] += x13 ^ xc;
            acc[14] += x14 ^ xc;
            acc[15] += x15 ^ xc;
        }
    }

    // ---- rows: add the first batch, stream the rest
#pragma unroll
    for (int u = 0; u < RB; ++u) racc = racc + rv[u];
    if (qok)
        for (int r = rg + RB * RG; r < N; r += RG) racc = racc + *reinterpret_cast<const u32x4 *>(rq + (uint64_t)r * pitch);

    // ---- combine
    u32x4 *lm4 = reinterpret_cast<u32x4 *>(lm) + 4 * tid;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        lm4[j] = u32x4{acc[4 * j] + nneg, acc[4 * j + 1] + nneg, acc[4 * j + 2] + nneg, acc[4 * j + 3] + nneg};
    *reinterpret_cast<u32x4 *>(lr + rg * T + 4 * q) = racc;
    __syncthreads();
    {
        const int j = tid % T, g = tid / T;
        const int jb = j / 16, jw = j % 16;
        uint32_t sum = 0;
#pragma unroll
        for (int e = g * 16; e < g * 16 + 16; ++e) {  // 16 of the 256/B (wave, seed-lane) entries of slot j
            const int wv = e / SPW, sle = e % SPW;
            sum += lm[(wv * 64 + sle * B + jb) * 16 + jw];
        }
#pragma unroll
        for (int r = g; r < RG; r += G) sum += lr[r * T + j];
        lp[g * T + j] = sum;
    }
    __syncthreads();
    if (tid < T) {
        uint32_t total = bias;
#pragma unroll
        for (int g = 0; g < G; ++g) total += lp[g * T + tid];
        if (slot0 + tid < L) out[slot0 + tid] = total;
    }

    // ---- sign counts (block 0), the same meta layout as seed_schedule_kernel with one part
    if (!SEG && blockIdx.x == 0) {
        uint32_t n = 0, bad = 0;
        for (int s = tid; s < K; s += 256) {
            const int sg = signs[s];
            n += sg < 0 ? 1u : 0u;
            bad += (sg != 1 && sg != -1) ? 1u : 0u;
        }
        __syncthreads();  // lp is free again
        lp[tid] = n;
        lm[tid] = bad;
        __syncthreads();
        if (tid == 0) {
            uint32_t tn = 0, tb = 0;
            for (int i = 0; i < 256; ++i) { tn += lp[i]; tb += lm[i]; }
            meta[0] = 1u;
            meta[2] = tn;
            meta[3] = tb;
        }
    }
}

// --------------------------------------------------- byte keystream (host PRF)
// out = in ^ ChaCha20(key, nonce) from block `counter`, one block per thread.
__global__ __launch_bounds__(256) void chacha20_xor_kernel(uint32_t k0, uint32_t k1, uint32_t k2,
                                                           uint32_t k3, uint32_t k4, uint32_t k5,
                                                           uint32_t k6, uint32_t k7, uint32_t n0,
                                                           uint32_t n1, uint64_t counter,
                                                           const uint8_t *__restrict__ in,
                                                           uint8_t *__restrict__ out, uint64_t n) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t off = b * 64;
    if (off >= n) return;
    const uint64_t blk = counter + b;
    uint32_t x0 = kSigma0, x1 = kSigma1, x2 = kSigma2, x3 = kSigma3;
    uint32_t x4 = k0, x5 = k1, x6 = k2, x7 = k3, x8 = k4, x9 = k5, x10 = k6, x11 = k7;
    uint32_t x12 = (uint32_t)blk, x13 = (uint32_t)(blk >> 32), x14 = n0, x15 = n1;
    const uint32_t i12 = x12, i13 = x13;
    for (int r = 0; r < 10; ++r) {
        FLM_QR4(x0, x4, x8, x12, x1, x5, x9, x13, x2, x6, x10, x14, x3, x7, x11, x15);
        FLM_QR4(x0, x5, x10, x15, x1, x6, x11, x12, x2, x7, x8, x13, x3, x4, x9, x14);
    }
    const uint32_t ks[16] = {x0 + kSigma0, x1 + kSigma1, x2 + kSigma2, x3 + kSigma3,
                             x4 + k0,      x5 + k1,      x6 + k2,      x7 + k3,
                             x8 + k4,      x9 + k5,      x10 + k6,     x11 + k7,
                             x12 + i12,    x13 + i13,    x14 + n0,     x15 + n1};
    const uint64_t m = (n - off) < 64 ? (n - off) : 64;
    for (uint64_t i = 0; i < m; ++i) out[off + i] = in[off + i] ^ (uint8_t)(ks[i >> 2] >> (8 * (i & 3)));
}

// ------------------------------------------------------- pair-mask work queue
// The dropout-pair masks of the CU-split reconstruction (reconstruct.py, pair_queue=True;
// SA_ServiceAgent.py:587-603) cut into units of (1024-slot tile, kUnitSeeds seeds), claimed
// from a counter so that two launches on different CU sets share them without a fixed split:
//   SIDE  (the EC CUs, once the combine is done): claims units until ws[1] (set on the
//         self-mask stream by flag_set_kernel when that pass ends) reads non-zero;
//   FINAL (all CUs, after both streams): claims the rest.
// A claimed unit is always finished, so every unit is added exactly once whatever the timing:
// the flag only moves the split.  No wave ever waits on the flag (it is read between units),
// so both grids drain on their own.  One wave per workgroup: the LDS transpose needs only a
// wave-local barrier, and waves that stop at different units never wait for each other.
// Units are chunk-major (consecutive claims hit different tiles); each lane makes ChaCha
// block `tile*64 + lane`, the 16 words go through LDS so that every u32 atomic add of the
// wave covers 64 consecutive slots.
constexpr int kUnitSeeds = 16;  // 32 and 64 measured the same at c5 (profiles/r02_ab_pair_units.log)

template <bool SIDE>
__global__ __launch_bounds__(64) void pair_units_kernel(const SeedRec *__restrict__ recs, int K,
                                                        uint32_t *__restrict__ dst, uint64_t L,
                                                        uint32_t n_tiles, uint32_t n_units,
                                                        uint32_t *__restrict__ ws) {
    __shared__ uint32_t lds[64 * 17];
    const int lane = threadIdx.x;
    for (;;) {
        uint32_t u = 0;
        if (lane == 0) {
            u = n_units;  // "stop"
            if (!SIDE || __hip_atomic_load(&ws[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
                u = __hip_atomic_fetch_add(&ws[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        u = __builtin_amdgcn_readfirstlane(__shfl(u, 0));
        if (u >= n_units) break;
        const uint32_t tile = u % n_tiles, chunk = u / n_tiles;
        const int k0 = (int)chunk * kUnitSeeds;
        const int k1 = min(K, k0 + kUnitSeeds);
        uint32_t m[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = 0u;
        uint32_t nneg = 0;
        const uint32_t ctr = tile * 64u + (uint32_t)lane;
        for (int k = k0; k < k1; ++k) {
            chacha_mask_add(&recs[k], ctr, m);
            nneg += (recs[k].xorc != kAbcd);
        }
        __syncthreads();  // the previous unit's reads of lds are done
#pragma unroll
        for (int i = 0; i < 16; ++i) lds[lane * 17 + i] = m[i] + nneg;
        __syncthreads();
        // one address per lane, the 16 stores at immediate offsets j * 256 B; the tile's valid
        // slot count bounds them (full tiles: all 1024)
        const uint64_t base = (uint64_t)tile * 1024u;
        const uint32_t valid = (uint32_t)min<uint64_t>(1024u, L - base);
        // slot e = j*64 + lane sits at lds[(e >> 4) * 17 + (e & 15)] = lds[lb + 68 j]
        uint32_t *p = dst + base + lane;
        const uint32_t lb = (uint32_t)(lane >> 4) * 17u + (uint32_t)(lane & 15);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((uint32_t)(j * 64 + lane) < valid)
                __hip_atomic_fetch_add(p + j * 64, lds[lb + 68 * j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ws[1] = 1 once every earlier launch on this stream has finished (release, device scope).
__global__ void flag_set_kernel(uint32_t *__restrict__ ws) {
    if (threadIdx.x == 0) __hip_atomic_store(&ws[1], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- mask expansion
// Standalone PRG expansion (north_star (i); the cancel_vec idiom of SA_ServiceAgent.py:596-603 and
// SA_ClientAgent.py:248-250 for a whole batch of seeds): out[k * pitch + l] = PRG(seed k)[slot0 + l]
// for l < L.  A unit is (seed k, 1024-slot chunk), numbered seed-major; one-wave workgroup g takes
// the contiguous run of units [g U / G, (g + 1) U / G), so it loads a seed's SeedRec once (scalar
// registers) for all of that seed's chunks in its run and writes consecutive 4 KiB of its row.
// Lane t makes ChaCha block ctr0 + 64 chunk + t (slots 16t..16t+15 of the chunk); the 16 words
// go through the wave's 4 KiB of LDS and come back in coalesced order, so each 16-B store
// instruction writes 1 KiB contiguous (lane t: slot 4t + 256j).  Measured against storing each
// lane's own 64 B (four 16-B stores at a 64-B lane stride): 1.45 vs 1.53 ms at K = 962, L = 2^20,
// and nontemporal forms the same (LDS-staged) or 4.5x slower (lane-strided partial lines;
// profiles/r06_expand_probe.log).  ~36 VGPRs: the grid is sized for occupancy (flm_set_tuning
// "expand_waves"), not for the unit count.
__global__ __launch_bounds__(64) void prg_expand_kernel(const SeedRec *__restrict__ recs, uint32_t chunks,
                                                        uint32_t n_units, uint64_t L, uint64_t pitch, uint32_t ctr0,
                                                        uint32_t *__restrict__ out) {
    __shared__ u32x4 lds[256];
    const int lane = threadIdx.x;
    const uint32_t u0 = (uint32_t)(((uint64_t)n_units * blockIdx.x) / gridDim.x);
    const uint32_t u1 = (uint32_t)(((uint64_t)n_units * (blockIdx.x + 1)) / gridDim.x);
    for (uint32_t u = u0; u < u1;) {
        const uint32_t k = u / chunks;
        const uint32_t end = min(u1, (k + 1) * chunks);
        const SeedRec rec = recs[k];  // wave-uniform: scalar loads, once per seed of the run
        uint32_t *row = out + (uint64_t)k * pitch;
        for (uint32_t chunk = u - k * chunks; u < end; ++u, ++chunk) {
            uint32_t m[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) m[i] = 0u;
            chacha_mask_add(&rec, ctr0 + chunk * 64u + (uint32_t)lane, m);
            const int valid = (int)min<uint64_t>(1024u, L - (uint64_t)chunk * 1024u);
            uint32_t *dst = row + (uint64_t)chunk * 1024u;
            __syncthreads();  // one wave per workgroup: the previous chunk's reads are done
#pragma unroll
            for (int j = 0; j < 4; ++j) lds[4 * lane + j] = u32x4{m[4 * j], m[4 * j + 1], m[4 * j + 2], m[4 * j + 3]};
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int slot = 4 * (lane + 64 * j);
                const u32x4 v = lds[lane + 64 * j];
                if (slot + 4 <= valid) {
                    *reinterpret_cast<u32x4 *>(dst + slot) = v;
                } else {
                    if (slot + 0 < valid) dst[slot + 0] = v.x;
                    if (slot + 1 < valid) dst[slot + 1] = v.y;
                    if (slot + 2 < valid) dst[slot + 2] = v.z;
                }
            }
        }
    }
}

// dst = a + b (mod 2^32), 16-B accesses, grid-stride.
__global__ __launch_bounds__(256) void add2_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                   uint32_t *__restrict__ dst, uint64_t n) {
    const uint64_t quads = n / 4, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t q = t0; q < quads; q += stride) {
        const uint4 x = reinterpret_cast<const uint4 *>(a)[q], y = reinterpret_cast<const uint4 *>(b)[q];
        reinterpret_cast<uint4 *>(dst)[q] = make_uint4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
    }
    const uint64_t t = 4 * quads + t0;
    if (t < n) dst[t] = a[t] + b[t];
}

// Loopback exchange of a device group whose ranks share one GPU (flm_group with repeated
// devices; tests and rehearsal only -- distinct GPUs use RCCL's reduce-scatter):
// dst[l] = sum_g parts.p[g][lo + l] for l < n, mod 2^32.  HBM-bound, uint4 when aligned.
__global__ __launch_bounds__(256) void shard_sum_kernel(PartPtrs parts, int G, uint64_t lo, uint64_t n,
                                                        uint32_t *__restrict__ dst) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((lo & 3) == 0) {
        const uint64_t quads = n / 4;
        for (uint64_t q = t0; q < quads; q += stride) {
            uint4 acc = make_uint4(0, 0, 0, 0);
            for (int g = 0; g < G; ++g) {
                const uint4 v = reinterpret_cast<const uint4 *>(parts.p[g] + lo)[q];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
            reinterpret_cast<uint4 *>(dst)[q] = acc;
        }
        for (uint64_t t = 4 * quads + t0; t < n; t += stride) {
            uint32_t a = 0;
            for (int g = 0; g < G; ++g) a += parts.p[g][lo + t];
            dst[t] = a;
        }
        return;
    }
    for (uint64_t t = t0; t < n; t += stride) {
        uint32_t a = 0;
        for (int g = 0; g < G; ++g) a += parts.p[g][lo + t];
        dst[t] = a;
    }
}

// ------------------------------------------------------------ fixed-point codec
// Float updates in, float mean out (the "replace it with model weights" of SA_ClientAgent.py:300-304).
// The codec's one definition is in DESIGN.md section 5 and, restated in numpy, tests/codec_cases.py:
//   encode: NaN -> 0, clip to [-c, c], t = x 2^f (exact), nearest-even or stochastic rounding, two's complement
//   decode: float32(float64(int32(s)) / (count 2^f))

// m[i] += ChaCha20_block(key at p, ctr)[i] ^ xc from the raw 32 key bytes (wave-uniform: scalar loads), as
// small_round_kernel's SEG mode does: no SeedRec table, so the call is one launch and touches no table ring.
__device__ __forceinline__ void chacha_raw_add(const uint8_t *__restrict__ p, uint32_t ctr, uint32_t xc,
                                               uint32_t (&m)[16]) {
    uint32_t k[8];
    if (((uintptr_t)p & 15) == 0) {
        const uint4 a0 = reinterpret_cast<const uint4 *>(p)[0], a1 = reinterpret_cast<const uint4 *>(p)[1];
        k[0] = a0.x; k[1] = a0.y; k[2] = a0.z; k[3] = a0.w;
        k[4] = a1.x; k[5] = a1.y; k[6] = a1.z; k[7] = a1.w;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            k[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
                   ((uint32_t)p[4 * i + 3] << 24);
    }
    uint32_t x0 = kSigma0, x1 = kSigma1, x2 = kSigma2, x3 = kSigma3;
    uint32_t x4 = k[0], x5 = k[1], x6 = k[2], x7 = k[3], x8 = k[4], x9 = k[5], x10 = k[6], x11 = k[7];
    uint32_t x12 = ctr, x13 = 0u, x14 = 0u, x15 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        FLM_QR4(x0, x4, x8, x12, x1, x5, x9, x13, x2, x6, x10, x14, x3, x7, x11, x15);
        FLM_QR4(x0, x5, x10, x15, x1, x6, x11, x12, x2, x7, x8, x13, x3, x4, x9, x14);
    }
    m[0] += (x0 + kSigma0) ^ xc;
    m[1] += (x1 + kSigma1) ^ xc;
    m[2] += (x2 + kSigma2) ^ xc;
    m[3] += (x3 + kSigma3) ^ xc;
    m[4] += (x4 + k[0]) ^ xc;
    m[5] += (x5 + k[1]) ^ xc;
    m[6] += (x6 + k[2]) ^ xc;
    m[7] += (x7 + k[3]) ^ xc;
    m[8] += (x8 + k[4]) ^ xc;
    m[9] += (x9 + k[5]) ^ xc;
    m[10] += (x10 + k[6]) ^ xc;
    m[11] += (x11 + k[7]) ^ xc;
    m[12] += (x12 + ctr) ^ xc;
    m[13] += x13 ^ xc;
    m[14] += x14 ^ xc;
    m[15] += x15 ^ xc;
}

// One element of the codec.  r: the dither word of this slot (stochastic rounding only).
template <bool STOCHASTIC>
__device__ __forceinline__ uint32_t codec_encode(float x, float clip, float scale, uint32_t r, uint32_t &nclip) {
#pragma clang fp contract(off)
    const bool nan = x != x;
    nclip += (nan || fabsf(x) > clip) ? 1u : 0u;
    x = nan ? 0.0f : x;
    const float t = fminf(fmaxf(x, -clip), clip) * scale;  // a power-of-two scale: exact
    if constexpr (!STOCHASTIC) {
        return (uint32_t)(int32_t)rintf(t);  // ties to even
    } else {
        const float ti = truncf(t), fr = fabsf(t - ti);           // fr exact: its bits are a subset of t's
        const uint32_t thr = (uint32_t)(fr * 4294967296.0f);      // < 2^32: fr <= 1 - 2^-24
        int32_t q = (int32_t)ti;
        if (r < thr) q += t < 0.0f ? -1 : 1;
        return (uint32_t)q;
    }
}

// out[l] = float32(float64(int32(sum[l])) / denom), denom = count 2^f (SA_ServiceAgent.py:538-540, 605: the
// final sum, as a mean).  16-byte loads and stores; a thread reads its quad before it writes it, so out may be
// sum.  HBM-bound: the double division hides under the stream.
__global__ __launch_bounds__(256) void decode_sum_kernel(const uint32_t *sum, uint64_t n, double denom, float *out) {
    const uint64_t quads = n / 4, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t q = t0; q < quads; q += stride) {
        const uint4 s = reinterpret_cast<const uint4 *>(sum)[q];
        float4 v;
        v.x = (float)((double)(int32_t)s.x / denom);
        v.y = (float)((double)(int32_t)s.y / denom);
        v.z = (float)((double)(int32_t)s.z / denom);
        v.w = (float)((double)(int32_t)s.w / denom);
        reinterpret_cast<float4 *>(out)[q] = v;
    }
    const uint64_t t = 4 * quads + t0;
    if (t < n) out[t] = (float)((double)(int32_t)sum[t] / denom);
}

// ------------------------------------------------------------ packed fixed-point codec
// P = 2 or 4 parameters per ring word, in fields of W = 32 / P bits (tests/pack_cases.py):
//   field u = q + B, q the codec's encode, B = ceil(c 2^f); word l' = sum_j u[P l' + j] << (W j); fields of
//   parameters past L hold 0.  With n 2B <= 2^W - 1 no field of a sum over n clients carries into the next.
//   decode: s_j = (S >> W j) & (2^W - 1), out[P l' + j] = float32(float64(s_j - count B) / (count 2^f)).

// One field: the codec's q of a parameter the row has, biased; 0 for a parameter past L (whatever v holds).
template <bool STOCHASTIC>
__device__ __forceinline__ uint32_t codec_field(bool have, float v, float clip, float scale, uint32_t r, uint32_t bias,
                                                uint32_t &nclip) {
    const uint32_t q = codec_encode<STOCHASTIC>(have ? v : 0.0f, clip, scale, r, nclip);
    return have ? q + bias : 0u;
}

// ------------------------------------------------------------ distributed-DP noise inside the encode-mask kernels
// The binomial mechanism (tests/dp_cases.py): b = noise_bits fair coins per parameter and
// client, m = ceil(b / 32) draws, r = b mod 32.  Draw d of parameter l is word 16 (m (l / 16) + d) + l % 16 of
// PRG(noise_i), the last draw ANDed with 2^r - 1 when r != 0; Z[l] = sum_d popcount(draw d) - b / 2; q' = q + Z.
// Unpacked the ring word is uint32(q'); packed the field is q' + B + b / 2 = q + B + sum_d popcount(draw d).

// One noise block: ChaCha block `blk` of the client's noise stream holds one draw for the 16 parameters par..par + 15.
// Unpacked, their popcounts go straight into the accumulator; packed, P of them make a word of the wave's own LDS
// region (Q: the 4 / P quads of this parameter block), which no other wave and no other lane touches.
template <int P>
__device__ __forceinline__ void noise_block_add(const uint8_t *__restrict__ key, uint32_t blk, uint32_t draw_mask,
                                                uint64_t par, uint64_t L, uint32_t (&m)[16], u32x4 *Q) {
    uint32_t z[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) z[j] = 0u;
    chacha_raw_add(key, blk, kAbcd, z);
    if constexpr (P == 1) {
        // parameters past L are never stored, so their noise needs no predicate here
#pragma unroll
        for (int j = 0; j < 16; ++j) m[j] = __popc(z[j] & draw_mask) + m[j];  // one v_bcnt_u32_b32 each
    } else {
        constexpr int W = 32 / P;
        // a stored word's upper fields may lie past L: those parameters get no noise
        const uint32_t have = par < L ? (uint32_t)(L - par < 16 ? L - par : 16) : 0u;
        uint32_t e[16 / P];
#pragma unroll
        for (int q = 0; q < 16 / P; ++q) {
            e[q] = 0u;
#pragma unroll
            for (int jj = 0; jj < P; ++jj) {
                const int j = P * q + jj;
                e[q] += ((uint32_t)j < have ? (uint32_t)__popc(z[j] & draw_mask) : 0u) << (W * jj);
            }
        }
        if constexpr (P == 4) {
            Q[0] += u32x4{e[0], e[1], e[2], e[3]};
        } else {
            Q[0] += u32x4{e[0], e[1], e[2], e[3]};
            Q[1] += u32x4{e[4], e[5], e[6], e[7]};
        }
    }
}

// The discrete Gaussian mechanism's share, sampled from a cumulative table (tests/dgauss_cases.py):
// cdt[0 .. T - 1] uint64, non-decreasing, T = 2 tau; parameter l draws u = hi 2^32 + lo, hi word 16 (2 beta) + l % 16
// and lo word 16 (2 beta + 1) + l % 16 of PRG(noise_i), beta = l / 16; z = #{j < T : cdt[j] <= u} - tau; q' = q + z.
// Unpacked the ring word is uint32(q'); packed the field is q' + B + tau = q + B + the count.

// The count of table entries <= u: a bisection without a branch on data.  The trip count depends on T alone (wave-
// uniform, host-known).  Whatever the table holds, every index read is below T and the count is in [0, T]: base + len
// never grows, and the last probe is tab[base] with len = 1.  The compare is a 64-bit unsigned one.  G draws go
// through the loop together (hi[g .. g + G) become their counts), so that G LDS reads are in flight at a time.
template <int G>
__device__ __forceinline__ void cdt_counts(const uint64_t *tab, uint32_t T, uint32_t (&hi)[16], const uint32_t (&lo)[16],
                                           int g) {
    uint64_t u[G];
    uint32_t base[G];
#pragma unroll
    for (int j = 0; j < G; ++j) u[j] = ((uint64_t)hi[g + j] << 32) | lo[g + j], base[j] = 0u;
#pragma unroll 1
    for (uint32_t len = T; len > 1u;) {
        const uint32_t h = len >> 1;
#pragma unroll
        for (int j = 0; j < G; ++j) base[j] += tab[base[j] + h - 1u] <= u[j] ? h : 0u;
        len -= h;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) hi[g + j] = base[j] + (tab[base[j]] <= u[j] ? 1u : 0u);
}

// One noise unit of the table mode: ChaCha blocks 2 blk (high words) and 2 blk + 1 (low words) of the client's noise
// stream are the 16 draws of parameter block blk, at par..par + 15; their counts add as noise_block_add's popcounts do.
// The high words stay in registers across the second block.
template <int P>
__device__ __forceinline__ void gauss_block_add(const uint8_t *__restrict__ key, uint32_t blk, const uint64_t *tab,
                                                uint32_t T, uint64_t par, uint64_t L, uint32_t (&m)[16], u32x4 *Q) {
    uint32_t hi[16], lo[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) hi[j] = lo[j] = 0u;
    chacha_raw_add(key, 2u * blk, kAbcd, hi);
    chacha_raw_add(key, 2u * blk + 1u, kAbcd, lo);
#pragma unroll
    for (int g = 0; g < 16; g += 4) cdt_counts<4>(tab, T, hi, lo, g);
    if constexpr (P == 1) {
        // parameters past L are never stored, so their noise needs no predicate here
#pragma unroll
        for (int j = 0; j < 16; ++j) m[j] += hi[j];
    } else {
        constexpr int W = 32 / P;
        // a stored word's upper fields may lie past L: those parameters get no noise
        const uint32_t have = par < L ? (uint32_t)(L - par < 16 ? L - par : 16) : 0u;
        uint32_t e[16 / P];
#pragma unroll
        for (int q = 0; q < 16 / P; ++q) {
            e[q] = 0u;
#pragma unroll
            for (int jj = 0; jj < P; ++jj) {
                const int j = P * q + jj;
                e[q] += ((uint32_t)j < have ? hi[j] : 0u) << (W * jj);
            }
        }
        Q[0] += u32x4{e[0], e[1], e[2], e[3]};
        if constexpr (P == 2) Q[1] += u32x4{e[4], e[5], e[6], e[7]};
    }
}

// ------------------------------------------------------------ the encode-mask kernel
// The parts of encode_mask_kernel below that stand on their own.

// The dealing of a client's unit list (unit = one ChaCha block per lane) over the four waves, rank = 3 - wave: the
// encoding wave (rank 0) carries E blocks of its own, so the first 3 E units go round ranks 1..3 and the rest round
// all four from rank 0.  E = 1: unit u runs on rank (u + 1) % 4, a step of 4 throughout.
template <int E>
__device__ __forceinline__ int64_t first_unit(int rank) { return rank ? rank - 1 : 3 * E; }
template <int E>
__device__ __forceinline__ int64_t next_unit(int64_t u) { return u + (u + 3 < 3 * E ? 3 : 4); }

// Waves per SIMD pinned, floor and ceiling, to those of the kernel an instantiation replaced: the stochastic ones
// without noise (7 at P = 1, 6 packed).  Left alone the allocator took 81 VGPRs at P = 4, one past the step to 6
// waves, or at P = 1 aimed at 8 waves with 63 and ran slower.  0: left alone (1 to 8); those match unasked.
template <int P, bool STOCHASTIC, bool NOISE>
constexpr int kEncodeWaves = STOCHASTIC && !NOISE ? (P == 1 ? 7 : 6) : 0;

// clipped[i] (zeroed by the call) gets one atomic add per workgroup: only the encoding wave counts, so its
// total is the workgroup's
__device__ __forceinline__ void clipped_add(uint32_t *clipped, uint32_t i, uint32_t nclip, int lane) {
    if (!clipped) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nclip += __shfl_xor(nclip, off);
    if (lane == 0 && nclip) atomicAdd(clipped + i, nclip);
}

// The four waves' partials meet in LDS and the tile is stored once: R, the lane's 16 words of its wave's region,
// takes the accumulator (ADD: on top of the words already there), then thread p sums quad p of the REGIONS regions
// (the waves' four, and a fifth where the packed words have one) and stores it, 16 bytes a thread (1 KiB
// contiguous per wave), word by word across the row's end at Lw.
template <bool ADD, int REGIONS>
__device__ __forceinline__ void tile_meet_store(const u32x4 *lds, u32x4 *R, const uint32_t (&m)[16], uint32_t nneg,
                                                uint32_t *row, uint32_t tile, uint64_t Lw) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32x4 a = u32x4{m[4 * j] + nneg, m[4 * j + 1] + nneg, m[4 * j + 2] + nneg, m[4 * j + 3] + nneg};
        if constexpr (ADD) R[j] += a;
        else R[j] = a;
    }
    __syncthreads();
    const int p = threadIdx.x;
    u32x4 acc = lds[p] + lds[256 + p] + lds[512 + p] + lds[768 + p];
    if constexpr (REGIONS == 5) acc += lds[1024 + p];
    const uint64_t slot = (uint64_t)tile * 1024u + 4u * (uint64_t)p;
    uint32_t *dst = row + slot;
    if (slot + 3 < Lw) {
        *reinterpret_cast<u32x4 *>(dst) = acc;
    } else {
        if (slot + 0 < Lw) dst[0] = acc.x;
        if (slot + 1 < Lw) dst[1] = acc.y;
        if (slot + 2 < Lw) dst[2] = acc.z;
    }
}

// out[i][l'] = word l' of x[i] (encoded, packed P to a word, noised) + sum_{k in [seg[i], seg[i+1])} signs[k] PRG(seeds[k])[l']
// (SA_ClientAgent.py:300-324), over Lw = ceil(L / P) ring words a row.
// Workgroup g = (client i, 1024-word tile) = (g / tiles, g % tiles) of a one-dimensional grid; four waves.  Every
// wave's lane t owns ChaCha block t of the tile (words 16t..16t+15) and keeps a 16-word accumulator in registers.
// The units: a unit adds one ChaCha block per lane, and any wave can run it.  With NOISE the P draws noise units
// come first (unit u is draw u / P of parameter block u % P: block draws (P (64 tile + t) + d) + dd of the noise
// stream is draw dd of parameter block d of the lane's P), then the client's seeds; first_unit / next_unit deal the
// list.  The loop over the two kinds of unit is rolled (the seeds-only loop is left to the compiler, as it was) and
// its bound is host-known; nothing loops on data.
// The encoding: rank 0 reads the lane's 16 P consecutive floats, one parameter block (one dither block's worth: in
// stochastic mode block P (64 tile + t) + d of the client's dither stream, which is indexed by parameter) per pass,
// the passes not unrolled, so that the footprint stays that of one ChaCha block beside the accumulator.  That is
// E = P blocks of its own in stochastic mode and about one in nearest mode.  Parameters past L read as 0.0 (a
// predicate per element: the padding of a row may hold anything), encode to a zero field and are never counted as
// clipped or stored.  The pass is written in the kernel, not in a helper: behind a function boundary the same text
// took 83 to 96 VGPRs at P = 4 stochastic, here 77 to 81 (profiles/codec_unify_resources.txt).
// The meet: the four partials meet in LDS (one 4 KiB region per wave) and the tile is stored once.
// P = 1: everything adds into the accumulator registers; bias is 0, and with NOISE the encoding wave adds -b / 2
// once per parameter (`half`).  P > 1: packed words go to LDS, indexed dynamically by the parameter block, so that
// no pass indexes the accumulator registers.  With NOISE every wave has some (its noise units'): they and the
// encoding wave's add into the wave's own region, zeroed first, and the accumulator joins them at the meet; the
// bias is B: the +b / 2 of the field bias B_n and the -b / 2 of Z cancel, so the popcounts add as they are.  Without
// noise only the encoding wave has any and stores them to a fifth region (20 KiB), with no zeroing and no
// read-modify-write: with the own region there too, the packed legs without noise measured up to 1.1 % slower
// than the kernel they replace.
// NOISE = false: the unit list is the seeds alone; noise, draws, last_mask and half are not read; at P = 1 the
// encoding wave calls codec_encode itself.  No instantiation spills.
template <int P, bool STOCHASTIC, bool NOISE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kEncodeWaves<P, STOCHASTIC, NOISE> ? kEncodeWaves<P, STOCHASTIC, NOISE> : 1,
                                                                         kEncodeWaves<P, STOCHASTIC, NOISE> ? kEncodeWaves<P, STOCHASTIC, NOISE> : 8)))
void encode_mask_kernel(const float *__restrict__ x, uint64_t x_pitch,
                                                          const int64_t *__restrict__ seg,
                                                          const uint8_t *__restrict__ seeds,
                                                          const int8_t *__restrict__ signs,
                                                          const uint8_t *__restrict__ dither,
                                                          const uint8_t *__restrict__ noise, uint32_t draws,
                                                          uint32_t last_mask, uint32_t half, uint64_t L, uint64_t Lw,
                                                          uint32_t tiles, float clip, float scale, uint32_t bias,
                                                          uint32_t *__restrict__ out, uint64_t out_pitch,
                                                          uint32_t *__restrict__ clipped) {
    static_assert(P == 1 || P == 2 || P == 4, "one, two or four fields per word");
    constexpr int E = STOCHASTIC ? P : 1;
    constexpr bool OWN = P > 1 && NOISE;    // packed words add into the wave's own region ...
    constexpr bool FIFTH = P > 1 && !NOISE;  // ... or, only the encoding wave having any, are stored to a fifth
    __shared__ u32x4 lds[(FIFTH ? 5 : 4) * 256];  // one 4 KiB region per wave (16 KiB), and the fifth
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x / tiles, tile = blockIdx.x - i * tiles;
    const uint32_t ctr = tile * 64u + (uint32_t)lane;
    const uint64_t par0 = (uint64_t)P * ((uint64_t)tile * 1024u + 16u * (uint64_t)lane);  // the lane's first parameter
    const int64_t k_lo = seg[i];
    const int64_t n_noise = NOISE ? (int64_t)P * (int64_t)draws : 0, n_units = n_noise + (seg[i + 1] - k_lo);

    u32x4 *R = lds + w * 256 + 4 * lane;  // the lane's 16 words of its wave's partial
    if constexpr (OWN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) R[j] = u32x4{0u, 0u, 0u, 0u};
    }
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) m[j] = 0u;
    uint32_t nneg = 0;
    const int rank = 3 - w;
    // The seed's four lines stand in both loops: through a lambda or a helper the allocator gave the stochastic
    // instantiations 16 VGPRs fewer and they ran 1.5 to 2.4 % slower.
    if constexpr (NOISE) {  // two bodies in the loop: kept rolled
#pragma unroll 1
        for (int64_t u = first_unit<E>(rank); u < n_units; u = next_unit<E>(u)) {
            if (u < n_noise) {
                const uint32_t d = (uint32_t)u % (uint32_t)P, dd = (uint32_t)u / (uint32_t)P;
                // draws ceil(L / 16) <= 2^32 (the call's length rule): the counter of a parameter block the row has
                // stays below 2^32; a block past L may wrap, and is predicated away or never stored
                noise_block_add<P>(noise + 32 * (size_t)i, draws * ((uint32_t)P * ctr + d) + dd,
                                   dd + 1 == draws ? last_mask : 0xffffffffu, par0 + 16u * d, L, m, R + (4 / P) * d);
                continue;
            }
            const int64_t k = k_lo + (u - n_noise);
            const bool neg = signs[k] < 0;
            nneg += neg ? 1u : 0u;
            chacha_raw_add(seeds + 32 * (size_t)k, ctr, neg ? ~kAbcd : kAbcd, m);  // -(ks ^ C) = (ks ^ ~C) + 1
        }
    } else {
        for (int64_t u = first_unit<E>(rank); u < n_units; u = E == 1 ? u + 4 : next_unit<E>(u)) {  // E = 1: said outright
            const int64_t k = k_lo + u;
            const bool neg = signs[k] < 0;
            nneg += neg ? 1u : 0u;
            chacha_raw_add(seeds + 32 * (size_t)k, ctr, neg ? ~kAbcd : kAbcd, m);  // -(ks ^ C) = (ks ^ ~C) + 1
        }
    }
    if (rank == 0) {
        const float *xr = x + (uint64_t)i * x_pitch;
        uint32_t nclip = 0;
#pragma unroll 1
        for (int d = 0; d < P; ++d) {
            constexpr int W = 32 / P;
            uint32_t r[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) r[j] = 0u;
            // parameters below 2^36 (the call's range rule): the dither block counter stays below 2^32
            if constexpr (STOCHASTIC) chacha_raw_add(dither + 32 * (size_t)i, (uint32_t)P * ctr + (uint32_t)d, kAbcd, r);
            uint32_t e[16 / P];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint64_t s = par0 + 16u * (uint32_t)d + 4u * j;
                // a quad that straddles L stays inside the row (x_pitch >= round_up(L, 4))
                const float4 v = s < L ? *reinterpret_cast<const float4 *>(xr + s) : make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (P == 1 && !NOISE) {  // the words themselves: 0.0 past L encodes to 0, and is not stored
                    m[4 * j + 0] += codec_encode<STOCHASTIC>(s + 0 < L ? v.x : 0.0f, clip, scale, r[4 * j + 0], nclip);
                    m[4 * j + 1] += codec_encode<STOCHASTIC>(s + 1 < L ? v.y : 0.0f, clip, scale, r[4 * j + 1], nclip);
                    m[4 * j + 2] += codec_encode<STOCHASTIC>(s + 2 < L ? v.z : 0.0f, clip, scale, r[4 * j + 2], nclip);
                    m[4 * j + 3] += codec_encode<STOCHASTIC>(s + 3 < L ? v.w : 0.0f, clip, scale, r[4 * j + 3], nclip);
                    continue;
                }
                const uint32_t u0 = codec_field<STOCHASTIC>(s + 0 < L, v.x, clip, scale, r[4 * j + 0], bias, nclip);
                const uint32_t u1 = codec_field<STOCHASTIC>(s + 1 < L, v.y, clip, scale, r[4 * j + 1], bias, nclip);
                const uint32_t u2 = codec_field<STOCHASTIC>(s + 2 < L, v.z, clip, scale, r[4 * j + 2], bias, nclip);
                const uint32_t u3 = codec_field<STOCHASTIC>(s + 3 < L, v.w, clip, scale, r[4 * j + 3], bias, nclip);
                if constexpr (P == 1) {  // bias is 0: the words themselves, less b / 2 (words past L are not stored)
                    m[4 * j + 0] += u0 - half;
                    m[4 * j + 1] += u1 - half;
                    m[4 * j + 2] += u2 - half;
                    m[4 * j + 3] += u3 - half;
                } else if constexpr (P == 4) {
                    e[j] = u0 | (u1 << W) | (u2 << 2 * W) | (u3 << 3 * W);
                } else {
                    e[2 * j + 0] = u0 | (u1 << W);
                    e[2 * j + 1] = u2 | (u3 << W);
                }
            }
            if constexpr (OWN) {
                R[(4 / P) * d] += u32x4{e[0], e[1], e[2], e[3]};
                if constexpr (P == 2) R[2 * d + 1] += u32x4{e[4], e[5], e[6], e[7]};
            } else if constexpr (FIFTH) {
                u32x4 *E4 = lds + 4 * 256 + 4 * lane;
                E4[(4 / P) * d] = u32x4{e[0], e[1], e[2], e[3]};
                if constexpr (P == 2) E4[2 * d + 1] = u32x4{e[4], e[5], e[6], e[7]};
            }
        }
        clipped_add(clipped, i, nclip, lane);
    }
    tile_meet_store<OWN, FIFTH ? 5 : 4>(lds, R, m, nneg, out + (uint64_t)i * out_pitch, tile, Lw);
}

// encode_mask_kernel's sibling for the table mode of the noise (gauss_block_add): the same workgroup, units, dealing,
// encoding pass and meet as encode_mask_kernel<P, STOCHASTIC, true>, over the same helpers, in a kernel of its own so
// that encode_mask_kernel's twelve instantiations keep their arguments and their instructions.  What differs:
// the workgroup first copies the T = 2 tau table entries to LDS, behind the waves' regions (dynamic LDS of 8 T bytes:
// the launch sizes it by T, not by the largest table); a client has P noise units, one per parameter block of the
// lane, each two ChaCha blocks and 16 counts; at P = 1 the encoding wave subtracts tau where it subtracts b / 2 there.
// No waves-per-SIMD pin: the allocator's own choice stands (profiles/dgauss_resources.txt).  Nothing spills.
template <int P, bool STOCHASTIC>
__global__ __launch_bounds__(256) void encode_gauss_mask_kernel(const float *__restrict__ x, uint64_t x_pitch,
                                                                const int64_t *__restrict__ seg,
                                                                const uint8_t *__restrict__ seeds,
                                                                const int8_t *__restrict__ signs,
                                                                const uint8_t *__restrict__ dither,
                                                                const uint8_t *__restrict__ noise,
                                                                const uint64_t *__restrict__ cdt, uint32_t T, uint64_t L,
                                                                uint64_t Lw, uint32_t tiles, float clip, float scale,
                                                                uint32_t bias, uint32_t *__restrict__ out,
                                                                uint64_t out_pitch, uint32_t *__restrict__ clipped) {
    static_assert(P == 1 || P == 2 || P == 4, "one, two or four fields per word");
    constexpr int E = STOCHASTIC ? P : 1;
    constexpr bool OWN = P > 1;  // packed words add into the wave's own region
    __shared__ u32x4 lds[4 * 256];  // one 4 KiB region per wave
    extern __shared__ __attribute__((aligned(8))) uint64_t tab[];  // the table: T entries
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x / tiles, tile = blockIdx.x - i * tiles;
    const uint32_t ctr = tile * 64u + (uint32_t)lane;
    const uint64_t par0 = (uint64_t)P * ((uint64_t)tile * 1024u + 16u * (uint64_t)lane);  // the lane's first parameter
    const int64_t k_lo = seg[i];
    const int64_t n_noise = P, n_units = n_noise + (seg[i + 1] - k_lo);

    u32x4 *R = lds + w * 256 + 4 * lane;  // the lane's 16 words of its wave's partial
    if constexpr (OWN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) R[j] = u32x4{0u, 0u, 0u, 0u};
    }
    for (uint32_t t = threadIdx.x; t < T; t += 256u) tab[t] = cdt[t];
    __syncthreads();
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) m[j] = 0u;
    uint32_t nneg = 0;
    const int rank = 3 - w;
#pragma unroll 1
    for (int64_t u = first_unit<E>(rank); u < n_units; u = next_unit<E>(u)) {  // two bodies in the loop: kept rolled
        if (u < n_noise) {
            // 2 ceil(L / 16) <= 2^32 (the call's length rule): both counters of a parameter block the row has stay
            // below 2^32; a block past L may wrap, and is predicated away or never stored
            gauss_block_add<P>(noise + 32 * (size_t)i, (uint32_t)P * ctr + (uint32_t)u, tab, T, par0 + 16u * (uint32_t)u, L,
                               m, R + (4 / P) * (uint32_t)u);
            continue;
        }
        const int64_t k = k_lo + (u - n_noise);
        const bool neg = signs[k] < 0;
        nneg += neg ? 1u : 0u;
        chacha_raw_add(seeds + 32 * (size_t)k, ctr, neg ? ~kAbcd : kAbcd, m);  // -(ks ^ C) = (ks ^ ~C) + 1
    }
    if (rank == 0) {
        const float *xr = x + (uint64_t)i * x_pitch;
        const uint32_t half = T >> 1;  // tau
        uint32_t nclip = 0;
#pragma unroll 1
        for (int d = 0; d < P; ++d) {
            constexpr int W = 32 / P;
            uint32_t r[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) r[j] = 0u;
            // parameters below 2^36 (the call's range rule): the dither block counter stays below 2^32
            if constexpr (STOCHASTIC) chacha_raw_add(dither + 32 * (size_t)i, (uint32_t)P * ctr + (uint32_t)d, kAbcd, r);
            uint32_t e[16 / P];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint64_t s = par0 + 16u * (uint32_t)d + 4u * j;
                // a quad that straddles L stays inside the row (x_pitch >= round_up(L, 4))
                const float4 v = s < L ? *reinterpret_cast<const float4 *>(xr + s) : make_float4(0.f, 0.f, 0.f, 0.f);
                const uint32_t u0 = codec_field<STOCHASTIC>(s + 0 < L, v.x, clip, scale, r[4 * j + 0], bias, nclip);
                const uint32_t u1 = codec_field<STOCHASTIC>(s + 1 < L, v.y, clip, scale, r[4 * j + 1], bias, nclip);
                const uint32_t u2 = codec_field<STOCHASTIC>(s + 2 < L, v.z, clip, scale, r[4 * j + 2], bias, nclip);
                const uint32_t u3 = codec_field<STOCHASTIC>(s + 3 < L, v.w, clip, scale, r[4 * j + 3], bias, nclip);
                if constexpr (P == 1) {  // bias is 0: the words themselves, less tau (words past L are not stored)
                    m[4 * j + 0] += u0 - half;
                    m[4 * j + 1] += u1 - half;
                    m[4 * j + 2] += u2 - half;
                    m[4 * j + 3] += u3 - half;
                } else if constexpr (P == 4) {
                    e[j] = u0 | (u1 << W) | (u2 << 2 * W) | (u3 << 3 * W);
                } else {
                    e[2 * j + 0] = u0 | (u1 << W);
                    e[2 * j + 1] = u2 | (u3 << W);
                }
            }
            if constexpr (OWN) {
                R[(4 / P) * d] += u32x4{e[0], e[1], e[2], e[3]};
                if constexpr (P == 2) R[2 * d + 1] += u32x4{e[4], e[5], e[6], e[7]};
            }
        }
        clipped_add(clipped, i, nclip, lane);
    }
    tile_meet_store<OWN, 4>(lds, R, m, nneg, out + (uint64_t)i * out_pitch, tile, Lw);
}

// One field of a summed word as the mean of `count` contributors; cb = count B.
template <int P>
__device__ __forceinline__ float unpack_field(uint32_t S, int j, int64_t cb, double denom) {
    constexpr int W = 32 / P;
    return (float)((double)((int64_t)((S >> (W * j)) & ((1u << W) - 1u)) - cb) / denom);
}

// the four floats of one word (P = 4), or of two (P = 2)
template <int P>
__device__ __forceinline__ float4 unpack_four(uint32_t S0, uint32_t S1, int64_t cb, double denom) {
    if constexpr (P == 4)
        return make_float4(unpack_field<4>(S0, 0, cb, denom), unpack_field<4>(S0, 1, cb, denom),
                           unpack_field<4>(S0, 2, cb, denom), unpack_field<4>(S0, 3, cb, denom));
    else
        return make_float4(unpack_field<2>(S0, 0, cb, denom), unpack_field<2>(S0, 1, cb, denom),
                           unpack_field<2>(S1, 0, cb, denom), unpack_field<2>(S1, 1, cb, denom));
}

// out[P l' + j] = float32(float64(field j of sum[l'] - count B) / denom), P l' + j < L; denom = count 2^f
// (SA_ServiceAgent.py:538-540, 605: the final sum, as a mean).  A thread reads a quad of words (16 bytes) and
// writes its 4 P floats with 16-byte stores; the up to 4 P - 1 parameters behind the last whole quad go one per
// thread.  Not in place: the output is P times the input.
template <int P>
__global__ __launch_bounds__(256) void decode_unpack_kernel(const uint32_t *__restrict__ sum, uint64_t L, int64_t cb,
                                                            double denom, float *__restrict__ out) {
    const uint64_t quads = L / (4 * P), stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t q = t0; q < quads; q += stride) {
        const uint4 s = reinterpret_cast<const uint4 *>(sum)[q];
        float4 *dst = reinterpret_cast<float4 *>(out) + P * q;
        if constexpr (P == 4) {
            dst[0] = unpack_four<4>(s.x, 0u, cb, denom);
            dst[1] = unpack_four<4>(s.y, 0u, cb, denom);
            dst[2] = unpack_four<4>(s.z, 0u, cb, denom);
            dst[3] = unpack_four<4>(s.w, 0u, cb, denom);
        } else {
            dst[0] = unpack_four<2>(s.x, s.y, cb, denom);
            dst[1] = unpack_four<2>(s.z, s.w, cb, denom);
        }
    }
    const uint64_t l = 4 * P * quads + t0;  // the tail, per element: fewer than 4 P parameters
    if (l < L) out[l] = unpack_field<P>(sum[l / P], (int)(l % P), cb, denom);
}

// One step of the modular decode's cascade (include/flamingo_hip.h, "decode modulo the field"): r is the summed word
// less the fields already done, cb = count B_n mod 2^32.  d = r - cb mod 2^32; Qh, returned, is d's low W bits centred
// into [-H, H - 1] (a sign extension); r becomes (d - Qh) >> W, whose dropped low W bits are 0, so the field's carry or
// borrow goes up with it.
template <int P>
__device__ __forceinline__ int32_t unpack_mod_step(uint32_t &r, uint32_t cb) {
    constexpr int W = 32 / P;
    const uint32_t d = r - cb;
    const int32_t q = (int32_t)(d << (32 - W)) >> (32 - W);
    r = (d - (uint32_t)q) >> W;
    return q;
}

// Qh as the mean of `count` contributors (denom = count 2^f: decode_unpack_kernel's division and single rounding), with
// |Qh| taken into the thread's near count and maximum; |Qh| <= H = 2^(W - 1), so Qh = -H counts as H.
__device__ __forceinline__ float unpack_mod_mean(int32_t q, double denom, uint32_t guard, uint32_t &near, uint32_t &most) {
    const uint32_t a = (uint32_t)(q < 0 ? -q : q);
    near += a >= guard ? 1u : 0u;
    most = a > most ? a : most;
    return (float)((double)q / denom);
}

// the four floats of one word (P = 4), or of two (P = 2), field 0 of each word first
template <int P>
__device__ __forceinline__ float4 unpack_mod_four(uint32_t S0, uint32_t S1, uint32_t cb, double denom, uint32_t guard,
                                                  uint32_t &near, uint32_t &most) {
    float o[4];
    if constexpr (P == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = unpack_mod_mean(unpack_mod_step<4>(S0, cb), denom, guard, near, most);
    } else {
        o[0] = unpack_mod_mean(unpack_mod_step<2>(S0, cb), denom, guard, near, most);
        o[1] = unpack_mod_mean(unpack_mod_step<2>(S0, cb), denom, guard, near, most);
        o[2] = unpack_mod_mean(unpack_mod_step<2>(S1, cb), denom, guard, near, most);
        o[3] = unpack_mod_mean(unpack_mod_step<2>(S1, cb), denom, guard, near, most);
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

// decode_unpack_kernel's sibling for sums taken modulo the field (SA_ServiceAgent.py:538-540, 605: the final sum, as a
// mean): out[P l' + j] = float32(float64(Qh_j) / denom), P l' + j < L, Qh_j by the cascade above, so a field of the sum
// may have carried into the one above it.  The same traffic and launch as decode_unpack_kernel: a quad of words in, 4 P
// floats out in 16-byte stores, the up to 4 P - 1 parameters behind the last whole quad one per thread (its word's
// cascade run up to that field).  stats (or NULL): a thread keeps its near count and its maximum over its grid-stride
// trips, a wave reduces them with __shfl_xor as clipped_add does, and lane 0 issues at most one atomicAdd (stats[0]) and
// one atomicMax (stats[1]).  Every parameter below L is counted once, by the thread that writes it.
template <int P>
__global__ __launch_bounds__(256) void decode_unpack_mod_kernel(const uint32_t *__restrict__ sum, uint64_t L, uint32_t cb,
                                                                double denom, uint32_t guard, float *__restrict__ out,
                                                                uint32_t *__restrict__ stats) {
    const uint64_t quads = L / (4 * P), stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t near = 0, most = 0;
    for (uint64_t q = t0; q < quads; q += stride) {
        const uint4 s = reinterpret_cast<const uint4 *>(sum)[q];
        float4 *dst = reinterpret_cast<float4 *>(out) + P * q;
        if constexpr (P == 4) {
            dst[0] = unpack_mod_four<4>(s.x, 0u, cb, denom, guard, near, most);
            dst[1] = unpack_mod_four<4>(s.y, 0u, cb, denom, guard, near, most);
            dst[2] = unpack_mod_four<4>(s.z, 0u, cb, denom, guard, near, most);
            dst[3] = unpack_mod_four<4>(s.w, 0u, cb, denom, guard, near, most);
        } else {
            dst[0] = unpack_mod_four<2>(s.x, s.y, cb, denom, guard, near, most);
            dst[1] = unpack_mod_four<2>(s.z, s.w, cb, denom, guard, near, most);
        }
    }
    const uint64_t l = 4 * P * quads + t0;  // the tail, per element: fewer than 4 P parameters
    if (l < L) {
        uint32_t r = sum[l / P];
        int32_t q = 0;
        for (int j = 0; j <= (int)(l % P); ++j) q = unpack_mod_step<P>(r, cb);  // the fields below are other threads'
        out[l] = unpack_mod_mean(q, denom, guard, near, most);
    }
    if (!stats) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        near += __shfl_xor(near, off);
        const uint32_t other = __shfl_xor(most, off);
        most = other > most ? other : most;
    }
    if ((threadIdx.x & 63) == 0) {
        if (near) atomicAdd(stats, near);
        if (most) atomicMax(stats + 1, most);
    }
}

// ------------------------------------------------------------ randomised block Hadamard rotation
// A float -> float step in front of the codec and behind its decode (include/flamingo_hip.h, DESIGN.md section 5,
// tests/rotate_cases.py): per block of H = 2^h parameters, forward: non-finite -> +0.0 (counted), sign flips,
// butterfly stages 0 .. h - 1 in that order, one multiply by c_h; inverse: the stages, the multiply, the flips.

// The tile's LDS image: element idx of the tile lives at word rot_sw(idx), idx with bits 2..3 XORed by bits 5..6
// and bit 4 by bit 8.  Bits 0..1 stay, so four consecutive elements stay one aligned 16-byte quad.  Banks
// (MI355X: b32 accesses in two groups of 32 lanes, bank = word mod 32, bits 0..4 of the word; b128 stores in
// groups of 8 lanes, bank = word mod 32; b128 loads in the four 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,
// 28-31} and those + 32, bank = word mod 64), with t the thread and t_i its bits:
//   first write, b128, idx = 16 t + 4 q: the 8 lanes of a group differ in t_0..t_2 = idx bits 4..6; word bits
//     2..4 are (q_0 ^ t_1, q_1 ^ t_2, t_0 ^ t_4): a bijection of t_0..t_2, 8 quads on 8 different quad-banks;
//   second access (read, and the write back to the same words), b32, idx = (t >> 4) << 8 | k << 4 | (t & 15):
//     the 32 lanes of a group differ in t_0..t_4 = idx bits 0..3 and 8; word bits 0..4 are (t_0, t_1,
//     t_2 ^ k_1, t_3 ^ k_2, k_0 ^ t_4): a bijection of t_0..t_4, 32 banks;
//   third access (read and write back), b32, idx = k << 8 | t: the lanes differ in idx bits 0..4, bits 5, 6 and 8
//     are the group's own: word bits 0..4 are t_0..t_4 XOR a constant, 32 banks;
//   last read, b128, idx = 1024 m + 4 t: word bits 2..5 are (t_0 ^ t_3, t_1 ^ t_4, t_2 ^ t_6, t_3); a 16-lane
//     group is four runs of four lanes whose (t_2, t_3) are (0,0), (1,1), (1,0), (0,1) in some order with t_4
//     fixed per run, so (bit 4, bit 5) tells the runs apart and (bit 2, bit 3) the lanes of a run: 16 quads on
//     the 16 quad-banks.
// So no access conflicts at all.
__device__ __forceinline__ int rot_sw(int idx) { return idx ^ (((idx >> 5) & 3) << 2) ^ (((idx >> 8) & 1) << 4); }

// Stages LO .. LO + 3 on 16 values, v[k] the element whose index bits LO .. LO + 3 are k; stages >= h are skipped
// (h is uniform over the launch: scalar branches).
template <int LO>
__device__ __forceinline__ void rot_stages(float (&v)[16], int h) {
#pragma clang fp contract(off)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (LO + s < h) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i >> s & 1) continue;
                const float a = v[i], b = v[i | 1 << s];
                v[i] = a + b;
                v[i | 1 << s] = a - b;
            }
        }
    }
}

__device__ __forceinline__ float rot_flip(float v, uint32_t bits, int j) {
    return __uint_as_float(__float_as_uint(v) ^ ((bits >> j & 1u) << 31));
}

// The float front end's thread geometry: a workgroup takes one tile of a row, 16 parameters a thread.
static_assert(256 * 16 == kFloatTile, "256 threads x 16 parameters are one tile");

// NaN or +-Inf: what the forward rotation, and the clip in front of it, take as +0.0
__device__ __forceinline__ bool rot_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// The forward read of a row of L floats: v = parameters p0 .. p0 + 15 (p0 a multiple of 16) as four 16-byte loads,
// 0.0 for every parameter at or past L (a predicate per element: the padding of a row may hold anything).
// rotate_kernel and l2_sumsq_kernel both read a row through this one body and rot_nonfinite, so the clip's sum is
// over exactly the values the rotation sees.
__device__ __forceinline__ void rot_read16(const float *xr, uint64_t p0, uint64_t L, float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t s = p0 + 4u * j;
        // a quad that straddles L stays inside the row (x_pitch >= round_up(L, 4))
        const float4 q = s < L ? *reinterpret_cast<const float4 *>(xr + s) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[4 * j] = s < L ? q.x : 0.0f, v[4 * j + 1] = s + 1 < L ? q.y : 0.0f;
        v[4 * j + 2] = s + 2 < L ? q.z : 0.0f, v[4 * j + 3] = s + 3 < L ? q.w : 0.0f;
    }
}

// Four results at parameter s of a row of L, s < L a multiple of 4: one 16-byte store, the last quad of a row element
// by element (nothing at or behind L is written).
__device__ __forceinline__ void rot_store4(float *orow, uint64_t s, uint64_t L, float4 q) {
    if (s + 3 < L) {
        *reinterpret_cast<float4 *>(orow + s) = q;
    } else {
        orow[s] = q.x;
        if (s + 1 < L) orow[s + 1] = q.y;
        if (s + 2 < L) orow[s + 2] = q.z;
    }
}

// out = the rotation of x, rows of L parameters taken as L_rot = round_up(L, 2^h): forward reads L floats a row
// (rot_read16) and writes L_rot, inverse reads L_rot and writes the L (rot_store4).  Workgroup g = (row,
// 4096-parameter tile) = (g / tiles, g % tiles) of a one-dimensional grid; a tile holds whole blocks.  Thread t
// loads parameters 16 t .. 16 t + 15 (four 16-byte loads) and runs stages 0..3 in registers; PHASES = ceil(h / 4)
// > 1: the tile goes through LDS (rot_sw above) and the thread takes the 16 elements that differ in index bits 4..7
// for stages 4..7, and PHASES = 3 once more those in bits 8..11.  The scaled values go back to the words they came
// from and the tile is stored from LDS in order, 16 bytes a thread and 4 KiB contiguous per store instruction of
// the workgroup (PHASES = 1 stores its registers, 64 bytes contiguous a thread).  Every global load of a tile
// precedes its first barrier, and a thread of PHASES = 1 writes what it alone read, so out may be x.  sign_bits:
// ceil(L_rot / 32) words of PRG(key), bit l % 32 of word l / 32 flips parameter l.
// nonfinite[row] (forward, zeroed by the call, or NULL): the threads' counts meet in LDS, the first wave adds them
// up and its first lane adds a non-zero total with one atomic.
// FACTOR (forward only): the L2 clip rides in the load (the section below): every finite input is first multiplied
// by row_factor[row], one float32 multiply between the non-finite zeroing and the sign flip; the row is the
// workgroup's, so the factor is one scalar load.  Without FACTOR row_factor is not read.
template <bool INVERSE, int PHASES, bool FACTOR>
__global__ __launch_bounds__(256) void rotate_kernel(const float *x, uint64_t x_pitch, uint64_t L, uint64_t L_rot,
                                                     uint32_t tiles, int h, float scale,
                                                     const uint32_t *__restrict__ sign_bits, float *out,
                                                     uint64_t out_pitch, uint32_t *__restrict__ nonfinite,
                                                     const float *__restrict__ row_factor) {
#pragma clang fp contract(off)
    static_assert(!(INVERSE && FACTOR), "the clip is the forward rotation's");
    __shared__ float4 lds4[PHASES > 1 ? 1024 : 1];  // the tile: 16 KiB
    __shared__ uint32_t cnt[INVERSE ? 1 : 256];
    float *lds = reinterpret_cast<float *>(lds4);
    const int t = threadIdx.x;
    const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const uint64_t base = (uint64_t)tile * kFloatTile;
    const float *xr = x + (uint64_t)row * x_pitch;
    float *orow = out + (uint64_t)row * out_pitch;

    // four consecutive results at parameter s of the row (s a multiple of 4, so they share a sign word)
    auto emit = [&](uint64_t s, float4 q) {
        if constexpr (!INVERSE) {
            if (s < L_rot) *reinterpret_cast<float4 *>(orow + s) = q;
        } else {
            if (s >= L) return;
            const uint32_t b = sign_bits[s >> 5] >> (s & 31);
            q = make_float4(rot_flip(q.x, b, 0), rot_flip(q.y, b, 1), rot_flip(q.z, b, 2), rot_flip(q.w, b, 3));
            rot_store4(orow, s, L, q);
        }
    };

    float v[16];
    const uint64_t p0 = base + 16u * (uint64_t)t;  // 16 parameters: all below L_rot, or none
    if constexpr (INVERSE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 q = p0 < L_rot ? *reinterpret_cast<const float4 *>(xr + p0 + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[4 * j] = q.x, v[4 * j + 1] = q.y, v[4 * j + 2] = q.z, v[4 * j + 3] = q.w;
        }
    } else {
        uint32_t bad = 0;
        const uint32_t sb = p0 < L_rot ? sign_bits[p0 >> 5] >> (p0 & 16) : 0u;
        float rf = 1.0f;
        if constexpr (FACTOR) rf = row_factor[row];
        rot_read16(xr, p0, L, v);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool nf = rot_nonfinite(v[j]);
            bad += nf ? 1u : 0u;
            if constexpr (FACTOR) v[j] = rot_flip(nf ? 0.0f : v[j] * rf, sb, j);
            else v[j] = rot_flip(nf ? 0.0f : v[j], sb, j);
        }
        if (nonfinite) cnt[t] = bad;
    }
    rot_stages<0>(v, h);

    if constexpr (PHASES == 1) {
        if constexpr (!INVERSE) {
            if (nonfinite) __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            emit(p0 + 4u * j, make_float4(v[4 * j] * scale, v[4 * j + 1] * scale, v[4 * j + 2] * scale, v[4 * j + 3] * scale));
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            lds4[rot_sw(16 * t + 4 * q) >> 2] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        __syncthreads();
        const int i1 = (t >> 4) << 8 | (t & 15);
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = lds[rot_sw(i1 | k << 4)];
        rot_stages<4>(v, h);
        if constexpr (PHASES == 2) {
#pragma unroll
            for (int k = 0; k < 16; ++k) lds[rot_sw(i1 | k << 4)] = v[k] * scale;
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) lds[rot_sw(i1 | k << 4)] = v[k];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = lds[rot_sw(k << 8 | t)];
            rot_stages<8>(v, h);
#pragma unroll
            for (int k = 0; k < 16; ++k) lds[rot_sw(k << 8 | t)] = v[k] * scale;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m) emit(base + 1024u * m + 4u * t, lds4[rot_sw(1024 * m + 4 * t) >> 2]);
    }

    if constexpr (!INVERSE) {
        if (nonfinite && t < 64) {  // after the first barrier of either shape
            uint32_t c = cnt[t] + cnt[t + 64] + cnt[t + 128] + cnt[t + 192];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
            if (t == 0 && c) atomicAdd(nonfinite + row, c);
        }
    }
}

// ------------------------------------------------------------ L2 clip of float updates
// The step in front of the rotation (include/flamingo_hip.h has the rule, tests/l2_cases.py restates it): per row
// the sum S of the squares in float64, in an order that depends on L alone, the factor s = min(1, C / sqrt(S)) as a
// float32, and x s.  No atomics anywhere: every add has fixed operands.

// a <- a + a[lane ^ off] for off = 1, 2, 4, 8, 16, 32: both lanes of a pair add the same two values (IEEE addition
// commutes), so every lane of the wave ends with the same bits.
__device__ __forceinline__ double l2_wave_sum(double a) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) a = a + __shfl_xor(a, off);
    return a;
}

// work[row tiles + tile] = the tile's partial sum of squares.  Workgroup g = (row, 4096-parameter tile) and thread t
// of it takes parameters 16 t .. 16 t + 15 of the tile through rot_read16 and rot_nonfinite, rotate_kernel's own read:
// what the rotation reads as +0.0 counts as +0.0.  The square of a float is exact in float64, so fma(d, d, acc) is
// acc + d d, added in the order v[0] .. v[15].
__global__ __launch_bounds__(256) void l2_sumsq_kernel(const float *__restrict__ x, uint64_t x_pitch, uint64_t L,
                                                       uint32_t tiles, double *__restrict__ work) {
#pragma clang fp contract(off)
    __shared__ double wave_sums[4];
    const int t = threadIdx.x;
    const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const float *xr = x + (uint64_t)row * x_pitch;
    float v[16];
    rot_read16(xr, (uint64_t)tile * kFloatTile + 16u * (uint64_t)t, L, v);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const double d = (double)(rot_nonfinite(v[j]) ? 0.0f : v[j]);
        acc = fma(d, d, acc);
    }
    acc = l2_wave_sum(acc);
    if ((t & 63) == 0) wave_sums[t >> 6] = acc;
    __syncthreads();
    if (t == 0) work[(uint64_t)row * tiles + tile] = ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

// One wave per row: lane k adds the row's partials k, k + 64, ... in that order, the wave sum is S, and
// factors[row] = S <= C^2 ? 1 : float32(C / sqrt(S)) in float64 (C^2 is exact there); sumsq[row] = S when asked.
__global__ __launch_bounds__(64) void l2_factor_kernel(const double *__restrict__ work, uint32_t tiles, float clip_norm,
                                                      float *__restrict__ factors, double *__restrict__ sumsq) {
#pragma clang fp contract(off)
    const uint32_t row = blockIdx.x;
    const double *w = work + (uint64_t)row * tiles;
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < tiles; i += 64) acc = acc + w[i];
    const double S = l2_wave_sum(acc);
    if (threadIdx.x == 0) {
        const double C = (double)clip_norm;
        factors[row] = S <= C * C ? 1.0f : (float)(C / sqrt(S));
        if (sumsq) sumsq[row] = S;
    }
}

// out = x factors[row] over the L parameters of every row, one float32 multiply each (plain IEEE: NaN stays NaN, a
// factor of 1 leaves the bits).  Workgroup g = (row, 4096-parameter tile); thread t takes the quads t, t + 256,
// t + 512, t + 768 of the tile, 16 bytes a load and a store (rot_store4 at the end of a row).  A thread
// writes what it alone read, so out may be x at equal pitches.
__global__ __launch_bounds__(256) void scale_rows_kernel(const float *x, uint64_t x_pitch, uint64_t L, uint32_t tiles,
                                                         const float *__restrict__ factors, float *out,
                                                         uint64_t out_pitch) {
#pragma clang fp contract(off)
    const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const float f = factors[row];
    const float *xr = x + (uint64_t)row * x_pitch;
    float *orow = out + (uint64_t)row * out_pitch;
    float4 q[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint64_t s = (uint64_t)tile * kFloatTile + 1024u * m + 4u * threadIdx.x;
        q[m] = s < L ? *reinterpret_cast<const float4 *>(xr + s) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint64_t s = (uint64_t)tile * kFloatTile + 1024u * m + 4u * threadIdx.x;
        if (s < L) rot_store4(orow, s, L, make_float4(q[m].x * f, q[m].y * f, q[m].z * f, q[m].w * f));
    }
}

// ------------------------------------------------------------ conditional stochastic rounding
// The pass in front of the stochastic encode (include/flamingo_hip.h has the rule, tests/round_cases.py restates it):
// for each of A candidate dither seeds a row, Q = the sum of q^2 over the row, q the integers encode_mask_kernel
// would round to under that seed; then the first candidate whose Q is within the bound.  Integer sums: exact in
// any order, atomics included.  Nothing of q is stored.

// a <- a + a[lane ^ off] for off = 1 .. 32, as l2_wave_sum, on 64-bit integers
__device__ __forceinline__ uint64_t round_wave_sum(uint64_t a) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) a += (uint64_t)__shfl_xor((unsigned long long)a, off);
    return a;
}

// sumsq[row A + a] += the tile's share of Q(candidate a of the row), a < A <= 8; sumsq zeroed by the call.  Workgroup
// g = (row, 4096-parameter tile) and thread t of it takes parameters 16 t .. 16 t + 15 of the tile through
// rot_read16, once, and keeps them; they are block 256 tile + t of every candidate's dither stream, words in
// parameter order, which is the block and the order encode_mask_kernel draws for them in every pack mode.  Per
// candidate: one ChaCha block from the key at its wave-uniform address (chacha_raw_add), the 16 q through
// codec_encode<true> itself -- the codec's NaN and clip rule, not rot_nonfinite: +-Inf clips to +-c -- squared as
// int64 and summed in uint64 (L B^2 <= 2^64 - 1, the call's rule: no sum wraps).  A parameter at or past L reads as
// +0.0, which encodes to 0 under any dither word; a thread with none below L skips the ChaCha.  The wave's sums meet
// by shuffles, the four waves' in LDS, and thread a adds the tile's total with one 64-bit atomic.
__global__ __launch_bounds__(256) void round_sumsq_kernel(const float *__restrict__ x, uint64_t x_pitch, uint64_t L,
                                                          uint32_t tiles, const uint8_t *__restrict__ candidates, int A,
                                                          float clip, float scale,
                                                          unsigned long long *__restrict__ sumsq) {
    __shared__ uint64_t wave_sums[4][8];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const uint64_t p0 = (uint64_t)tile * kFloatTile + 16u * (uint64_t)t;
    float v[16];
    rot_read16(x + (uint64_t)row * x_pitch, p0, L, v);
    // ceil(L / 16) <= 2^32 (the call's length rule): the counter of a block the row has stays below 2^32
    const uint32_t blk = tile * 256u + (uint32_t)t;
    const uint8_t *keys = candidates + 32 * (size_t)row * (size_t)A;
#pragma unroll 1
    for (int a = 0; a < A; ++a) {
        uint64_t acc = 0;
        if (p0 < L) {
            uint32_t r[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) r[j] = 0u;
            chacha_raw_add(keys + 32 * (size_t)a, blk, kAbcd, r);
            uint32_t nclip = 0;  // thrown away: the encode counts
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int64_t q = (int64_t)(int32_t)codec_encode<true>(v[j], clip, scale, r[j], nclip);
                acc += (uint64_t)(q * q);
            }
        }
        acc = round_wave_sum(acc);
        if (lane == 0) wave_sums[w][a] = acc;
    }
    __syncthreads();
    if (t < A)
        atomicAdd(sumsq + (uint64_t)row * (uint64_t)A + (uint64_t)t,
                  (unsigned long long)(wave_sums[0][t] + wave_sums[1][t] + wave_sums[2][t] + wave_sums[3][t]));
}

// One thread per row: chosen[row] = the smallest a < A with sumsq[row A + a] <= max_sumsq, or A when there is none,
// and dither[row] = that candidate's 32 bytes (candidate 0's when there is none), copied byte by byte: no alignment
// is asked of either array.
__global__ __launch_bounds__(64) void round_select_kernel(const unsigned long long *__restrict__ sumsq,
                                                          const uint8_t *__restrict__ candidates, int N, int A,
                                                          unsigned long long max_sumsq, uint8_t *__restrict__ dither,
                                                          uint32_t *__restrict__ chosen) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= N) return;
    int pick = A;
    for (int a = A - 1; a >= 0; --a)
        if (sumsq[(size_t)row * (size_t)A + (size_t)a] <= max_sumsq) pick = a;
    chosen[row] = (uint32_t)pick;
    const uint8_t *src = candidates + 32 * ((size_t)row * (size_t)A + (size_t)(pick < A ? pick : 0));
    for (int b = 0; b < 32; ++b) dither[32 * (size_t)row + b] = src[b];
}

#undef FLM_QR
#undef FLM_ROTL

// ----------------------------------------------------------------- launchers
uint64_t encode_mask_groups(int N, uint64_t L) { return (uint64_t)N * ((L + 1023) / 1024); }

hipError_t launch_encode_mask(const float *d_x, uint64_t x_pitch, int N, const int64_t *d_seg, const uint8_t *d_seeds,
                              const int8_t *d_signs, const uint8_t *d_dither, const uint8_t *d_noise, uint64_t L,
                              const CodecParams &c, uint32_t *d_out, uint64_t out_pitch, uint32_t *d_clipped,
                              hipStream_t stream) {
    if (c.pack != 1 && c.pack != 2 && c.pack != 4) return hipErrorInvalidValue;
    if (c.noise_bits < 0 || c.noise_bits > 1024 || c.noise_bits % 2 || (c.noise_bits && !d_noise)) return hipErrorInvalidValue;
    const uint64_t Lw = (L + (uint64_t)c.pack - 1) / (uint64_t)c.pack;
    const uint64_t groups = encode_mask_groups(N, Lw);
    if (groups == 0) return hipSuccess;
    if (groups > 0x7fffffffull || c.frac_bits < 0 || c.frac_bits > 30) return hipErrorInvalidValue;
    const uint32_t tiles = (uint32_t)((Lw + 1023) / 1024);
    const float scale = (float)(1u << c.frac_bits);
    const uint32_t draws = (uint32_t)(c.noise_bits + 31) / 32, r = (uint32_t)c.noise_bits % 32;
    const uint32_t last_mask = r ? (1u << r) - 1u : 0xffffffffu, half = (uint32_t)c.noise_bits / 2;
    // [pack / 2][stochastic][noise]: pack is 1, 2 or 4 (refused above otherwise), so pack / 2 is 0, 1 or 2
#define FLM_E(P) {{encode_mask_kernel<P, false, false>, encode_mask_kernel<P, false, true>}, \
                  {encode_mask_kernel<P, true, false>, encode_mask_kernel<P, true, true>}}
    static constexpr decltype(&encode_mask_kernel<1, false, false>) kernels[3][2][2] = {FLM_E(1), FLM_E(2), FLM_E(4)};
#undef FLM_E
    hipLaunchKernelGGL(kernels[c.pack / 2][d_dither != nullptr][c.noise_bits != 0], dim3((unsigned)groups), dim3(256), 0,
                       stream, d_x, x_pitch, d_seg, d_seeds, d_signs, d_dither, d_noise, draws, last_mask, half, L, Lw, tiles,
                       c.clip, scale, c.pack == 1 ? 0u : c.bias, d_out, out_pitch, d_clipped);
    return hipGetLastError();
}

hipError_t launch_encode_gauss_mask(const float *d_x, uint64_t x_pitch, int N, const int64_t *d_seg, const uint8_t *d_seeds,
                                    const int8_t *d_signs, const uint8_t *d_dither, const uint8_t *d_noise,
                                    const uint64_t *d_cdt, int tail, uint64_t L, const CodecParams &c, uint32_t *d_out,
                                    uint64_t out_pitch, uint32_t *d_clipped, hipStream_t stream) {
    if (c.pack != 1 && c.pack != 2 && c.pack != 4) return hipErrorInvalidValue;
    if (tail < 1 || tail > 512 || !d_noise || !d_cdt || ((uintptr_t)d_cdt & 7)) return hipErrorInvalidValue;
    const uint64_t Lw = (L + (uint64_t)c.pack - 1) / (uint64_t)c.pack;
    const uint64_t groups = encode_mask_groups(N, Lw);
    if (groups == 0) return hipSuccess;
    if (groups > 0x7fffffffull || c.frac_bits < 0 || c.frac_bits > 30) return hipErrorInvalidValue;
    const uint32_t tiles = (uint32_t)((Lw + 1023) / 1024), T = 2u * (uint32_t)tail;
    const float scale = (float)(1u << c.frac_bits);
    // [pack / 2][stochastic], as launch_encode_mask's
    static constexpr decltype(&encode_gauss_mask_kernel<1, false>) kernels[3][2] = {
        {encode_gauss_mask_kernel<1, false>, encode_gauss_mask_kernel<1, true>},
        {encode_gauss_mask_kernel<2, false>, encode_gauss_mask_kernel<2, true>},
        {encode_gauss_mask_kernel<4, false>, encode_gauss_mask_kernel<4, true>}};
    hipLaunchKernelGGL(kernels[c.pack / 2][d_dither != nullptr], dim3((unsigned)groups), dim3(256), 8u * T, stream, d_x,
                       x_pitch, d_seg, d_seeds, d_signs, d_dither, d_noise, d_cdt, T, L, Lw, tiles, c.clip, scale,
                       c.pack == 1 ? 0u : c.bias, d_out, out_pitch, d_clipped);
    return hipGetLastError();
}

hipError_t launch_decode_unpack(const uint32_t *d_sum, uint64_t L, int pack, int64_t count_bias, double denom, float *d_out,
                                hipStream_t stream) {
    if (L == 0) return hipSuccess;
    if (pack != 2 && pack != 4) return hipErrorInvalidValue;
    const uint64_t quads = L / (4 * (uint64_t)pack);
    const unsigned g = (unsigned)std::min<uint64_t>(4096, (quads + 255) / 256 + 1);  // + 1: the tail's threads
    if (pack == 2)
        hipLaunchKernelGGL(decode_unpack_kernel<2>, dim3(g), dim3(256), 0, stream, d_sum, L, count_bias, denom, d_out);
    else
        hipLaunchKernelGGL(decode_unpack_kernel<4>, dim3(g), dim3(256), 0, stream, d_sum, L, count_bias, denom, d_out);
    return hipGetLastError();
}

hipError_t launch_decode_unpack_mod(const uint32_t *d_sum, uint64_t L, int pack, uint32_t count_bias, double denom,
                                    uint32_t guard, float *d_out, uint32_t *d_stats, hipStream_t stream) {
    if (L == 0) return hipSuccess;
    if (pack != 2 && pack != 4) return hipErrorInvalidValue;
    const uint64_t quads = L / (4 * (uint64_t)pack);
    const unsigned g = (unsigned)std::min<uint64_t>(4096, (quads + 255) / 256 + 1);  // launch_decode_unpack's grid
    if (pack == 2)
        hipLaunchKernelGGL(decode_unpack_mod_kernel<2>, dim3(g), dim3(256), 0, stream, d_sum, L, count_bias, denom, guard,
                           d_out, d_stats);
    else
        hipLaunchKernelGGL(decode_unpack_mod_kernel<4>, dim3(g), dim3(256), 0, stream, d_sum, L, count_bias, denom, guard,
                           d_out, d_stats);
    return hipGetLastError();
}

hipError_t launch_decode_sum(const uint32_t *d_sum, uint64_t n, double denom, float *d_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t g = std::min<uint64_t>(4096, (n / 4 + 255) / 256 + 1);
    hipLaunchKernelGGL(decode_sum_kernel, dim3((unsigned)g), dim3(256), 0, stream, d_sum, n, denom, d_out);
    return hipGetLastError();
}

uint64_t rotate_groups(int N, uint64_t L_rot) { return (uint64_t)N * float_tiles(L_rot); }

hipError_t launch_rotate(const float *d_x, uint64_t x_pitch, int N, uint64_t L, uint64_t L_rot, int log2_block,
                         const uint32_t *d_sign_bits, bool inverse, float *d_out, uint64_t out_pitch,
                         uint32_t *d_nonfinite, const float *d_factors, hipStream_t stream) {
    const uint64_t groups = rotate_groups(N, L_rot);
    if (groups == 0) return hipSuccess;
    if (groups > 0x7fffffffull || log2_block < 4 || log2_block > 12 || L_rot % (1u << log2_block) || L > L_rot ||
        (inverse && d_factors))
        return hipErrorInvalidValue;
    // c_h = float32(2^(-h / 2)): a power of two, times float32(sqrt(1 / 2)) = 0x3F3504F3 for odd h
    const uint32_t rsqrt2_bits = 0x3F3504F3u;
    float rsqrt2;
    memcpy(&rsqrt2, &rsqrt2_bits, sizeof rsqrt2);
    const float scale = ldexpf(log2_block % 2 ? rsqrt2 : 1.0f, -(log2_block / 2));
    // [forward, inverse, forward with the clip's multiply in its load][phases - 1], phases = ceil(h / 4)
    static constexpr decltype(&rotate_kernel<false, 1, false>) kernels[3][3] = {
        {rotate_kernel<false, 1, false>, rotate_kernel<false, 2, false>, rotate_kernel<false, 3, false>},
        {rotate_kernel<true, 1, false>, rotate_kernel<true, 2, false>, rotate_kernel<true, 3, false>},
        {rotate_kernel<false, 1, true>, rotate_kernel<false, 2, true>, rotate_kernel<false, 3, true>}};
    hipLaunchKernelGGL(kernels[d_factors ? 2 : inverse][(log2_block - 1) / 4], dim3((unsigned)groups), dim3(256), 0, stream,
                       d_x, x_pitch, L, L_rot, (uint32_t)float_tiles(L_rot), log2_block, scale, d_sign_bits, d_out, out_pitch,
                       inverse ? nullptr : d_nonfinite, d_factors);
    return hipGetLastError();
}

uint64_t l2_tiles(uint64_t L) { return float_tiles(L); }

hipError_t launch_l2_factors(const float *d_x, uint64_t x_pitch, int N, uint64_t L, float clip_norm, double *d_work,
                             float *d_factors, double *d_sumsq, hipStream_t stream) {
    const uint64_t tiles = l2_tiles(L);
    if (N < 1 || tiles == 0 || tiles > 0x7fffffffull / (uint64_t)N) return hipErrorInvalidValue;
    hipLaunchKernelGGL(l2_sumsq_kernel, dim3((unsigned)(tiles * (uint64_t)N)), dim3(256), 0, stream, d_x, x_pitch, L,
                       (uint32_t)tiles, d_work);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(l2_factor_kernel, dim3((unsigned)N), dim3(64), 0, stream, d_work, (uint32_t)tiles, clip_norm,
                       d_factors, d_sumsq);
    return hipGetLastError();
}

hipError_t launch_scale_rows(const float *d_x, uint64_t x_pitch, int N, uint64_t L, const float *d_factors, float *d_out,
                             uint64_t out_pitch, hipStream_t stream) {
    const uint64_t tiles = l2_tiles(L);
    if (N < 1 || tiles == 0 || tiles > 0x7fffffffull / (uint64_t)N) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)(tiles * (uint64_t)N)), dim3(256), 0, stream, d_x, x_pitch, L,
                       (uint32_t)tiles, d_factors, d_out, out_pitch);
    return hipGetLastError();
}

hipError_t launch_round_select(const float *d_x, uint64_t x_pitch, int N, uint64_t L, int frac_bits, float clip,
                               const uint8_t *d_candidates, int attempts, uint64_t max_sumsq, uint64_t *d_sumsq,
                               uint8_t *d_dither, uint32_t *d_chosen, hipStream_t stream) {
    const uint64_t tiles = float_tiles(L);
    if (N < 1 || tiles == 0 || tiles > 0x7fffffffull / (uint64_t)N || attempts < 1 || attempts > 8 || frac_bits < 0 ||
        frac_bits > 30)
        return hipErrorInvalidValue;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(d_sumsq);
    hipLaunchKernelGGL(round_sumsq_kernel, dim3((unsigned)(tiles * (uint64_t)N)), dim3(256), 0, stream, d_x, x_pitch, L,
                       (uint32_t)tiles, d_candidates, attempts, clip, (float)(1u << frac_bits), sums);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(round_select_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, stream, sums, d_candidates, N,
                       attempts, (unsigned long long)max_sumsq, d_dither, d_chosen);
    return hipGetLastError();
}

// Workgroups of the seed-schedule launch: one per 256 seeds, more when it also zero-fills
// (about 16 KiB per workgroup, at most 1024).  meta needs 2 + 2 * this many words.
int seed_schedule_groups(int K, uint64_t zero_n) {
    const uint64_t g = (uint64_t)((K + 255) / 256 > 0 ? (K + 255) / 256 : 1);
    const uint64_t z = std::min<uint64_t>(1024, (zero_n + 4095) / 4096);
    return (int)std::max(g, z);
}

hipError_t launch_seed_schedule(const uint8_t *d_seeds, const int8_t *d_signs, int K, SeedRec *d_recs,
                                uint32_t *d_meta, hipStream_t stream, uint32_t *d_zero, uint64_t zero_n) {
    const unsigned grid = (unsigned)seed_schedule_groups(K, d_zero ? zero_n : 0);
    hipLaunchKernelGGL(seed_schedule_kernel, dim3(grid), dim3(256), 0, stream, d_seeds, d_signs, K, d_recs, d_meta,
                       d_zero, d_zero ? zero_n : 0);
    return hipGetLastError();
}

template <int S, bool BL, bool MERGED, int WPE, int RUM = 2, int AUX = 0, bool SPREAD = false>
static void launch_items_t(const Item *d_items, int n_items, const uint32_t *d_rows, uint64_t row_pitch,
                           const SeedRec *d_recs, const uint32_t *d_meta, uint32_t *d_out, hipStream_t stream) {
    hipLaunchKernelGGL((items_kernel<S, BL, MERGED, WPE, RUM, AUX, SPREAD>), dim3(n_items), dim3(kThreads), 0, stream, d_items, d_rows,
                       row_pitch, d_recs, d_meta, d_out);
}

hipError_t launch_items(int subtiles, int variant, const Item *d_items, int n_items, const uint32_t *d_rows,
                        uint64_t row_pitch, const SeedRec *d_recs, const uint32_t *d_meta, uint32_t *d_out,
                        hipStream_t stream) {
    if (n_items <= 0) return hipSuccess;
#define FLM_L(S, BL, MG, W, ...) \
    launch_items_t<S, BL, MG, W, ##__VA_ARGS__>(d_items, n_items, d_rows, row_pitch, d_recs, d_meta, d_out, stream)
#define FLM_V(S)                                                     \
    switch (variant) {                                               \
        case kVarCoalesced: FLM_L(S, false, false, 4); break;        \
        case kVarBlock: FLM_L(S, true, false, 4); break;             \
        case kVarMerged: FLM_L(S, true, true, 4, 2, 0); break;           \
        case kVarMergedW8: FLM_L(S, true, true, 8); break;           \
        case kVarMergedRU4: FLM_L(S, true, true, 4, 4, 0); break;    \
        case kVarMergedNT: FLM_L(S, true, true, 4, 2, 2); break;     \
        case kVarMergedRU4NT: FLM_L(S, true, true, 4, 4, 2); break;  \
        case kVarMergedSpread: FLM_L(S, true, true, 4, 2, 0, true); break; \
        case kVarBlockSpread: FLM_L(S, true, false, 4, 2, 0, true); break; \
        default: return hipErrorInvalidValue;                        \
    }
    switch (subtiles) {
        case 1: FLM_V(1) break;
        case 4: FLM_V(4) break;
        case 16: FLM_V(16) break;
        default: return hipErrorInvalidValue;
    }
#undef FLM_V
#undef FLM_L
    return hipGetLastError();
}

int small_round_slots(int B) { return 16 * B; }

hipError_t launch_small_round(int B, const uint32_t *d_rows, uint64_t pitch, int N, const uint8_t *d_seeds,
                              const int8_t *d_signs, int K, uint64_t L, uint64_t mask_lo, uint64_t mask_hi,
                              uint32_t ctr0, uint32_t *d_out, uint32_t *d_meta, hipStream_t stream) {
    const uint64_t T = (uint64_t)small_round_slots(B);
    const unsigned grid = (unsigned)((L + T - 1) / T);
    switch (B) {
        case 1: hipLaunchKernelGGL(small_round_kernel<1>, dim3(grid), dim3(256), 0, stream, d_rows, pitch, N, d_seeds,
                                   d_signs, K, L, mask_lo, mask_hi, ctr0, d_out, d_meta); break;
        case 2: hipLaunchKernelGGL(small_round_kernel<2>, dim3(grid), dim3(256), 0, stream, d_rows, pitch, N, d_seeds,
                                   d_signs, K, L, mask_lo, mask_hi, ctr0, d_out, d_meta); break;
        case 4: hipLaunchKernelGGL(small_round_kernel<4>, dim3(grid), dim3(256), 0, stream, d_rows, pitch, N, d_seeds,
                                   d_signs, K, L, mask_lo, mask_hi, ctr0, d_out, d_meta); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_small_client_mask(const uint32_t *d_x, uint64_t pitch, int N, const int64_t *d_seg,
                                   const uint8_t *d_seeds, const int8_t *d_signs, uint64_t L, uint32_t bias,
                                   uint32_t *d_out, hipStream_t stream) {
    constexpr int B = 16;  // 256-slot tiles: 4 seeds x 16 blocks per wave, 16 seeds per pass
    const dim3 grid((unsigned)((L + 16 * B - 1) / (16 * B)), (unsigned)N);
    hipLaunchKernelGGL((small_round_kernel<B, true>), grid, dim3(256), 0, stream, d_x, pitch, 0, d_seeds, d_signs, 0,
                       L, (uint64_t)0, L, 0u, d_out, (uint32_t *)nullptr, d_seg, bias);
    return hipGetLastError();
}

uint32_t pair_units_count(int K, uint64_t L, uint32_t *n_tiles) {
    const uint64_t t = (L + 1023) / 1024, c = (uint64_t)((K + kUnitSeeds - 1) / kUnitSeeds);
    if (n_tiles) *n_tiles = (uint32_t)t;
    const uint64_t n = t * c;
    return n > 0xF0000000ull ? 0xFFFFFFFFu : (uint32_t)n;  // caller rejects the sentinel
}

hipError_t launch_pair_units(bool side, const SeedRec *d_recs, int K, uint32_t *d_dst, uint64_t L, uint32_t *d_ws,
                             int groups, hipStream_t stream) {
    uint32_t n_tiles = 0;
    const uint32_t n_units = pair_units_count(K, L, &n_tiles);
    if (n_units == 0 || groups <= 0) return hipSuccess;
    if (side)
        hipLaunchKernelGGL(pair_units_kernel<true>, dim3(groups), dim3(64), 0, stream, d_recs, K, d_dst, L, n_tiles,
                           n_units, d_ws);
    else
        hipLaunchKernelGGL(pair_units_kernel<false>, dim3(groups), dim3(64), 0, stream, d_recs, K, d_dst, L, n_tiles,
                           n_units, d_ws);
    return hipGetLastError();
}

hipError_t launch_prg_expand(const SeedRec *d_recs, int K, uint64_t L, uint64_t pitch, uint32_t ctr0,
                             uint32_t *d_out, int groups, hipStream_t stream) {
    const uint64_t chunks = (L + 1023) / 1024, units = chunks * (uint64_t)K;
    if (K <= 0 || L == 0) return hipSuccess;
    if (units > 0xFFFFFFFFull || groups <= 0) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<uint64_t>(units, (uint64_t)groups);
    hipLaunchKernelGGL(prg_expand_kernel, dim3(grid), dim3(64), 0, stream, d_recs, (uint32_t)chunks, (uint32_t)units,
                       L, pitch, ctr0, d_out);
    return hipGetLastError();
}

hipError_t launch_flag_set(uint32_t *d_ws, hipStream_t stream) {
    hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(64), 0, stream, d_ws);
    return hipGetLastError();
}

hipError_t launch_add2(const uint32_t *d_a, const uint32_t *d_b, uint32_t *d_dst, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t g = std::min<uint64_t>(2048, (n / 4 + 255) / 256 + 1);
    hipLaunchKernelGGL(add2_kernel, dim3((unsigned)g), dim3(256), 0, stream, d_a, d_b, d_dst, n);
    return hipGetLastError();
}

hipError_t launch_shard_sum(const uint32_t *const *d_parts, int G, uint64_t lo, uint64_t n, uint32_t *d_dst,
                            hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (G < 1 || G > kMaxParts) return hipErrorInvalidValue;
    PartPtrs pp{};
    for (int g = 0; g < G; ++g) pp.p[g] = d_parts[g];
    const uint64_t grid = std::min<uint64_t>(2048, (n / 4 + 255) / 256 + 1);
    hipLaunchKernelGGL(shard_sum_kernel, dim3((unsigned)grid), dim3(256), 0, stream, pp, G, lo, n, d_dst);
    return hipGetLastError();
}

hipError_t launch_chacha20_xor(const uint32_t key[8], const uint32_t nonce[2], uint64_t counter,
                               const uint8_t *d_in, uint8_t *d_out, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 63) / 64;
    const unsigned grid = (unsigned)((blocks + 255) / 256);
    hipLaunchKernelGGL(chacha20_xor_kernel, dim3(grid), dim3(256), 0, stream, key[0], key[1], key[2], key[3],
                       key[4], key[5], key[6], key[7], nonce[0], nonce[1], counter, d_in, d_out, (uint64_t)n);
    return hipGetLastError();
}

}  // namespace flm

