// flm_internal.h -- the kernel launchers (flm_kernels.hip, flm_p256.hip) and the host-runtime hooks (flm::rt)
// that flm_runtime.hip shares with flm_comm.hip and flm_store.hip.  The records the launchers take (Item, SeedRec,
// ItemsVariant) are in the HIP-free flm_items.h, filled by flm_planner.h; the argument rules and array lists of the
// calls whose launchers are declared here (the round path's and the batch crypto calls') are in the HIP-free
// flm_call_args.h.  Not part of the public ABI.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <hip/hip_runtime.h>

#include "flm_host_layout.h"
#include "flm_items.h"

namespace flm {

// b"abcd" as a little-endian word (util/param.py:12).
constexpr uint32_t kAbcd = 0x64636261u;
// ChaCha20 "expand 32-byte k".
constexpr uint32_t kSigma0 = 0x61707865u, kSigma1 = 0x3320646eu, kSigma2 = 0x79622d32u,
                   kSigma3 = 0x6b206574u;

// Launchers (flm_kernels.hip).  All enqueue on `stream` and return hipError_t.
// d_zero (optional): zero-fill zero_n u32 words of the round's output in the same launch.
hipError_t launch_seed_schedule(const uint8_t *d_seeds, const int8_t *d_signs, int K, SeedRec *d_recs,
                                uint32_t *d_meta, hipStream_t stream, uint32_t *d_zero = nullptr,
                                uint64_t zero_n = 0);
int seed_schedule_groups(int K, uint64_t zero_n);
// subtiles: 1, 4 or 16 sub-tiles of 1024 slots per workgroup.
hipError_t launch_items(int subtiles, int variant, const Item *d_items, int n_items, const uint32_t *d_rows,
                        uint64_t row_pitch, const SeedRec *d_recs, const uint32_t *d_meta,
                        uint32_t *d_out, hipStream_t stream);
// One-launch round for small rounds (flm_kernels.hip small_round_kernel): a workgroup owns
// 16*B slots (B = 1, 2, 4), sums every row there and adds every seed's mask; meta gets the
// sign counts (one part).  mask_lo % 16 == 0 and (mask_hi % 16 == 0 or mask_hi == L).
int small_round_slots(int B);
hipError_t launch_small_round(int B, const uint32_t *d_rows, uint64_t pitch, int N, const uint8_t *d_seeds,
                              const int8_t *d_signs, int K, uint64_t L, uint64_t mask_lo, uint64_t mask_hi,
                              uint32_t ctr0, uint32_t *d_out, uint32_t *d_meta, hipStream_t stream);
// Client masking with the same kernel (SEG mode): grid (L/256, N), row i gets seeds
// [d_seg[i], d_seg[i+1]) on top of x row i (or the constant `bias` when d_x is NULL).
hipError_t launch_small_client_mask(const uint32_t *d_x, uint64_t pitch, int N, const int64_t *d_seg,
                                   const uint8_t *d_seeds, const int8_t *d_signs, uint64_t L, uint32_t bias,
                                   uint32_t *d_out, hipStream_t stream);
// Fixed-point codec (encode_mask_kernel, decode_sum_kernel, decode_unpack_kernel).  The codec's parameters as the
// rule of flm_call_args.h passed them: pack = 1, 2 or 4 parameters per ring word, noise_bits even in 0..1024 (0:
// no binomial noise), bias = ceil(clip 2^frac_bits), the codec's own (ignored at pack = 1).
struct CodecParams {
    int frac_bits;
    float clip;
    int pack, noise_bits;
    uint32_t bias;
};
// d_out[i][l'] = word l' of the encoded, packed and noised d_x[i] + client i's masks: L counts parameters, d_out rows
// hold ceil(L / pack) words, one workgroup per (client, 1024-word tile) of a one-dimensional grid
// (encode_mask_groups(N, ceil(L / pack)) of them, at most 2^31 - 1).  d_x rows are read 16 bytes at a time up to
// round_up(L, 4) floats; d_dither N x 32 selects stochastic rounding, NULL nearest-even; d_noise N x 32 bytes, read
// when noise_bits > 0; d_clipped N words, zeroed by the caller, or NULL.
uint64_t encode_mask_groups(int N, uint64_t L);
hipError_t launch_encode_mask(const float *d_x, uint64_t x_pitch, int N, const int64_t *d_seg, const uint8_t *d_seeds,
                              const int8_t *d_signs, const uint8_t *d_dither, const uint8_t *d_noise, uint64_t L,
                              const CodecParams &c, uint32_t *d_out, uint64_t out_pitch, uint32_t *d_clipped,
                              hipStream_t stream);
// launch_encode_mask with the noise of the table mode (encode_gauss_mask_kernel), tail in 1..512: d_noise N x 32 bytes
// and d_cdt 2 tail uint64 entries, 8-byte aligned, both read; c.noise_bits is not.  The launch asks 16 tail bytes of
// dynamic LDS for the table.
hipError_t launch_encode_gauss_mask(const float *d_x, uint64_t x_pitch, int N, const int64_t *d_seg, const uint8_t *d_seeds,
                                    const int8_t *d_signs, const uint8_t *d_dither, const uint8_t *d_noise,
                                    const uint64_t *d_cdt, int tail, uint64_t L, const CodecParams &c, uint32_t *d_out,
                                    uint64_t out_pitch, uint32_t *d_clipped, hipStream_t stream);
// d_out[l] = float32(float64(int32(d_sum[l])) / denom), l < n; d_out may be d_sum; both 16-byte aligned
hipError_t launch_decode_sum(const uint32_t *d_sum, uint64_t n, double denom, float *d_out, hipStream_t stream);
// d_out[pack l' + j] = float32(float64(field j of d_sum[l'] - count_bias) / denom) for the L parameters; d_out is
// not d_sum; both 16-byte aligned
hipError_t launch_decode_unpack(const uint32_t *d_sum, uint64_t L, int pack, int64_t count_bias, double denom, float *d_out,
                                hipStream_t stream);
// The same of a sum taken modulo the field (decode_unpack_mod_kernel): d_out[pack l' + j] = float32(float64(Qh_j) / denom),
// Qh_j the centred residue of the carry-aware cascade with count_bias = count B_n mod 2^32; guard in 1..2^(32/pack - 1);
// d_stats two words zeroed by the caller (the kernel adds #{|Qh| >= guard} into [0] and takes max |Qh| into [1]), or NULL
hipError_t launch_decode_unpack_mod(const uint32_t *d_sum, uint64_t L, int pack, uint32_t count_bias, double denom,
                                    uint32_t guard, float *d_out, uint32_t *d_stats, hipStream_t stream);
// Randomised block Hadamard rotation (rotate_kernel): rows of L parameters taken as L_rot = round_up(L, 2^log2_block),
// log2_block in 4..12; forward reads L floats a row (up to round_up(L, 4) of them, 16 bytes at a time) and writes L_rot,
// inverse reads L_rot and writes L; d_sign_bits ceil(L_rot / 32) words; d_out may be d_x at equal pitches; d_nonfinite
// (forward only) N words, zeroed by the caller, or NULL.  One workgroup per (row, kFloatTile-parameter tile) of a
// one-dimensional grid (rotate_groups(N, L_rot) of them, at most 2^31 - 1).  d_factors NULL: the rotation alone; else
// (forward only, the inverse with factors is refused) the L2 clip's multiply rides in the load (rotate_kernel<false,
// PHASES, true>): every finite input times d_factors[row] first, everything else as without.
uint64_t rotate_groups(int N, uint64_t L_rot);
hipError_t launch_rotate(const float *d_x, uint64_t x_pitch, int N, uint64_t L, uint64_t L_rot, int log2_block,
                         const uint32_t *d_sign_bits, bool inverse, float *d_out, uint64_t out_pitch,
                         uint32_t *d_nonfinite, const float *d_factors, hipStream_t stream);
// L2 clip (l2_sumsq_kernel, l2_factor_kernel, scale_rows_kernel): rows of L > 0 floats, read through the rotation's
// own row read.  launch_l2_factors: d_work N l2_tiles(L) doubles (one partial per tile, written then read),
// d_factors N floats, d_sumsq N doubles or NULL; two launches.  launch_scale_rows: d_out = d_x d_factors[row], d_out
// may be d_x at equal pitches.  One workgroup per (row, tile), at most 2^31 - 1 of them.
uint64_t l2_tiles(uint64_t L);
hipError_t launch_l2_factors(const float *d_x, uint64_t x_pitch, int N, uint64_t L, float clip_norm, double *d_work,
                             float *d_factors, double *d_sumsq, hipStream_t stream);
hipError_t launch_scale_rows(const float *d_x, uint64_t x_pitch, int N, uint64_t L, const float *d_factors, float *d_out,
                             uint64_t out_pitch, hipStream_t stream);
// Conditional stochastic rounding (round_sumsq_kernel, round_select_kernel): d_sumsq[row A + a] += Q(candidate a of the
// row) over N rows of L > 0 floats (the caller zeroes d_sumsq on the stream first), then d_chosen and d_dither from
// them; two launches, one workgroup per (row, tile) and one thread per row.  A = attempts in 1..8.
hipError_t launch_round_select(const float *d_x, uint64_t x_pitch, int N, uint64_t L, int frac_bits, float clip,
                               const uint8_t *d_candidates, int attempts, uint64_t max_sumsq, uint64_t *d_sumsq,
                               uint8_t *d_dither, uint32_t *d_chosen, hipStream_t stream);
uint32_t pair_units_count(int K, uint64_t L, uint32_t *n_tiles);
hipError_t launch_pair_units(bool side, const SeedRec *d_recs, int K, uint32_t *d_dst, uint64_t L, uint32_t *d_ws,
                             int groups, hipStream_t stream);
hipError_t launch_flag_set(uint32_t *d_ws, hipStream_t stream);
// d_out[k * pitch + l] = PRG(seed k)[16 ctr0 + l], l < L, k < K (prg_expand_kernel): `groups` one-wave
// workgroups take contiguous runs of the K x ceil(L / 1024) seed-major units.
hipError_t launch_prg_expand(const SeedRec *d_recs, int K, uint64_t L, uint64_t pitch, uint32_t ctr0,
                             uint32_t *d_out, int groups, hipStream_t stream);
hipError_t launch_add2(const uint32_t *d_a, const uint32_t *d_b, uint32_t *d_dst, uint64_t n, hipStream_t stream);
// dst[l] = sum_{g<G} d_parts[g][lo + l], l < n (G <= kMaxParts, all on the launching device).
constexpr int kMaxParts = 16;
struct PartPtrs {
    const uint32_t *p[kMaxParts];
};
hipError_t launch_shard_sum(const uint32_t *const *d_parts, int G, uint64_t lo, uint64_t n, uint32_t *d_dst,
                            hipStream_t stream);
hipError_t launch_chacha20_xor(const uint32_t key[8], const uint32_t nonce[2], uint64_t counter,
                               const uint8_t *d_in, uint8_t *d_out, size_t n, hipStream_t stream);

// P-256 (flm_p256.hip: the launchers and kernels; its device layers are the flm_fe256.h,
// flm_jac256.h, flm_sha256.h and flm_aes128.h headers it alone includes). d_jac holds T*D Jacobian results as SoA planes [T][24][D].
hipError_t launch_ec_mul(const uint8_t *d_points, const uint8_t *d_scalars, int per_element, int T, int D,
                         uint32_t *d_jac, uint32_t *d_flags, hipStream_t stream, int threads, int waves,
                         int coop = 0, int terms = 1, unsigned lds_pad = 0);
// Partial sums the combine's ec_mul leaves per element: T, or ceil(T / terms) with Straus lanes.
int ec_mul_groups(int T, int terms);
hipError_t launch_shamir_combine(const uint8_t *d_shares, const uint8_t *d_lambdas, int T, int M, uint8_t *d_out,
                                 hipStream_t stream);
// d_out[c][i] = sum_j d_coeffs[j][i] xs[c]^j mod n (shamir_deal_kernel): coeffs T x M x 32, out C x M x 32
hipError_t launch_shamir_deal(const uint8_t *d_coeffs, int T, int M, const uint32_t *d_xs, int C, uint8_t *d_out,
                              hipStream_t stream);
// d_out = d_in ^ AES-128-GCM keystream of (key i, nonce i), n messages of len bytes (aes_gcm_xor_kernel)
hipError_t launch_aes_gcm_xor(const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len, const uint8_t *d_in,
                              uint8_t *d_out, uint32_t len, int n, hipStream_t stream);
// AES-128-GCM with its tag, n messages of len bytes under aad_len bytes of AAD each (aes_gcm_auth_kernel):
// seal writes d_out and d_tags (n x 16); open checks d_tags, writes d_ok (n) and the plaintext, or zero
// bytes where the tag is wrong.  d_aad is unread when aad_len is 0, d_in and d_out when len is 0.
hipError_t launch_aes_gcm_seal(const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len, const uint8_t *d_aad,
                               uint32_t aad_len, const uint8_t *d_in, uint8_t *d_out, uint32_t len, uint8_t *d_tags,
                               int n, hipStream_t stream);
hipError_t launch_aes_gcm_open(const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len, const uint8_t *d_aad,
                               uint32_t aad_len, const uint8_t *d_in, const uint8_t *d_tags, uint8_t *d_out,
                               uint32_t len, uint8_t *d_ok, int n, hipStream_t stream);
// d_ok[i] = ECDSA verdict of (pubkey i, digest i, signature i); d_flags n words or NULL (ecdsa_verify_kernel)
hipError_t launch_ecdsa_verify(const uint8_t *d_pubkeys, const uint8_t *d_digests, const uint8_t *d_sigs, int n,
                               uint8_t *d_ok, uint32_t *d_flags, hipStream_t stream);
// d_ok[i] = whether shares[i] G equals dealer row i's committed polynomial at xs[i] (feldman_verify_kernel);
// d_commitments T x M x 64 term-major, d_dealer n indices < M or NULL (row i: dealer i % M), x_bits 1..32;
// d_points (n x 64, that polynomial's point) and d_flags (n words) may be NULL
hipError_t launch_feldman_verify(const uint8_t *d_commitments, int T, int M, const uint32_t *d_dealer,
                                 const uint32_t *d_xs, int x_bits, const uint8_t *d_shares, int n, uint8_t *d_ok,
                                 uint8_t *d_points, uint32_t *d_flags, hipStream_t stream);
hipError_t launch_ec_finish(const uint8_t *d_base, const uint32_t *d_jac, int T, int D, int negate,
                            uint8_t *d_points_out, uint8_t *d_digests_out, uint32_t *d_flags, hipStream_t stream);
// hash_str_to_curve of n messages (d_msgs: n x 64 bytes + d_lens), or of the decimal strings of
// v0 .. v0+n-1 (d_msgs NULL); d_out n x 64 wire bytes, d_flags n words (written)
hipError_t launch_hash_to_curve(const uint8_t *d_msgs, const uint32_t *d_lens, uint32_t v0, int n, uint8_t *d_out,
                                uint32_t *d_flags, hipStream_t stream);
// the same kernel's tail (mod n, map_to_curve, Q_0 + Q_1) on d_uniform: n x 96 bytes in the place of
// expand_message_xmd's output (h2c_from_uniform_kernel)
hipError_t launch_h2c_from_uniform(const uint8_t *d_uniform, int n, uint8_t *d_out, uint32_t *d_flags,
                                   hipStream_t stream);

}  // namespace flm

// Host-runtime hooks shared by flm_runtime.hip and flm_comm.hip (not exported in the header).
struct flm_ctx;
namespace flm {
namespace rt {
int set_error(flm_ctx *ctx, int code, const char *msg);
int device_of(const flm_ctx *ctx);
hipStream_t stream_of(const flm_ctx *ctx);
void **comm_slot(flm_ctx *ctx);
// n bytes between host buffers on the context's copy threads (the CPU side of a pinned-buffer copy)
void host_copy(flm_ctx *ctx, void *dst, const void *src, size_t n);
// The calling thread's current device belongs to the caller: every entry point that selects a
// device (its context's, or each rank's of a group or store) gives the caller's back on return.
// torch and the agents' own HIP code allocate on the current device, and a group call that left
// it on its last rank's GPU would move them there.  set() switches only when needed (hipGetDevice
// is a thread-local read), so a call on the caller's own device costs no hipSetDevice at all.
struct DeviceScope {
    int old = -1;
    DeviceScope() {
        if (hipGetDevice(&old) != hipSuccess) old = -1;
    }
    explicit DeviceScope(int want) : DeviceScope() { (void)set(want); }
    hipError_t set(int want) {
        int now = -1;
        if (hipGetDevice(&now) == hipSuccess && now == want) return hipSuccess;
        return hipSetDevice(want);
    }
    ~DeviceScope() {
        int now = -1;
        if (old >= 0 && hipGetDevice(&now) == hipSuccess && now != old) (void)hipSetDevice(old);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};
// Size of a scratch allocation that must hold `bytes`: half again as much, at most 64 MiB extra,
// in whole 4 KiB pages.  Buffers sized by per-round counts (K seeds, D pairs) change by a few
// percent from round to round; allocating exactly made every new maximum a hipFree + hipMalloc,
// and hipFree waits for the whole device (4.8 ms inside the server's unmask, profiles/r05_hip_api_top.txt).
inline size_t grow_bytes(size_t bytes) {
    const size_t slack = bytes / 2 < (size_t(64) << 20) ? bytes / 2 : (size_t(64) << 20);
    return (bytes + slack + 4095) & ~size_t(4095);
}
// Upload host rows and seeds and enqueue the fused round over mask window [mask_lo, mask_hi) into
// d_out (L words) on the context's stream; returns without synchronising.
int host_round_async(flm_ctx *ctx, const uint32_t *const *rows, int N, const uint8_t *seeds, const int8_t *signs,
                     int K, size_t L, size_t mask_lo, size_t mask_hi, uint32_t *d_out);
}  // namespace rt
void comm_release(flm_ctx *ctx);  // flm_comm.hip: drop the context's communicator (flm_free)
// flm_comm.hip: synchronise every device, finalize a one-thread clique's members in one RCCL group,
// then destroy them (flm_group_free)
void comm_release_clique(flm_ctx *const *ctxs, int n);
}  // namespace flm
// The host-copy layout (flm_host_layout.h) of n spans, for the CPU tests: no context, no HIP call.
// route, pitch and offset get n entries each, *total the bounce bytes.
extern "C" int flm_host_layout(int n, const uint64_t *width, const uint64_t *rows, const int *may_in_place,
                               int *route, uint64_t *pitch, uint64_t *offset, uint64_t *total);
// Hash to curve from the uniform bytes on, for the GPU tests: uniform is n x 96 bytes (big endian, what
// expand_message_xmd(msg, DST, 96) gives), out n x 64 wire bytes, flags_out n words or NULL; host
// pointers, with flm_hash_to_curve's conventions (infinity is a result: flags bit 2 and zero bytes).
extern "C" int flm_h2c_from_uniform(flm_ctx *ctx, const uint8_t *uniform, int n, uint8_t *out, uint32_t *flags_out);
