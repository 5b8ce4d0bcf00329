// flm_call_args.h -- the calls of flm_runtime.hip that come in a host-pointer and a *_dev form: the round
// path (client masking with and without the codec, decode, PRG expansion, mask accumulation, the round
// itself, ChaCha20) and the batch crypto calls (P-256, Shamir, AES-GCM, ECDSA, Feldman, hash to curve).
// Their argument rules, and per call the one ordered list of the arrays its host-pointer form moves --
// width, rows and pitches, direction, whether it may run in place, which of the context's scratch
// buffers it lands in, whether it is there at all.  HostCopies::declare takes that list, and so does
// tools/args_check.cpp: plain C++ with no HIP in it, like flm_host_layout.h, so the rules and the
// lists the runtime uses are the ones checked on the CPU under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <initializer_list>

#include "flm_planner.h"

namespace flm {
namespace rt __attribute__((visibility("hidden"))) {  // the library exports nothing of this header

constexpr size_t kMaxRows = size_t(1) << 26;  // lanes (rows, shares, coefficients, commitments) per call
constexpr size_t kAesMaxLen = 256;            // bytes per message
constexpr size_t kAesMaxAad = 64;             // bytes of AAD per message

constexpr uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

// ------------------------------------------------------------------ the round path's rules
// each *_error: nullptr when the call may run, else what is wrong -- one text per mistake, whichever
// form of the call meets it.  FLM_EINVAL unless the rule says FLM_ERANGE.

inline const char *signs_error(const int8_t *signs, int64_t K) {
    for (int64_t k = 0; k < K; ++k)
        if (signs[k] != 1 && signs[k] != -1) return "signs must be +1 or -1";
    return nullptr;
}

// Client i's seeds are seeds[seg[i] .. seg[i + 1]): seg[0] = 0, non-decreasing (a decreasing pair would
// wrap a seed count and read past the table), K = seg[N] <= 2^31 - 1 seeds, each with a sign of +1 or -1.
inline const char *seg_signs_error(int N, const int64_t *seg, const int8_t *signs, int64_t *K_out) {
    if (!seg) return "NULL argument";
    if (seg[0] != 0) return "seg[0] must be 0";
    for (int i = 0; i < N; ++i)
        if (seg[i + 1] < seg[i]) return "seg must be non-decreasing";
    const int64_t K = seg[N];
    if (K > 0x7fffffff) return "too many seeds";
    if (K > 0 && !signs) return "NULL seeds/signs";
    *K_out = K;
    return signs_error(signs, K);
}

// flm_client_mask[_dev], flm_client_encode_mask[_dev]: the arrays either form needs.  rows_given: out, and x
// where the call cannot do without it.
inline const char *client_args_error(bool rows_given, int N, const int64_t *seg, const void *seeds, const int8_t *signs,
                                     int64_t *K_out) {
    if (!rows_given) return "NULL argument";
    if (const char *why = seg_signs_error(N, seg, signs, K_out)) return why;
    return *K_out > 0 && !seeds ? "NULL seeds/signs" : nullptr;
}

// rows of L words `pitch` words apart, read and written four words at a time
inline const char *row_pitch_error(size_t pitch, size_t L) {
    return pitch % 4 || pitch < round_up(L, 4) ? "pitch must be a multiple of 4 and >= round_up(L, 4)" : nullptr;
}

// the kernels' 16-byte accesses: every device pointer given (NULL passes: an absent array)
inline const char *align16_error(std::initializer_list<const void *> dev) {
    uintptr_t all = 0;
    for (const void *p : dev) all |= (uintptr_t)p;
    return all & 15 ? "device arrays must be 16-byte aligned" : nullptr;
}
// the L2 clip's smaller accesses (NULL passes): the factors of a call, 4 bytes each ...
inline const char *align4_error(const void *factors) {
    return (uintptr_t)factors & 3 ? "factors must be 4-byte aligned" : nullptr;
}
// ... and, in the call that also takes doubles, those at 8 bytes: one text for the three arrays
inline const char *l2_factors_align_error(const void *work, const void *sumsq, const void *factors) {
    return (((uintptr_t)work | (uintptr_t)sumsq) & 7) || align4_error(factors)
               ? "work and sumsq must be 8-byte aligned, factors 4-byte aligned" : nullptr;
}

inline const char *frac_bits_error(int frac_bits) {
    return frac_bits < 0 || frac_bits > 30 ? "frac_bits outside 0..30" : nullptr;
}

// The codec's one rule.  pack = 1, 2 or 4 fields of W = 32 / pack bits per ring word (unpacked_ok: whether the
// entry point admits pack = 1), each client adding binomial noise Z in [-b/2, b/2], b = noise_bits even in 0..1024
// (0: off).  B = ceil(clip 2^f): clip 2^f is exact in double (a float times a power of two), so is its ceiling,
// and every product is compared in integers.  Headroom for n contributors (FLM_ERANGE, *range set):
//   n B <= 2^31 - 1, whatever the pack;
//   packed, fields hold q + B in [0, 2B]: n 2B <= 2^W - 1, so that no field of the sum carries into its neighbour;
//   with noise, B_n = B + b/2 in B's place in the rule of that pack;
//   with noise and a row of L_params > 0 parameters: ceil(b / 32) ceil(L_params / 16) <= 2^32 blocks of the noise
//   stream, whose block counter has no high word.
// *bias: B, the codec's own; *bias_n: B_n (either may be NULL).
inline const char *codec_error(int frac_bits, float clip, int pack, bool unpacked_ok, int noise_bits, int64_t n,
                               uint64_t L_params, bool *range, uint32_t *bias = nullptr, uint32_t *bias_n = nullptr) {
    *range = false;
    if (pack != 2 && pack != 4 && !(unpacked_ok && pack == 1)) return unpacked_ok ? "pack must be 1, 2 or 4" : "pack must be 2 or 4";
    if (noise_bits < 0 || noise_bits > 1024 || noise_bits % 2) return "noise_bits must be even and in 0..1024";
    if (const char *why = frac_bits_error(frac_bits)) return why;
    if (!(clip > 0.0f) || !std::isfinite(clip)) return "clip must be finite and positive";
    if (n < 1) return "a count of contributors must be at least 1";
    *range = true;  // from here on the parameters are fine and the sum is what can wrap
    const double m = std::ceil((double)clip * std::ldexp(1.0, frac_bits));  // >= 1: clip > 0
    if (m > 2147483647.0 || (uint64_t)n > 2147483647ull / (uint64_t)m)
        return "that many contributors of magnitude up to ceil(clip 2^frac_bits) can wrap the 32-bit sum";
    const uint64_t B = (uint64_t)m, Bn = B + (uint64_t)noise_bits / 2;
    const uint64_t top = pack == 1 ? 2147483647ull : (uint64_t(1) << (32 / pack)) - 1;
    if (pack > 1 && (2 * B > top || (uint64_t)n > top / (2 * B)))
        return "that many contributors of fields up to 2 ceil(clip 2^frac_bits) can carry out of a packed field";
    if (bias) *bias = (uint32_t)B;
    if (bias_n) *bias_n = (uint32_t)Bn;
    if (noise_bits != 0) {
        const uint64_t each = pack == 1 ? Bn : 2 * Bn;
        if (each > top || (uint64_t)n > top / each)
            return "that many contributors of magnitude up to ceil(clip 2^frac_bits) + noise_bits / 2 have no headroom";
        const uint64_t draws = ((uint64_t)noise_bits + 31) / 32, blocks = L_params / 16 + (L_params % 16 ? 1 : 0);
        if (blocks > (uint64_t(1) << 32) / draws)  // draws blocks <= 2^32, without overflow
            return "the noise stream of a row that long ends beyond 2^32 blocks (its block counter has no high word)";
    }
    *range = false;
    return nullptr;
}

// flm_codec_check_modular, flm_decode_unpack_mod[_dev], flm_store_unmask_unpack_mod_f32: the packed codec's rule for a
// sum decoded modulo the field, where carries between the fields are followed instead of excluded.  The codec's own
// refusals (pack 2 or 4 only, noise_bits, frac_bits, clip, n >= 1), then, FLM_ERANGE (*range set): one contributor's
// field must fit, 2 B_n <= 2^W - 1, which is the codec's rule at n = 1, and n <= 2^31 - 1.  Nothing bounds n B_n: the
// decode takes it mod 2^32.  *bias_n: B_n = B + noise_bits / 2 (the table mode passes noise_bits = 2 tail).
inline const char *modular_error(int frac_bits, float clip, int pack, int noise_bits, int64_t n, bool *range,
                                 uint32_t *bias_n = nullptr) {
    if (const char *why = codec_error(frac_bits, clip, pack, false, noise_bits, n < 1 ? n : 1, 0, range, nullptr, bias_n))
        return why;
    if (n > 2147483647ll) return *range = true, "a count of contributors must be at most 2^31 - 1";
    return nullptr;
}
// ... and the decode's own: guard in 1..H = 2^(W - 1) (FLM_EINVAL; pack already 2 or 4), L <= 2^32 - 1 parameters
// (FLM_ERANGE, *range set: the near count is a 32-bit word)
inline const char *modular_decode_error(int pack, int64_t guard, uint64_t L, bool *range) {
    *range = false;
    if (guard < 1 || guard > (int64_t(1) << (32 / pack - 1))) return "guard must be in 1..2^(32 / pack - 1)";
    if (L > 0xFFFFFFFFull) return *range = true, "the near count of that many parameters does not fit 32 bits";
    return nullptr;
}
// d_out may not alias d_sum: the ceil(L / pack) words and the L floats are disjoint ranges
inline const char *modular_alias_error(const void *d_sum, const void *d_out, uint64_t L, int pack) {
    const uintptr_t s = (uintptr_t)d_sum, o = (uintptr_t)d_out;
    const uint64_t Lw = (L + (uint64_t)pack - 1) / (uint64_t)pack;
    return s < o + 4 * L && o < s + 4 * Lw ? "out must not overlap sum" : nullptr;
}

// flm_codec_check_gauss, flm_client_encode_gauss_mask[_dev]: the codec's rule with the table mode of the noise, each
// client adding Z in [-tail, tail] sampled from a cumulative table of T = 2 tail entries.  tail in 1..512 (the table is
// at most 8 KiB, and 2 tail <= 1024 is a noise_bits the decodes accept); tail = 0 is not "off": the calls without noise
// exist.  Then the codec's own rule at any pack, and, FLM_ERANGE (*range set): headroom with B_n = B + tail in B's place
// (unpacked n B_n <= 2^31 - 1, packed n 2 B_n <= 2^W - 1); for a row of L_params > 0 parameters 2 ceil(L_params / 16)
// <= 2^32 blocks of the noise stream (two per parameter block), whose block counter has no high word.
inline const char *codec_gauss_error(int frac_bits, float clip, int pack, int tail, int64_t n, uint64_t L_params, bool *range,
                                     uint32_t *bias = nullptr, uint32_t *bias_n = nullptr) {
    *range = false;
    if (tail < 1 || tail > 512) return "tail must be in 1..512";
    uint32_t B = 0;
    if (const char *why = codec_error(frac_bits, clip, pack, true, 0, n, 0, range, &B)) return why;
    *range = true;
    const uint64_t Bn = (uint64_t)B + (uint64_t)tail, each = pack == 1 ? Bn : 2 * Bn;
    const uint64_t top = pack == 1 ? 2147483647ull : (uint64_t(1) << (32 / pack)) - 1;
    if (each > top || (uint64_t)n > top / each)
        return "that many contributors of magnitude up to ceil(clip 2^frac_bits) + tail have no headroom";
    if (L_params / 16 + (L_params % 16 ? 1 : 0) > (uint64_t(1) << 31))
        return "the noise stream of a row that long ends beyond 2^32 blocks (its block counter has no high word)";
    *range = false;
    if (bias) *bias = B;
    if (bias_n) *bias_n = (uint32_t)Bn;
    return nullptr;
}
// flm_dgauss_check_table, and the host form of the call: T = 2 tail entries that never decrease.  (The device form
// cannot see its table: whatever it holds, the kernel's count stays in [0, T] and no field leaves its headroom.)
inline const char *dgauss_table_error(const uint64_t *cdt, int tail) {
    if (!cdt) return "NULL argument";
    if (tail < 1 || tail > 512) return "tail must be in 1..512";
    for (int j = 1; j < 2 * tail; ++j)
        if (cdt[j] < cdt[j - 1]) return "the table must be non-decreasing";
    return nullptr;
}
// the kernel copies the table to LDS with 8-byte loads (NULL passes: refused as an absent array)
inline const char *cdt_align_error(const void *d_cdt) {
    return (uintptr_t)d_cdt & 7 ? "cdt must be 8-byte aligned" : nullptr;
}

// words of a row of L parameters
constexpr size_t packed_words(size_t L, int pack) { return (L + (size_t)pack - 1) / (size_t)pack; }

// flm_decode_sum[_dev], flm_store_unmask_f32: the mean over `count` contributors at frac_bits
inline const char *decode_error(int frac_bits, int64_t count) {
    if (const char *why = frac_bits_error(frac_bits)) return why;
    return count < 1 ? "count must be at least 1" : nullptr;
}

// a PRG window starts on a ChaCha block ...
inline const char *slot0_error(uint64_t slot0) { return slot0 % 16 ? "slot0 must be a multiple of 16" : nullptr; }
// ... and ends at or below 2^36 (flm::plan::slot_range_ok): FLM_ERANGE
inline const char *slot_range_error(uint64_t slot0, uint64_t n) {
    return flm::plan::slot_range_ok(slot0, n) ? nullptr
                                              : "PRG slots end beyond 2^36 (block counter high word must stay 0)";
}

// flm_prg_expand[_dev]
inline const char *prg_expand_error(const void *seeds, const void *out, uint64_t slot0) {
    return !seeds || !out ? "NULL argument" : slot0_error(slot0);
}

// the launch sizes: encode_mask_kernel's one-dimensional grid of flm::encode_mask_groups workgroups ...
inline const char *encode_mask_launch_error(uint64_t groups) {
    return groups > 0x7fffffffull ? "more than 2^31 - 1 1024-slot tiles" : nullptr;
}
// ... and prg_expand_kernel's 32-bit unit counter
inline uint64_t prg_expand_units(int K, size_t L) { return (uint64_t)K * ((L + 1023) / 1024); }
inline const char *prg_expand_launch_error(int K, size_t L) {
    return prg_expand_units(K, L) > 0xFFFFFFFFull ? "more than 2^32 1024-slot units" : nullptr;
}

// flm_rotate_check, flm_rotate[_dev]: the randomised block Hadamard rotation's one rule.  Blocks of H = 2^log2_block
// parameters, log2_block in 4..12 (a 4096-parameter tile of rotate_kernel holds whole blocks; below 16 a thread's 16
// parameters would span blocks); a row of L > 0 parameters counts as *L_rot = round_up(L, H).  The sign of parameter l
// is bit l % 32 of word l / 32 of PRG(key): L_rot / 32 words (rounded up) that must end at or below the PRG's 2^36
// slots, else FLM_ERANGE (*range set) -- which also keeps round_up from wrapping.
inline const char *rotate_error(uint64_t L, int log2_block, bool *range, uint64_t *L_rot) {
    *range = false;
    if (log2_block < 4 || log2_block > 12) return "log2_block outside 4..12";
    if (L == 0) return "a row of no parameters";
    *range = true;
    if (L > (uint64_t(1) << 41) || !flm::plan::slot_range_ok(0, round_up(round_up(L, uint64_t(1) << log2_block), 32) / 32))
        return "the sign stream of a row that long ends beyond 2^36 PRG slots";
    *range = false;
    *L_rot = round_up(L, uint64_t(1) << log2_block);
    return nullptr;
}
// words of sign stream for a rotated row
constexpr uint64_t rotate_sign_words(uint64_t L_rot) { return (L_rot + 31) / 32; }
// rotate_kernel's, and the L2 kernels', one-dimensional grid of a workgroup per (row, tile)
static_assert(flm::kFloatTile == 4096, "the text below names the tile");
constexpr const char *kTooManyFloatTiles = "more than 2^31 - 1 4096-parameter tiles";
inline const char *rotate_launch_error(uint64_t groups) { return groups > 0x7fffffffull ? kTooManyFloatTiles : nullptr; }

// flm_l2_clip_check, flm_l2_factors_dev, flm_scale_rows_dev, flm_l2_clip, flm_rotate_clip: the L2 clip's one rule.
// N >= 1 rows of L > 0 parameters, a clip radius that is finite and positive; one workgroup per (row, 4096-parameter
// tile) of a one-dimensional grid, so N ceil(L / 4096) <= 2^31 - 1, else FLM_ERANGE (*range set).  *work_doubles: the
// tile partials of a call, N ceil(L / 4096).
inline const char *l2_clip_error(uint64_t L, float clip_norm, int N, bool *range, uint64_t *work_doubles) {
    *range = false;
    if (L == 0) return "a row of no parameters";
    if (N < 1) return "N must be at least 1";
    if (!(clip_norm > 0.0f) || !std::isfinite(clip_norm)) return "clip_norm must be finite and positive";
    const uint64_t tiles = flm::float_tiles(L);
    *range = tiles > 0x7fffffffull / (uint64_t)N;
    if (*range) return kTooManyFloatTiles;
    *work_doubles = (uint64_t)N * tiles;
    return nullptr;
}

// flm_round_check, flm_round_select[_dev]: conditional stochastic rounding's one rule.  A row of L > 0 parameters,
// `attempts` candidate dither seeds in 1..8, the codec's own rule at pack = 1 with n = 1 (its code: FLM_ERANGE when
// ceil(clip 2^f) alone passes 2^31 - 1).  Then, FLM_ERANGE (*range set): Q = sum q^2 <= L B^2 must fit a uint64,
// B = ceil(clip 2^f) as the codec computes it; and ceil(L / 16) <= 2^32 blocks of the dither stream, whose block
// counter has no high word.
inline const char *round_error(uint64_t L, int frac_bits, float clip, int attempts, bool *range) {
    *range = false;
    if (L == 0) return "a row of no parameters";
    if (attempts < 1 || attempts > 8) return "attempts outside 1..8";
    uint32_t B = 0;
    if (const char *why = codec_error(frac_bits, clip, 1, true, 0, 1, 0, range, &B)) return why;
    *range = true;
    if (L > ~uint64_t(0) / ((uint64_t)B * (uint64_t)B))  // B >= 1, B^2 < 2^62
        return "that many squares of up to ceil(clip 2^frac_bits)^2 can wrap the 64-bit sum";
    if (L / 16 + (L % 16 ? 1 : 0) > (uint64_t(1) << 32))
        return "the dither stream of a row that long ends beyond 2^32 blocks (its block counter has no high word)";
    *range = false;
    return nullptr;
}
// round_sumsq_kernel's grid of a workgroup per (row, tile): FLM_ERANGE
inline const char *round_launch_error(int N, uint64_t L) {
    return N > 0 && flm::float_tiles(L) > 0x7fffffffull / (uint64_t)N ? kTooManyFloatTiles : nullptr;
}

// flm_round_bound: the bound on Q of conditional rounding (Kairouz et al., Algorithm 1), in float64 and in this order,
// every operation rounded on its own (no contraction): s = ((double)C 2^f) (1 + 2^-19), r = sqrt((double)d),
// b1 = (s + r) (s + r), b2 = (s s + (double)d 0.25) + tail (s + r 0.5), *max_sumsq = (uint64)floor(min(b1, b2)).
// No log, no exp: only sqrt, which IEEE rounds correctly.  FLM_ERANGE (*range set) for a result >= 2^63.
inline const char *round_bound_error(float clip_norm, int frac_bits, uint64_t d, double tail, bool *range, uint64_t *max_sumsq) {
#pragma clang fp contract(off)
    *range = false;
    if (!(clip_norm > 0.0f) || !std::isfinite(clip_norm)) return "clip_norm must be finite and positive";
    if (const char *why = frac_bits_error(frac_bits)) return why;
    if (d == 0) return "a row of no parameters";
    if (!(tail >= 0.0) || !std::isfinite(tail)) return "tail must be finite and not negative";
    const double s = ((double)clip_norm * std::ldexp(1.0, frac_bits)) * (1.0 + std::ldexp(1.0, -19));
    const double r = std::sqrt((double)d);
    const double b1 = (s + r) * (s + r);
    const double b2 = (s * s + (double)d * 0.25) + tail * (s + r * 0.5);
    const double b = std::floor(b1 < b2 ? b1 : b2);
    if (!(b < 9223372036854775808.0)) {
        *range = true;
        return "a bound of 2^63 or more";
    }
    *max_sumsq = (uint64_t)b;
    return nullptr;
}

// flm_aggregate_dev, flm_aggregate_unmask_dev: the rows, the mask window and its PRG slots, the output.
// *range: the refusal is the slot range's (FLM_ERANGE).
inline const char *aggregate_error(const void *d_rows, size_t row_pitch, int N, int K, size_t L, size_t mask_lo,
                                   size_t mask_hi, uint64_t prg_slot0, const void *d_out, bool *range) {
    *range = false;
    if (N < 0 || K < 0) return "negative N or K";
    if (N > 0)
        if (const char *why = row_pitch_error(row_pitch, L)) return why;
    if (const char *why = align16_error({N > 0 ? d_rows : nullptr, d_out})) return why;
    if (mask_hi > L || mask_lo > mask_hi) return "mask window outside [0, L)";
    if ((mask_hi > mask_lo && mask_lo % 16) || prg_slot0 % 16) return "mask_lo and prg_slot0 must be multiples of 16";
    if (const char *why = slot_range_error(prg_slot0, mask_hi)) return *range = true, why;
    return (N > 0 && !d_rows) || !d_out ? "NULL argument" : nullptr;
}

// ------------------------------------------------------------------ the batch crypto calls' rules
// each *_dims_error: nullptr when the call may run (a batch of 0 runs nothing), else what is wrong

inline const char *shamir_deal_dims_error(int T, int M, int C) {
    if (T < 1) return "T must be at least 1 (term 0 is the secret)";
    if (C < 1) return "C must be at least 1";
    if (M < 0) return "negative M";
    if ((size_t)T * (size_t)M > kMaxRows || (size_t)C * (size_t)M > kMaxRows) return "batch too large";
    return nullptr;
}

// index of the first zero among the C evaluation points, or -1 (f(0) is the secret itself)
inline int shamir_deal_zero_x(const uint32_t *xs, int C) {
    for (int c = 0; c < C; ++c)
        if (xs[c] == 0) return c;
    return -1;
}

inline const char *aes_gcm_dims_error(int nonce_len, size_t len, int n) {
    if (nonce_len != 12 && nonce_len != 16) return "nonce_len must be 12 or 16";
    if (len < 1 || len > kAesMaxLen) return "len must be in 1..256";
    if (n < 0) return "negative n";
    if ((size_t)n > kMaxRows) return "batch too large";
    return nullptr;
}

// flm_aes_gcm_seal / flm_aes_gcm_open: len 0 is a tag over the AAD alone
inline const char *aes_gcm_auth_dims_error(int nonce_len, size_t aad_len, size_t len, int n) {
    if (nonce_len != 12 && nonce_len != 16) return "nonce_len must be 12 or 16";
    if (len > kAesMaxLen) return "len must be in 0..256";
    if (aad_len > kAesMaxAad) return "aad_len must be in 0..64";
    if (n < 0) return "negative n";
    if ((size_t)n > kMaxRows) return "batch too large";
    return nullptr;
}
// the arrays a call of n > 0 messages must be given: aad iff aad_len > 0, in and out iff len > 0
inline const char *aes_gcm_auth_null_error(const void *keys, const void *nonces, const void *aad, size_t aad_len,
                                           const void *in, const void *out, size_t len, const void *tags,
                                           const void *ok, bool open) {
    if (!keys || !nonces || !tags || (open && !ok)) return "NULL argument";
    if ((aad != nullptr) != (aad_len != 0)) return "aad must be NULL exactly when aad_len is 0";
    if (len != 0 && (!in || !out)) return "NULL argument";
    return nullptr;
}

inline const char *ecdsa_verify_dims_error(int n) {
    if (n < 0) return "negative n";
    if ((size_t)n > kMaxRows) return "batch too large";
    return nullptr;
}
// the kernel reads each row with 16-byte loads: the _dev form's input pointers must allow them
inline bool ecdsa_verify_aligned(uintptr_t pubkeys, uintptr_t digests, uintptr_t sigs) {
    return ((pubkeys | digests | sigs) & 15) == 0;
}

inline const char *feldman_verify_dims_error(int T, int M, int x_bits, int n) {
    if (T < 1) return "T must be at least 1 (term 0 commits to the secret)";
    if (M < 1) return "M must be at least 1";
    if (x_bits < 1 || x_bits > 32) return "x_bits must be in 1..32";
    if (n < 0) return "negative n";
    if ((size_t)n > kMaxRows || (size_t)T * (size_t)M > kMaxRows) return "batch too large";
    return nullptr;
}
// index of the first row whose dealer is not below M, or -1 (the host form's check; dealer may be NULL)
inline int feldman_bad_dealer(const uint32_t *dealer, int n, int M) {
    if (!dealer) return -1;
    for (int i = 0; i < n; ++i)
        if (dealer[i] >= (uint32_t)M) return i;
    return -1;
}
// the kernel reads commitments and shares, and writes points, with 16-byte accesses
inline bool feldman_verify_aligned(uintptr_t commitments, uintptr_t shares, uintptr_t points) {
    return ((commitments | shares | points) & 15) == 0;
}

// ------------------------------------------------------------------ the arrays
// The context's scratch buffers, by the flm_ctx member behind each.  Slots, not meanings: AES keys
// travel in ec_scal, Feldman's verdicts in bytes_out.  Which array takes which slot, and in what
// order the arrays are declared, fixes the bounce layout and the allocation pattern: keep both.
enum Slot : uint8_t { ec_in, ec_base, ec_scal, ec_out, ec_dig, ec_flags, bytes_in, bytes_out, rows, out, seeds, signs, kSlots };

struct Arg {
    size_t width, rows;       // bytes per row, rows (a plain array: one row)
    size_t h_pitch, d_pitch;  // bytes between rows on the host and in the scratch buffer
    Slot slot;
    bool is_out;
    bool in_place;  // may run in the bounce buffer itself (flm_host_layout.h), rows at the layout's pitch
    bool present;   // an optional array the caller left out takes no span and no slot
};
constexpr int kMaxArgs = 8;  // HostCopies' limit
struct ArgList {
    Arg a[kMaxArgs];
    int n;
};

constexpr Arg arg_in(size_t bytes, Slot s, bool present = true) { return {bytes, 1, bytes, bytes, s, false, false, present}; }
constexpr Arg arg_out(size_t bytes, Slot s, bool present = true) { return {bytes, 1, bytes, bytes, s, true, false, present}; }
constexpr Arg in_place(Arg a) { return {a.width, a.rows, a.h_pitch, a.d_pitch, a.slot, a.is_out, true, a.present}; }
// n_rows rows of a's bytes each: packed on the host, d_pitch bytes apart in the scratch buffer
constexpr Arg pitched(Arg a, size_t n_rows, size_t d_pitch) {
    return {a.width, n_rows, a.width, d_pitch, a.slot, a.is_out, a.in_place, a.present};
}

// two arrays of one call in the same scratch buffer would overwrite each other
inline bool names_slot_twice(const ArgList &l) {
    unsigned seen = 0;
    for (int i = 0; i < l.n; ++i) {
        if (!l.a[i].present) continue;
        if (seen >> l.a[i].slot & 1u) return true;
        seen |= 1u << l.a[i].slot;
    }
    return false;
}

// Per call, the arrays in the order of the host pointers HostCopies::declare is given.  n, T, M, C, D
// as the call's own arguments, size_t so that no product overflows below the row limit.

// shares, lambdas, c1, flags, points_out, seeds_out
inline ArgList ec_combine_args(size_t T, size_t D, bool c1, bool points, bool seeds) {
    return {{arg_in(T * D * 64, ec_in), arg_in(T * 32, ec_scal), arg_in(D * 64, ec_base, c1), arg_out(D * 4, ec_flags),
             arg_out(D * 64, ec_out, points), arg_out(D * 32, ec_dig, seeds)}, 6};
}
// shares, lambdas, seeds_out
inline ArgList shamir_combine_args(size_t T, size_t M) {
    return {{arg_in(T * M * 32, ec_in), arg_in(T * 32, ec_scal), arg_out(M * 32, ec_dig)}, 3};
}
// coeffs, xs, shares_out
inline ArgList shamir_deal_args(size_t T, size_t M, size_t C) {
    return {{arg_in(T * M * 32, ec_in), arg_in(C * 4, ec_scal), arg_out(C * M * 32, ec_out)}, 3};
}
// keys, nonces, in, out (in == out on the host is fine: they are two spans)
inline ArgList aes_gcm_xor_args(size_t nonce_len, size_t len, size_t n) {
    return {{arg_in(n * 16, ec_scal), arg_in(n * nonce_len, ec_base), in_place(arg_in(n * len, bytes_in)),
             in_place(arg_out(n * len, bytes_out))}, 4};
}
// keys, nonces, aad, in, out, tags (seal writes them, open reads them), ok_out (open)
inline ArgList aes_gcm_auth_args(size_t nonce_len, size_t aad_len, size_t len, size_t n, bool open) {
    return {{arg_in(n * 16, ec_scal), arg_in(n * nonce_len, ec_base), arg_in(n * aad_len, ec_in, aad_len != 0),
             in_place(arg_in(n * len, bytes_in, len != 0)), in_place(arg_out(n * len, bytes_out, len != 0)),
             open ? arg_in(n * 16, ec_dig) : arg_out(n * 16, ec_dig), arg_out(n, ec_out, open)}, 7};
}
// pubkeys, digests, sigs, ok_out, flags_out
inline ArgList ecdsa_verify_args(size_t n, bool flags) {
    return {{arg_in(n * 64, ec_in), arg_in(n * 32, ec_base), arg_in(n * 64, ec_scal), arg_out(n, ec_out),
             arg_out(n * 4, ec_flags, flags)}, 5};
}
// commitments, dealer, xs, shares, ok_out, points_out, flags_out
inline ArgList feldman_verify_args(size_t T, size_t M, size_t n, bool dealer, bool points, bool flags) {
    return {{arg_in(T * M * 64, ec_in), arg_in(n * 4, ec_dig, dealer), arg_in(n * 4, ec_scal), arg_in(n * 32, ec_base),
             arg_out(n, bytes_out), arg_out(n * 64, ec_out, points), arg_out(n * 4, ec_flags, flags)}, 7};
}
// points, scalars, flags, out
inline ArgList ec_mul_args(size_t n) {
    return {{arg_in(n * 64, ec_in), arg_in(n * 32, ec_scal), arg_out(n * 4, ec_flags), arg_out(n * 64, ec_out)}, 4};
}
// uniform bytes or messages, lens (with messages), flags, out; neither input: the decimal form
inline ArgList h2c_args(size_t n, bool uniform, bool msgs) {
    return {{arg_in(n * (uniform ? 96 : 64), ec_in, uniform || msgs), arg_in(n * 4, ec_scal, msgs && !uniform),
             arg_out(n * 4, ec_flags), arg_out(n * 64, ec_out)}, 4};
}


// The round path.  N, K, L as the call's own arguments; rows of L words travel at the host forms' device
// pitch of round_up(L, 64) words.  Seeds and signs are declared at K = 0 too (no bytes, the buffers
// still allocated).

constexpr size_t host_row_pitch(size_t L) { return round_up(L, 64) * 4; }  // bytes

// x, seeds, signs, out.  One client's call (c5: 4 MiB in, 4 MiB out) runs in place: the kernel reads x from
// and writes out to the pinned bounce buffer, so the link carries both at once instead of a DMA each way;
// x and out have one shape, so one pitch.  Nothing reads the device copy of the signs (flm_client_mask_dev
// takes them from the host array): without it out's bounce offset moves, a change to measure on its own.
inline ArgList client_mask_args(size_t N, size_t K, size_t L, bool x) {
    return {{in_place(pitched(arg_in(L * 4, rows, x), N, host_row_pitch(L))), arg_in(K * 32, seeds), arg_in(K, signs),
             in_place(pitched(arg_out(L * 4, out), N, host_row_pitch(L)))}, 4};
}
// flm_client_encode_mask, _pack_mask, _noise_mask: x (L floats a row), seeds, dither, noise, out (Lw =
// packed_words(L, pack) words a row), clipped; the signs stay on the host.  x and out in place as flm_client_mask's,
// each at a pitch of its own; the clients' N x 32 noise seeds, when they travel, in ec_scal.
inline ArgList client_encode_mask_args(size_t N, size_t K, size_t L, size_t Lw, bool dither, bool noise, bool clipped) {
    return {{in_place(pitched(arg_in(L * 4, rows), N, host_row_pitch(L))), arg_in(K * 32, seeds),
             arg_in(N * 32, bytes_in, dither), arg_in(N * 32, ec_scal, noise),
             in_place(pitched(arg_out(Lw * 4, out), N, host_row_pitch(Lw))), arg_out(N * 4, bytes_out, clipped)}, 6};
}
// flm_client_encode_gauss_mask: client_encode_mask_args with the noise seeds always there and the table's T = 2 tail
// uint64 entries after them, in ec_dig
inline ArgList client_encode_gauss_mask_args(size_t N, size_t K, size_t L, size_t Lw, bool dither, size_t T, bool clipped) {
    return {{in_place(pitched(arg_in(L * 4, rows), N, host_row_pitch(L))), arg_in(K * 32, seeds),
             arg_in(N * 32, bytes_in, dither), arg_in(N * 32, ec_scal), arg_in(T * 8, ec_dig),
             in_place(pitched(arg_out(Lw * 4, out), N, host_row_pitch(Lw))), arg_out(N * 4, bytes_out, clipped)}, 7};
}
// sum (Lw words), out (L floats); Lw = L: the unpacked decode, which may then run in place
inline ArgList decode_unpack_args(size_t L, size_t Lw) {
    return {{in_place(arg_in(Lw * 4, rows)), in_place(arg_out(L * 4, out))}, 2};
}
// flm_decode_unpack_mod: the packed decode's sum and out, and stats (two words: the kernel's atomics land in device
// memory, never in the bounce buffer)
inline ArgList decode_unpack_mod_args(size_t L, size_t Lw, bool stats) {
    return {{in_place(arg_in(Lw * 4, rows)), in_place(arg_out(L * 4, out)), arg_out(8, ec_flags, stats)}, 3};
}
// flm_rotate, flm_rotate_clip: x (N rows of L_in floats), out (N rows of L_out floats), key, nonfinite, and the clip's
// factors and sumsq as flm_l2_clip's (absent for the plain rotation); forward L_in = L and L_out = L_rot, the inverse
// the other way round.  x and out in place as the decode's, rows at the in-place pitch of round_up(width, 16) bytes,
// which is what rotate_kernel's 16-byte accesses need.  The sign words the key expands to live in a buffer of the
// context that no list names (flm_ctx::rot_signs).
inline ArgList rotate_args(size_t N, size_t L_in, size_t L_out, bool nonfinite, bool factors, bool sumsq) {
    return {{in_place(pitched(arg_in(L_in * 4, rows), N, host_row_pitch(L_in))),
             in_place(pitched(arg_out(L_out * 4, out), N, host_row_pitch(L_out))), arg_in(32, seeds),
             arg_out(N * 4, bytes_out, nonfinite), arg_out(N * 4, ec_flags, factors), arg_out(N * 8, ec_dig, sumsq)}, 6};
}
// flm_l2_clip: x and out (N rows of L floats, in place as the rotation's), factors (N floats), sumsq (N doubles).
// The tile partials, and the factors when the caller wants none back, live in a buffer of the context that no list
// names (flm_ctx::l2_work).
inline ArgList l2_clip_args(size_t N, size_t L, bool factors, bool sumsq) {
    return {{in_place(pitched(arg_in(L * 4, rows), N, host_row_pitch(L))),
             in_place(pitched(arg_out(L * 4, out), N, host_row_pitch(L))), arg_out(N * 4, ec_flags, factors),
             arg_out(N * 8, ec_dig, sumsq)}, 4};
}
// flm_round_select: x (N rows of L floats, in place as the rotation's: read only), candidates (N A seeds), sumsq
// (N A uint64: the kernel's atomics land in device memory, never in the bounce buffer), dither (N seeds), chosen (N
// words)
inline ArgList round_select_args(size_t N, size_t L, size_t A) {
    return {{in_place(pitched(arg_in(L * 4, rows), N, host_row_pitch(L))), arg_in(N * A * 32, seeds),
             arg_out(N * A * 8, ec_dig), arg_out(N * 32, bytes_out), arg_out(N * 4, ec_flags)}, 5};
}
// seeds, out (K rows)
inline ArgList prg_expand_args(size_t K, size_t L) {
    return {{arg_in(K * 32, seeds), in_place(pitched(arg_out(L * 4, out), K, host_row_pitch(L)))}, 2};
}
// acc as the one row read, acc as the row written (in place in the bounce buffer when it fits), seeds, signs.
// The rows first, the seeds after: with the seeds between them, out off a 4 KiB boundary, the call measured
// 0.41 ms against 0.34-0.37.
inline ArgList mask_accumulate_args(size_t K, size_t L) {
    return {{in_place(pitched(arg_in(L * 4, rows), 1, host_row_pitch(L))),
             in_place(pitched(arg_out(L * 4, out), 1, host_row_pitch(L))), arg_in(K * 32, seeds), arg_in(K, signs)}, 4};
}
// seeds, signs, out (a group's rank keeps its sum on the device: no out).  The rows go up on their own
// (upload_rows: one host pointer each).
inline ArgList aggregate_unmask_args(size_t K, size_t L, bool out_host) {
    return {{arg_in(K * 32, seeds), arg_in(K, signs), arg_out(L * 4, out, out_host)}, 3};
}
// in, out (in == out on the host is fine: they are two spans)
inline ArgList chacha20_xor_args(size_t n) { return {{in_place(arg_in(n, bytes_in)), in_place(arg_out(n, bytes_out))}, 2}; }

}  // namespace rt
}  // namespace flm
