// flm_call_args.h -- the batch crypto calls of flm_runtime.hip (P-256, Shamir, AES-GCM, ECDSA, Feldman,
// hash to curve): their argument rules, and per call the one ordered list of the arrays its
// host-pointer form moves -- bytes, direction, whether it may run in place, which of the context's
// scratch buffers it lands in, whether it is there at all.  HostCopies::declare takes that list, and
// so does tools/args_check.cpp: plain C++ with no HIP in it, like flm_host_layout.h, so the rules and
// the lists the runtime uses are the ones checked on the CPU under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace flm {
namespace rt __attribute__((visibility("hidden"))) {  // the library exports nothing of this header

constexpr size_t kMaxRows = size_t(1) << 26;  // lanes (rows, shares, coefficients, commitments) per call
constexpr size_t kAesMaxLen = 256;            // bytes per message
constexpr size_t kAesMaxAad = 64;             // bytes of AAD per message

// ------------------------------------------------------------------ the rules
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
enum Slot : uint8_t { ec_in, ec_base, ec_scal, ec_out, ec_dig, ec_flags, bytes_in, bytes_out, kSlots };

struct Arg {
    size_t bytes;
    Slot slot;
    bool is_out;
    bool in_place;  // may run in the bounce buffer itself (flm_host_layout.h)
    bool present;   // an optional array the caller left out takes no span and no slot
};
constexpr int kMaxArgs = 8;  // HostCopies' limit
struct ArgList {
    Arg a[kMaxArgs];
    int n;
};

constexpr Arg arg_in(size_t bytes, Slot s, bool present = true) { return {bytes, s, false, false, present}; }
constexpr Arg arg_out(size_t bytes, Slot s, bool present = true) { return {bytes, s, true, false, present}; }
constexpr Arg in_place(Arg a) { return {a.bytes, a.slot, a.is_out, true, a.present}; }

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

}  // namespace rt
}  // namespace flm
