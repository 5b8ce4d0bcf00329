// flm_deal_args.h -- argument rules of flm_shamir_deal[_dev], flm_aes_gcm_xor[_dev] and
// flm_aes_gcm_seal[_dev] / flm_aes_gcm_open[_dev] (flm_runtime.hip).  Plain C++ with no HIP in it, like flm_host_layout.h, so the rules and the
// byte counts the host-pointer calls declare to HostCopies run on the CPU under the host sanitizers
// (tools/deal_args_check.cpp, tools/gcm_args_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace flm {
namespace rt {

constexpr size_t kDealMaxLanes = size_t(1) << 26;  // shares or coefficients per call (as ec_dims)
constexpr size_t kAesMaxLen = 256;                 // bytes per message

// nullptr when a dealing of T coefficients x M secrets at C points may run, else what is wrong
inline const char *shamir_deal_dims_error(int T, int M, int C) {
    if (T < 1) return "T must be at least 1 (term 0 is the secret)";
    if (C < 1) return "C must be at least 1";
    if (M < 0) return "negative M";
    if ((size_t)T * (size_t)M > kDealMaxLanes || (size_t)C * (size_t)M > kDealMaxLanes) return "batch too large";
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
    if ((size_t)n > kDealMaxLanes) return "batch too large";
    return nullptr;
}

// flm_aes_gcm_seal / flm_aes_gcm_open: len 0 is a tag over the AAD alone
constexpr size_t kAesMaxAad = 64;  // bytes of AAD per message
inline const char *aes_gcm_auth_dims_error(int nonce_len, size_t aad_len, size_t len, int n) {
    if (nonce_len != 12 && nonce_len != 16) return "nonce_len must be 12 or 16";
    if (len > kAesMaxLen) return "len must be in 0..256";
    if (aad_len > kAesMaxAad) return "aad_len must be in 0..64";
    if (n < 0) return "negative n";
    if ((size_t)n > kDealMaxLanes) return "batch too large";
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

// bytes of each array of a call, as the host-pointer forms declare them to HostCopies
struct ShamirDealBytes {
    size_t coeffs, xs, shares;
};
inline ShamirDealBytes shamir_deal_bytes(int T, int M, int C) {
    return {(size_t)T * (size_t)M * 32, (size_t)C * 4, (size_t)C * (size_t)M * 32};
}
struct AesGcmBytes {
    size_t keys, nonces, data;
};
inline AesGcmBytes aes_gcm_bytes(int nonce_len, size_t len, int n) {
    return {(size_t)n * 16, (size_t)n * (size_t)nonce_len, (size_t)n * len};
}

struct AesGcmAuthBytes {
    size_t keys, nonces, aad, data, tags, ok;
};
inline AesGcmAuthBytes aes_gcm_auth_bytes(int nonce_len, size_t aad_len, size_t len, int n) {
    return {(size_t)n * 16, (size_t)n * (size_t)nonce_len, (size_t)n * aad_len, (size_t)n * len, (size_t)n * 16, (size_t)n};
}

}  // namespace rt
}  // namespace flm
