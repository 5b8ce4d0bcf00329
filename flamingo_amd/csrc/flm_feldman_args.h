// flm_feldman_args.h -- argument rules of flm_feldman_verify[_dev] (flm_runtime.hip).  Plain C++ with no
// HIP in it, like flm_ecdsa_args.h and flm_deal_args.h, so the rules and the byte counts the
// host-pointer call declares to HostCopies run on the CPU under the host sanitizers
// (tools/feldman_args_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace flm {
namespace rt {

constexpr size_t kFeldmanMaxRows = size_t(1) << 26;  // share checks, and commitments, per call (as ec_dims)

// nullptr when n checks against T x M commitments may run (n = 0 runs nothing), else what is wrong
inline const char *feldman_verify_dims_error(int T, int M, int x_bits, int n) {
    if (T < 1) return "T must be at least 1 (term 0 commits to the secret)";
    if (M < 1) return "M must be at least 1";
    if (x_bits < 1 || x_bits > 32) return "x_bits must be in 1..32";
    if (n < 0) return "negative n";
    if ((size_t)n > kFeldmanMaxRows || (size_t)T * (size_t)M > kFeldmanMaxRows) return "batch too large";
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

// bytes of each array of a call, as the host-pointer form declares them to HostCopies
struct FeldmanVerifyBytes {
    size_t commitments, dealer, xs, shares, ok, points, flags;
};
inline FeldmanVerifyBytes feldman_verify_bytes(int T, int M, int n) {
    return {(size_t)T * (size_t)M * 64, (size_t)n * 4, (size_t)n * 4, (size_t)n * 32,
            (size_t)n,                  (size_t)n * 64, (size_t)n * 4};
}

}  // namespace rt
}  // namespace flm
