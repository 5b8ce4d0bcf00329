// flm_ecdsa_args.h -- argument rules of flm_ecdsa_verify[_dev] (flm_runtime.hip).  Plain C++ with no
// HIP in it, like flm_deal_args.h, so the rules and the byte counts the host-pointer call declares to
// HostCopies run on the CPU under the host sanitizers (tools/ecdsa_args_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace flm {
namespace rt {

constexpr size_t kEcdsaMaxRows = size_t(1) << 26;  // signatures per call (the EC size limit, ec_dims)

// nullptr when a batch of n signatures may run (n = 0 runs nothing), else what is wrong
inline const char *ecdsa_verify_dims_error(int n) {
    if (n < 0) return "negative n";
    if ((size_t)n > kEcdsaMaxRows) return "batch too large";
    return nullptr;
}

// the kernel reads each row with 16-byte loads: the _dev form's input pointers must allow them
inline bool ecdsa_verify_aligned(uintptr_t pubkeys, uintptr_t digests, uintptr_t sigs) {
    return ((pubkeys | digests | sigs) & 15) == 0;
}

// bytes of each array of a call, as the host-pointer form declares them to HostCopies
struct EcdsaVerifyBytes {
    size_t pubkeys, digests, sigs, ok, flags;
};
inline EcdsaVerifyBytes ecdsa_verify_bytes(int n) {
    return {(size_t)n * 64, (size_t)n * 32, (size_t)n * 64, (size_t)n, (size_t)n * 4};
}

}  // namespace rt
}  // namespace flm
