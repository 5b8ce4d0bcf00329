// ecdsa_args_check.cpp -- the host side of flm_ecdsa_verify without a GPU, for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I flamingo_amd/csrc tools/ecdsa_args_check.cpp -o build/ecdsa_args_check && build/ecdsa_args_check
// It runs the argument rules (flm_ecdsa_args.h) over accepted and refused calls, and for the accepted
// ones declares the call's five arrays to the bounce-buffer layout (flm_host_layout.h) exactly as the
// host-pointer entry point does, then copies every array into and out of a heap buffer of the size
// the layout returned -- the copies HostCopies makes, with the kernel replaced by a byte-wise stand-in
// that reads every input byte of a row and writes its verdict and flag word.  A span placed past the
// buffer, or overlapping another, is then a sanitizer report or a failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flm_ecdsa_args.h"
#include "flm_host_layout.h"

using namespace flm::rt;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// one call of n rows through a heap "bounce buffer"; with_flags as flags_out != NULL
static void through_bounce(int n, bool with_flags) {
    const EcdsaVerifyBytes nb = ecdsa_verify_bytes(n);
    std::vector<HostSpan> spans = {{nb.pubkeys, 1, false}, {nb.digests, 1, false}, {nb.sigs, 1, false}, {nb.ok, 1, false}};
    if (with_flags) spans.push_back({nb.flags, 1, false});
    const size_t total = host_layout(spans.data(), (int)spans.size());
    std::vector<uint8_t> bounce(total);
    size_t end = 0;
    for (const HostSpan &s : spans) {
        CHECK(s.route == kRouteBounce);  // 2^26 rows x 64 bytes would stream; every shape here is far below
        CHECK(s.offset >= end && s.offset % 256 == 0);
        CHECK(s.offset + s.rows * s.pitch <= total);
        end = s.offset + s.rows * s.pitch;
    }
    // inputs in
    std::vector<uint8_t> pk(nb.pubkeys), dg(nb.digests), sg(nb.sigs);
    for (size_t i = 0; i < pk.size(); ++i) pk[i] = (uint8_t)(i * 7 + 1);
    for (size_t i = 0; i < dg.size(); ++i) dg[i] = (uint8_t)(i * 5 + 2);
    for (size_t i = 0; i < sg.size(); ++i) sg[i] = (uint8_t)(i * 3 + 3);
    std::memcpy(bounce.data() + spans[0].offset, pk.data(), pk.size());
    std::memcpy(bounce.data() + spans[1].offset, dg.data(), dg.size());
    std::memcpy(bounce.data() + spans[2].offset, sg.data(), sg.size());
    // the kernel's stand-in: row i reads its 64 + 32 + 64 bytes, writes ok[i] and flags[i]
    const uint8_t *bq = bounce.data() + spans[0].offset, *be = bounce.data() + spans[1].offset,
                  *bs = bounce.data() + spans[2].offset;
    uint8_t *bok = bounce.data() + spans[3].offset;
    for (int i = 0; i < n; ++i) {
        uint32_t sum = 0;
        for (int k = 0; k < 64; ++k) sum += bq[(size_t)i * 64 + k] + bs[(size_t)i * 64 + k];
        for (int k = 0; k < 32; ++k) sum += be[(size_t)i * 32 + k];
        bok[i] = (uint8_t)(sum & 1u);
        if (with_flags) std::memcpy(bounce.data() + spans[4].offset + (size_t)i * 4, &sum, 4);
    }
    // outputs out
    std::vector<uint8_t> ok(nb.ok);
    std::vector<uint32_t> fl(with_flags ? n : 0);
    std::memcpy(ok.data(), bok, ok.size());
    if (with_flags) std::memcpy(fl.data(), bounce.data() + spans[4].offset, nb.flags);
    for (int i = 0; i < n; ++i) {
        uint32_t sum = 0;
        for (int k = 0; k < 64; ++k) sum += pk[(size_t)i * 64 + k] + sg[(size_t)i * 64 + k];
        for (int k = 0; k < 32; ++k) sum += dg[(size_t)i * 32 + k];
        CHECK(ok[i] == (sum & 1u));
        if (with_flags) CHECK(fl[i] == sum);
    }
}

int main() {
    CHECK(ecdsa_verify_dims_error(-1) && ecdsa_verify_dims_error(-0x7fffffff - 1));
    CHECK(ecdsa_verify_dims_error((1 << 26) + 1) && ecdsa_verify_dims_error(0x7fffffff));
    CHECK(!ecdsa_verify_dims_error(0) && !ecdsa_verify_dims_error(1) && !ecdsa_verify_dims_error(61));
    CHECK(!ecdsa_verify_dims_error(1 << 26));  // exactly the EC size limit
    CHECK(kEcdsaMaxRows == (size_t(1) << 26));
    CHECK(ecdsa_verify_aligned(0x1000, 0x2010, 0x30f0));
    CHECK(!ecdsa_verify_aligned(0x1001, 0x2000, 0x3000) && !ecdsa_verify_aligned(0x1000, 0x2008, 0x3000) &&
          !ecdsa_verify_aligned(0x1000, 0x2000, 0x300f));
    const EcdsaVerifyBytes top = ecdsa_verify_bytes(1 << 26);  // no overflow at the limit
    CHECK(top.pubkeys == (size_t(1) << 32) && top.digests == (size_t(1) << 31) && top.sigs == (size_t(1) << 32) &&
          top.ok == (size_t(1) << 26) && top.flags == (size_t(1) << 28));
    const EcdsaVerifyBytes none = ecdsa_verify_bytes(0);
    CHECK(none.pubkeys == 0 && none.digests == 0 && none.sigs == 0 && none.ok == 0 && none.flags == 0);
    for (int n : {1, 2, 61, 63, 64, 65, 255, 256, 257, 3660, 4096, 245760}) {
        CHECK(!ecdsa_verify_dims_error(n));
        const EcdsaVerifyBytes nb = ecdsa_verify_bytes(n);
        CHECK(nb.pubkeys == (size_t)n * 64 && nb.digests == (size_t)n * 32 && nb.sigs == (size_t)n * 64 &&
              nb.ok == (size_t)n && nb.flags == (size_t)n * 4);
        through_bounce(n, true);
        through_bounce(n, false);
    }
    std::printf(failures ? "%d checks failed\n" : "ecdsa_args_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
