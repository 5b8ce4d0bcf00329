// deal_args_check.cpp -- the host side of flm_shamir_deal / flm_aes_gcm_xor without a GPU, for the
// host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I flamingo_amd/csrc tools/deal_args_check.cpp -o build/deal_args_check && build/deal_args_check
// It runs the argument rules (flm_deal_args.h) over accepted and refused calls, and for the accepted
// ones declares the call's arrays to the bounce-buffer layout (flm_host_layout.h) exactly as the
// host-pointer entry points do, then copies every array into and out of a heap buffer of the size
// the layout returned -- the copies HostCopies makes, with the kernel replaced by a byte-wise stand-in.
// A span placed past the buffer, or overlapping another, is then a sanitizer report or a failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flm_deal_args.h"
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

// the spans of one call through a heap "bounce buffer": inputs copied in, outputs filled and copied out
static void through_bounce(std::vector<HostSpan> spans, const std::vector<bool> &is_out) {
    const size_t total = host_layout(spans.data(), (int)spans.size());
    std::vector<uint8_t> bounce(total);
    size_t end = 0;
    for (size_t i = 0; i < spans.size(); ++i) {
        const HostSpan &s = spans[i];
        CHECK(s.route != kRouteRing);  // every shape here is far below the staging size
        CHECK(s.offset >= end && s.offset % 256 == 0);
        const size_t room = s.rows * s.pitch;
        CHECK(s.offset + room <= total);
        end = s.offset + room;
        std::vector<uint8_t> host(s.rows * s.width, (uint8_t)(i + 1));
        for (size_t r = 0; r < s.rows; ++r) {
            uint8_t *b = bounce.data() + s.offset + r * s.pitch;
            if (is_out[i]) {
                std::memset(b, 0x5a, s.width);  // the kernel's stand-in
                std::memcpy(host.data() + r * s.width, b, s.width);
            } else {
                std::memcpy(b, host.data() + r * s.width, s.width);
            }
        }
        if (is_out[i] && !host.empty()) CHECK(host.front() == 0x5a && host.back() == 0x5a);
    }
}

int main() {
    // ---- flm_shamir_deal
    CHECK(shamir_deal_dims_error(0, 1, 1) && shamir_deal_dims_error(-1, 1, 1));
    CHECK(shamir_deal_dims_error(1, 1, 0) && shamir_deal_dims_error(1, 1, -3));
    CHECK(shamir_deal_dims_error(1, -1, 1));
    CHECK(shamir_deal_dims_error(1 << 14, 1 << 13, 1) && shamir_deal_dims_error(1, 1 << 20, 1 << 7));
    CHECK(shamir_deal_dims_error(0x7fffffff, 0x7fffffff, 0x7fffffff));  // no overflow on the way to "too large"
    CHECK(!shamir_deal_dims_error(1, 0, 1) && !shamir_deal_dims_error(20, 4096, 60));
    CHECK(!shamir_deal_dims_error(1 << 13, 1 << 13, 1 << 13));  // exactly 2^26 lanes
    const uint32_t ok[4] = {1, 2, 2, 0xffffffffu}, bad[4] = {1, 2, 0, 0};
    CHECK(shamir_deal_zero_x(ok, 4) == -1 && shamir_deal_zero_x(bad, 4) == 2 && shamir_deal_zero_x(bad, 2) == -1);
    const int deals[][3] = {{1, 1, 1}, {1, 2, 3}, {2, 1, 3}, {3, 65, 5}, {40, 130, 60}, {20, 4096, 60}};
    for (const auto &d : deals) {
        CHECK(!shamir_deal_dims_error(d[0], d[1], d[2]));
        const ShamirDealBytes nb = shamir_deal_bytes(d[0], d[1], d[2]);
        CHECK(nb.coeffs == (size_t)d[0] * d[1] * 32 && nb.xs == (size_t)d[2] * 4 && nb.shares == (size_t)d[2] * d[1] * 32);
        through_bounce({{nb.coeffs, 1, false}, {nb.xs, 1, false}, {nb.shares, 1, false}}, {false, false, true});
    }
    // ---- flm_aes_gcm_xor
    CHECK(aes_gcm_dims_error(13, 32, 1) && aes_gcm_dims_error(0, 32, 1) && aes_gcm_dims_error(-16, 32, 1));
    CHECK(aes_gcm_dims_error(16, 0, 1) && aes_gcm_dims_error(16, 257, 1) && aes_gcm_dims_error(12, (size_t)-1, 1));
    CHECK(aes_gcm_dims_error(16, 32, -1) && aes_gcm_dims_error(16, 32, (1 << 26) + 1));
    CHECK(!aes_gcm_dims_error(12, 1, 0) && !aes_gcm_dims_error(16, 256, 1 << 26));
    const size_t lens[] = {1, 15, 16, 17, 32, 33, 64, 256};
    for (int nonce_len : {12, 16})
        for (size_t len : lens)
            for (int n : {1, 65, 245760}) {
                CHECK(!aes_gcm_dims_error(nonce_len, len, n));
                const AesGcmBytes nb = aes_gcm_bytes(nonce_len, len, n);
                CHECK(nb.keys == (size_t)n * 16 && nb.nonces == (size_t)n * nonce_len && nb.data == (size_t)n * len);
                if (nb.data >= kStageBytes) continue;  // 245,760 x 256 B streams through the ring instead
                through_bounce({{nb.keys, 1, false}, {nb.nonces, 1, false}, {nb.data, 1, true}, {nb.data, 1, true}},
                               {false, false, false, true});
            }
    std::printf(failures ? "%d checks failed\n" : "deal_args_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
