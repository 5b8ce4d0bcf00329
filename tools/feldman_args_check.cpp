// feldman_args_check.cpp -- the host side of flm_feldman_verify without a GPU, for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I flamingo_amd/csrc tools/feldman_args_check.cpp -o build/feldman_args_check && build/feldman_args_check
// It runs the argument rules (flm_feldman_args.h) over accepted and refused calls, and for the accepted
// ones declares the call's arrays (dealer, points_out and flags_out optional) to the bounce-buffer
// layout (flm_host_layout.h) exactly as the host-pointer entry point does, then copies every array into
// and out of a heap buffer of the size the layout returned -- the copies HostCopies makes, with the
// kernel replaced by a byte-wise stand-in that reads what a row's lane reads (its x, its share, its
// dealer's T commitments) and writes its verdict, point and flag word.  A span placed past the buffer,
// or overlapping another, or a dealer index the rules let through, is then a sanitizer report or a
// failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flm_feldman_args.h"
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

static uint32_t row_sum(const uint8_t *com, int T, int M, uint32_t d, uint32_t x, const uint8_t *share) {
    uint32_t sum = x;
    for (int k = 0; k < T; ++k)
        for (int b = 0; b < 64; ++b) sum += com[((size_t)k * M + d) * 64 + b];
    for (int b = 0; b < 32; ++b) sum += share[b];
    return sum;
}

// one call of n rows against T x M commitments through a heap "bounce buffer"
static void through_bounce(int T, int M, int n, bool with_dealer, bool with_points, bool with_flags) {
    const FeldmanVerifyBytes nb = feldman_verify_bytes(T, M, n);
    std::vector<HostSpan> spans = {{nb.commitments, 1, false}};
    int i_dealer = -1, i_points = -1, i_flags = -1;
    if (with_dealer) i_dealer = (int)spans.size(), spans.push_back({nb.dealer, 1, false});
    const int i_xs = (int)spans.size();
    spans.push_back({nb.xs, 1, false});
    const int i_sh = (int)spans.size();
    spans.push_back({nb.shares, 1, false});
    const int i_ok = (int)spans.size();
    spans.push_back({nb.ok, 1, false});
    if (with_points) i_points = (int)spans.size(), spans.push_back({nb.points, 1, false});
    if (with_flags) i_flags = (int)spans.size(), spans.push_back({nb.flags, 1, false});
    CHECK(spans.size() <= 8);  // HostCopies::kMaxSpans
    const size_t total = host_layout(spans.data(), (int)spans.size());
    std::vector<uint8_t> bounce(total);
    size_t end = 0;
    for (const HostSpan &s : spans) {
        CHECK(s.route == kRouteBounce);
        CHECK(s.offset >= end && s.offset % 256 == 0);
        CHECK(s.offset + s.rows * s.pitch <= total);
        end = s.offset + s.rows * s.pitch;
    }
    std::vector<uint8_t> com(nb.commitments), sh(nb.shares);
    std::vector<uint32_t> dealer(n), xs(n);
    for (size_t i = 0; i < com.size(); ++i) com[i] = (uint8_t)(i * 7 + 1);
    for (size_t i = 0; i < sh.size(); ++i) sh[i] = (uint8_t)(i * 3 + 3);
    for (int i = 0; i < n; ++i) dealer[i] = (uint32_t)((i * 5 + 2) % M), xs[i] = (uint32_t)i * 2654435761u;
    CHECK(feldman_bad_dealer(with_dealer ? dealer.data() : nullptr, n, M) == -1);
    std::memcpy(bounce.data() + spans[0].offset, com.data(), com.size());
    if (with_dealer) std::memcpy(bounce.data() + spans[i_dealer].offset, dealer.data(), nb.dealer);
    std::memcpy(bounce.data() + spans[i_xs].offset, xs.data(), nb.xs);
    std::memcpy(bounce.data() + spans[i_sh].offset, sh.data(), sh.size());
    // the kernel's stand-in
    for (int i = 0; i < n; ++i) {
        uint32_t d = (uint32_t)(i % M), x;
        if (with_dealer) std::memcpy(&d, bounce.data() + spans[i_dealer].offset + (size_t)i * 4, 4);
        std::memcpy(&x, bounce.data() + spans[i_xs].offset + (size_t)i * 4, 4);
        const uint32_t sum = row_sum(bounce.data() + spans[0].offset, T, M, d, x,
                                     bounce.data() + spans[i_sh].offset + (size_t)i * 32);
        bounce[spans[i_ok].offset + i] = (uint8_t)(sum & 1u);
        if (with_points) std::memset(bounce.data() + spans[i_points].offset + (size_t)i * 64, (int)(sum & 0xff), 64);
        if (with_flags) std::memcpy(bounce.data() + spans[i_flags].offset + (size_t)i * 4, &sum, 4);
    }
    // outputs out
    std::vector<uint8_t> ok(nb.ok), pts(with_points ? nb.points : 0);
    std::vector<uint32_t> fl(with_flags ? n : 0);
    std::memcpy(ok.data(), bounce.data() + spans[i_ok].offset, ok.size());
    if (with_points) std::memcpy(pts.data(), bounce.data() + spans[i_points].offset, nb.points);
    if (with_flags) std::memcpy(fl.data(), bounce.data() + spans[i_flags].offset, nb.flags);
    for (int i = 0; i < n; ++i) {
        const uint32_t d = with_dealer ? dealer[i] : (uint32_t)(i % M);
        const uint32_t sum = row_sum(com.data(), T, M, d, xs[i], sh.data() + (size_t)i * 32);
        CHECK(ok[i] == (sum & 1u));
        if (with_points) CHECK(pts[(size_t)i * 64] == (sum & 0xff) && pts[(size_t)i * 64 + 63] == (sum & 0xff));
        if (with_flags) CHECK(fl[i] == sum);
    }
}

int main() {
    CHECK(feldman_verify_dims_error(0, 5, 6, 1) && feldman_verify_dims_error(-1, 5, 6, 1));
    CHECK(feldman_verify_dims_error(3, 0, 6, 1) && feldman_verify_dims_error(3, -2, 6, 1));
    CHECK(feldman_verify_dims_error(3, 5, 0, 1) && feldman_verify_dims_error(3, 5, 33, 1) &&
          feldman_verify_dims_error(3, 5, -1, 1));
    CHECK(feldman_verify_dims_error(3, 5, 6, -1) && feldman_verify_dims_error(3, 5, 6, -0x7fffffff - 1));
    CHECK(feldman_verify_dims_error(3, 5, 6, (1 << 26) + 1) && feldman_verify_dims_error(3, 5, 6, 0x7fffffff));
    CHECK(feldman_verify_dims_error(1 << 14, (1 << 12) + 1, 6, 1));               // T x M above the limit
    CHECK(feldman_verify_dims_error(0x7fffffff, 0x7fffffff, 6, 1));               // ... and no overflow on the way
    CHECK(!feldman_verify_dims_error(1, 1, 1, 0) && !feldman_verify_dims_error(22, 60, 6, 3600) &&
          !feldman_verify_dims_error(3, 5, 32, 1 << 26) && !feldman_verify_dims_error(1 << 14, 1 << 12, 6, 1));
    CHECK(kFeldmanMaxRows == (size_t(1) << 26));
    const uint32_t dl[4] = {0, 4, 5, 9};
    CHECK(feldman_bad_dealer(dl, 4, 10) == -1 && feldman_bad_dealer(dl, 4, 9) == 3 && feldman_bad_dealer(dl, 4, 5) == 2 &&
          feldman_bad_dealer(dl, 2, 5) == -1 && feldman_bad_dealer(nullptr, 4, 1) == -1 && feldman_bad_dealer(dl, 0, 1) == -1);
    CHECK(feldman_verify_aligned(0x1000, 0x2010, 0x30f0) && feldman_verify_aligned(0x1000, 0x2010, 0));
    CHECK(!feldman_verify_aligned(0x1001, 0x2000, 0x3000) && !feldman_verify_aligned(0x1000, 0x2008, 0x3000) &&
          !feldman_verify_aligned(0x1000, 0x2000, 0x300f));
    const FeldmanVerifyBytes top = feldman_verify_bytes(1 << 14, 1 << 12, 1 << 26);  // no overflow at the limits
    CHECK(top.commitments == (size_t(1) << 32) && top.dealer == (size_t(1) << 28) && top.xs == (size_t(1) << 28) &&
          top.shares == (size_t(1) << 31) && top.ok == (size_t(1) << 26) && top.points == (size_t(1) << 32) &&
          top.flags == (size_t(1) << 28));
    const FeldmanVerifyBytes none = feldman_verify_bytes(3, 5, 0);
    CHECK(none.commitments == 3 * 5 * 64 && none.dealer == 0 && none.xs == 0 && none.shares == 0 && none.ok == 0 &&
          none.points == 0 && none.flags == 0);
    const int shapes[][3] = {{1, 1, 1}, {3, 5, 25}, {4, 6, 36}, {22, 60, 60}, {22, 60, 3600}, {3, 7, 63}, {3, 7, 64},
                             {3, 7, 65}, {2, 129, 129}};
    for (const auto &s : shapes) {
        CHECK(!feldman_verify_dims_error(s[0], s[1], 6, s[2]));
        for (int opt = 0; opt < 8; ++opt) through_bounce(s[0], s[1], s[2], opt & 1, opt & 2, opt & 4);
    }
    std::printf(failures ? "%d checks failed\n" : "feldman_args_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
