// gcm_args_check.cpp -- the host side of flm_aes_gcm_seal / flm_aes_gcm_open without a GPU, for the
// host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I flamingo_amd/csrc tools/gcm_args_check.cpp -o build/gcm_args_check && build/gcm_args_check
// It runs the argument rules (flm_deal_args.h) over accepted and refused calls, and for the accepted
// ones declares the call's arrays to the bounce-buffer layout (flm_host_layout.h) in the order the
// host-pointer entry points do -- keys, nonces, aad if any, in and out if any, tags, and open's ok --
// then copies every array into and out of a heap buffer of the size the layout returned, with the
// kernel replaced by a byte-wise stand-in.  A span placed past the buffer, or overlapping another,
// is then a sanitizer report or a failed check.
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

static void through_bounce(std::vector<HostSpan> spans, const std::vector<bool> &is_out) {
    CHECK(spans.size() <= 8);  // HostCopies' limit
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
    // ---- sizes
    CHECK(aes_gcm_auth_dims_error(13, 16, 32, 1) && aes_gcm_auth_dims_error(0, 16, 32, 1) &&
          aes_gcm_auth_dims_error(-16, 16, 32, 1) && aes_gcm_auth_dims_error(8, 0, 0, 0));
    CHECK(aes_gcm_auth_dims_error(16, 16, 257, 1) && aes_gcm_auth_dims_error(12, 0, (size_t)-1, 1));
    CHECK(aes_gcm_auth_dims_error(16, 65, 32, 1) && aes_gcm_auth_dims_error(16, (size_t)-1, 32, 1) &&
          aes_gcm_auth_dims_error(16, (size_t)(int)-4, 32, 1));
    CHECK(aes_gcm_auth_dims_error(16, 16, 32, -1) && aes_gcm_auth_dims_error(16, 16, 32, (1 << 26) + 1));
    CHECK(!aes_gcm_auth_dims_error(12, 0, 0, 0) && !aes_gcm_auth_dims_error(16, 64, 256, 1 << 26));
    CHECK(!aes_gcm_auth_dims_error(16, 0, 0, 1));   // a tag over nothing at all is still a tag
    CHECK(!aes_gcm_auth_dims_error(12, 16, 0, 1));  // len 0: a tag over the AAD alone
    CHECK(aes_gcm_dims_error(16, 0, 1));            // flm_aes_gcm_xor's own rule stands: len 0 refused
    // ---- arrays
    const uint8_t a = 0;
    const void *p = &a;
    for (bool open : {false, true}) {
        const void *ok = open ? p : nullptr;
        CHECK(!aes_gcm_auth_null_error(p, p, p, 16, p, p, 32, p, ok, open));
        CHECK(!aes_gcm_auth_null_error(p, p, nullptr, 0, p, p, 32, p, ok, open));
        CHECK(!aes_gcm_auth_null_error(p, p, p, 16, nullptr, nullptr, 0, p, ok, open));
        CHECK(aes_gcm_auth_null_error(nullptr, p, p, 16, p, p, 32, p, ok, open));
        CHECK(aes_gcm_auth_null_error(p, nullptr, p, 16, p, p, 32, p, ok, open));
        CHECK(aes_gcm_auth_null_error(p, p, nullptr, 16, p, p, 32, p, ok, open));  // aad_len without aad
        CHECK(aes_gcm_auth_null_error(p, p, p, 0, p, p, 32, p, ok, open));         // aad without aad_len
        CHECK(aes_gcm_auth_null_error(p, p, p, 16, nullptr, p, 32, p, ok, open));
        CHECK(aes_gcm_auth_null_error(p, p, p, 16, p, nullptr, 32, p, ok, open));
        CHECK(aes_gcm_auth_null_error(p, p, p, 16, p, p, 32, nullptr, ok, open));
    }
    CHECK(aes_gcm_auth_null_error(p, p, p, 16, p, p, 32, p, nullptr, true));  // open needs ok_out
    // ---- byte counts and the bounce layout
    const size_t lens[] = {0, 1, 15, 16, 17, 32, 33, 64, 256}, aads[] = {0, 1, 16, 20, 64};
    for (int nonce_len : {12, 16})
        for (size_t len : lens)
            for (size_t aad_len : aads)
                for (int n : {1, 65, 245760})
                    for (bool open : {false, true}) {
                        CHECK(!aes_gcm_auth_dims_error(nonce_len, aad_len, len, n));
                        const AesGcmAuthBytes nb = aes_gcm_auth_bytes(nonce_len, aad_len, len, n);
                        CHECK(nb.keys == (size_t)n * 16 && nb.nonces == (size_t)n * nonce_len && nb.aad == (size_t)n * aad_len &&
                              nb.data == (size_t)n * len && nb.tags == (size_t)n * 16 && nb.ok == (size_t)n);
                        if (nb.data >= kStageBytes) continue;  // 245,760 x 256 B streams through the ring instead
                        std::vector<HostSpan> spans = {{nb.keys, 1, false}, {nb.nonces, 1, false}};
                        std::vector<bool> is_out = {false, false};
                        if (aad_len) spans.push_back({nb.aad, 1, false}), is_out.push_back(false);
                        if (len) {
                            spans.push_back({nb.data, 1, true}), is_out.push_back(false);
                            spans.push_back({nb.data, 1, true}), is_out.push_back(true);
                        }
                        spans.push_back({nb.tags, 1, false}), is_out.push_back(!open);
                        if (open) spans.push_back({nb.ok, 1, false}), is_out.push_back(true);
                        through_bounce(spans, is_out);
                    }
    std::printf(failures ? "%d checks failed\n" : "gcm_args_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
