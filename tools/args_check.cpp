// args_check.cpp -- the host side of the calls that come in a host-pointer and a *_dev form, without a GPU, for
// the host sanitizers: the round path (flm_client_mask, flm_client_encode_mask, flm_decode_sum, flm_prg_expand,
// flm_mask_accumulate, flm_aggregate_unmask, flm_chacha20_xor, flm_rotate) and the batch crypto calls (flm_shamir_combine /
// _deal, flm_aes_gcm_xor / _seal / _open, flm_ecdsa_verify, flm_feldman_verify, flm_ec_combine, flm_ec_mul,
// hash to curve):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I flamingo_amd/csrc tools/args_check.cpp -o build/args_check && build/args_check
// It runs the argument rules (flm_call_args.h) over accepted and refused calls, and for the accepted
// ones takes the call's list of arrays -- the very list the host-pointer entry point declares to
// HostCopies -- through the bounce-buffer layout (flm_host_layout.h): every input copied into a heap
// buffer of the size the layout returned, a byte-wise stand-in for the kernel that reads every input
// byte and writes every output byte, every output copied out and compared.  A span placed past the
// buffer or overlapping another is then a sanitizer report or a failed check; so is a list that names
// one scratch buffer twice, for any combination of its optional arrays.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flm_call_args.h"
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

// n bytes at p all equal v
static bool all_bytes(const uint8_t *p, size_t n, uint8_t v) { return !n || (p[0] == v && !std::memcmp(p, p + 1, n - 1)); }

// One call's list through a heap "bounce buffer", as HostCopies::declare, begin() and finish() move it:
// rows x width bytes per array, row by row between the host rows at h_pitch and the bounce rows at the
// layout's pitch (the padded round_up(width, 16) in place, else packed).  Array i holds the byte i + 1
// on the way in and 0x80 + i on the way out, and the bounce buffer 0xEE wherever no array's bytes
// lie, so a span that overlaps another, or a row that runs into the next one's, loses bytes that the
// stand-in or the caller then misses.
static void through_bounce(const ArgList &l) {
    CHECK(l.n <= kMaxArgs && !names_slot_twice(l));
    std::vector<HostSpan> spans;
    std::vector<Arg> args;
    for (int i = 0; i < l.n; ++i)
        if (l.a[i].present) spans.push_back({l.a[i].width, l.a[i].rows, l.a[i].in_place}), args.push_back(l.a[i]);
    const size_t total = host_layout(spans.data(), (int)spans.size());
    std::vector<uint8_t> bounce(total, 0xEE);
    std::vector<std::vector<uint8_t>> host(spans.size());
    size_t end = 0;
    for (size_t i = 0; i < spans.size(); ++i) {
        const HostSpan &s = spans[i];
        const Arg &a = args[i];
        CHECK(s.route == (a.in_place ? kRouteInPlace : kRouteBounce));  // every shape here is below the staging size
        CHECK(s.pitch == (a.in_place ? (s.width + 15) / 16 * 16 : s.width));
        CHECK(a.h_pitch >= a.width && a.d_pitch >= a.width);
        CHECK(s.offset >= end && s.offset % 256 == 0);
        CHECK(s.offset + s.rows * s.pitch <= total);
        end = s.offset + s.rows * s.pitch;
        host[i].assign(a.rows * a.h_pitch, (uint8_t)(i + 1));
        if (a.is_out) continue;
        for (size_t r = 0; r < s.rows && s.width; ++r)  // inputs in
            std::memcpy(bounce.data() + s.offset + r * s.pitch, host[i].data() + r * a.h_pitch, s.width);
    }
    for (size_t i = 0; i < spans.size(); ++i)  // the kernel's stand-in: every input byte read ...
        for (size_t r = 0; r < spans[i].rows && !args[i].is_out; ++r)
            CHECK(all_bytes(bounce.data() + spans[i].offset + r * spans[i].pitch, spans[i].width, (uint8_t)(i + 1)));
    for (size_t i = 0; i < spans.size(); ++i)  // ... and every output byte written
        for (size_t r = 0; r < spans[i].rows && args[i].is_out && spans[i].width; ++r)
            std::memset(bounce.data() + spans[i].offset + r * spans[i].pitch, (int)(0x80 + i), spans[i].width);
    size_t held = 0;
    for (size_t i = 0; i < spans.size(); ++i) {  // outputs out; the inputs are still whole
        const HostSpan &s = spans[i];
        for (size_t r = 0; r < s.rows && s.width; ++r) {
            const uint8_t *b = bounce.data() + s.offset + r * s.pitch;
            if (args[i].is_out) std::memcpy(host[i].data() + r * args[i].h_pitch, b, s.width);
            CHECK(all_bytes(b, s.width, (uint8_t)(args[i].is_out ? 0x80 + i : i + 1)));
        }
        held += s.rows * s.width;
        if (args[i].is_out) CHECK(all_bytes(host[i].data(), host[i].size(), (uint8_t)(0x80 + i)));  // h_pitch == width here
    }
    size_t padding = 0;
    for (uint8_t b : bounce) padding += b == 0xEE;
    CHECK(padding == total - held);  // nothing written between the rows or the spans
}

static bool bytes_are(const ArgList &l, std::initializer_list<size_t> want) {
    if ((size_t)l.n != want.size()) return false;
    for (int i = 0; i < l.n; ++i)
        if (l.a[i].width != want.begin()[i]) return false;
    return true;
}

static void check_lists() {
    CHECK(kMaxRows == (size_t(1) << 26));
    const ArgList twice = {{arg_in(4, ec_in), arg_out(4, ec_out), arg_out(4, ec_in)}, 3};
    const ArgList absent = {{arg_in(4, ec_in), arg_out(4, ec_out), arg_out(4, ec_in, false)}, 3};
    CHECK(names_slot_twice(twice) && !names_slot_twice(absent));
    // every call, every combination of its optional arrays: no scratch buffer twice, and they pass the layout
    for (int opt = 0; opt < 8; ++opt) {
        through_bounce(ec_combine_args(3, 5, opt & 1, opt & 2, opt & 4));
        through_bounce(feldman_verify_args(3, 5, 25, opt & 1, opt & 2, opt & 4));
        through_bounce(aes_gcm_auth_args(12, opt & 1 ? 20 : 0, opt & 2 ? 33 : 0, 65, opt & 4));
        if (opt < 3) through_bounce(h2c_args(65, opt == 1, opt == 2));
    }
    through_bounce(shamir_combine_args(20, 4055));
    through_bounce(shamir_combine_args(0, 1));  // T = 0: the sum over nothing
    through_bounce(ec_mul_args(65));
    // the optional arrays are exactly the ones the flags name
    const ArgList f = feldman_verify_args(3, 5, 25, false, true, false), e = ecdsa_verify_args(7, false);
    CHECK(f.n == 7 && !f.a[1].present && f.a[5].present && !f.a[6].present && f.a[0].present && f.a[4].is_out);
    CHECK(e.n == 5 && !e.a[4].present && e.a[3].present && e.a[3].is_out && !e.a[2].is_out);
    const ArgList seal = aes_gcm_auth_args(12, 0, 0, 4, false), open = aes_gcm_auth_args(12, 1, 1, 4, true);
    CHECK(!seal.a[2].present && !seal.a[3].present && !seal.a[4].present && seal.a[5].is_out && !seal.a[6].present);
    CHECK(open.a[2].present && open.a[3].in_place && open.a[4].in_place && !open.a[5].is_out && open.a[6].is_out);
}

// The round path's lists: every combination of the optional arrays, at the GPU test's shapes (L = 1: a row
// below one 16-byte quad, 5: a quad and a tail, 1025) and one that fills whole 64-word pitches.
static void check_round_lists() {
    // a two-row, 20-byte span in place: rows at 32, the 12 bytes after each untouched
    const ArgList padded = {{in_place(pitched(arg_in(20, rows), 2, 256)), in_place(pitched(arg_out(20, out), 2, 256))}, 2};
    HostSpan sp[2] = {{20, 2, true}, {20, 2, true}};
    CHECK(host_layout(sp, 2) == 512 && sp[0].pitch == 32 && sp[1].offset == 256 && sp[1].route == kRouteInPlace);
    through_bounce(padded);
    for (size_t L : {size_t(1), size_t(5), size_t(64), size_t(1025)})
        for (size_t N : {size_t(1), size_t(3)})
            for (size_t K : {size_t(0), size_t(3)})
                for (int opt = 0; opt < 4; ++opt) {
                    through_bounce(client_encode_mask_args(N, K, L, L, opt & 1, false, opt & 2));
                    for (int pack : {2, 4}) {
                        through_bounce(client_encode_mask_args(N, K, L, packed_words(L, pack), opt & 1, false, opt & 2));
                        if (!opt) through_bounce(decode_unpack_args(L, packed_words(L, pack)));
                        if (opt < 2) through_bounce(decode_unpack_mod_args(L, packed_words(L, pack), opt & 1));
                    }
                    for (int pack : {1, 2, 4})
                        through_bounce(client_encode_mask_args(N, K, L, packed_words(L, pack), opt & 1, true, opt & 2));
                    for (int pack : {1, 2, 4})   // flm_client_encode_gauss_mask: the table after the noise seeds
                        for (size_t T : {size_t(2), size_t(74), size_t(1024)})
                            through_bounce(client_encode_gauss_mask_args(N, K, L, packed_words(L, pack), opt & 1, T, opt & 2));
                    if (opt < 2) through_bounce(client_mask_args(N, K, L, opt & 1));
                    if (opt < 2) through_bounce(aggregate_unmask_args(K, L, opt & 1));
                    if (opt) continue;
                    through_bounce(prg_expand_args(K, L));
                    through_bounce(mask_accumulate_args(K, L));
                    through_bounce(decode_unpack_args(L, L));
                    through_bounce(chacha20_xor_args(L));
                }
    // flm_rotate: forward L in and L_rot out, the inverse the other way round, with and without the counts
    for (size_t L : {size_t(1), size_t(15), size_t(16), size_t(17), size_t(4097)})
        for (int h : {4, 5, 12})
            for (size_t N : {size_t(1), size_t(3)})
                for (int opt = 0; opt < 2; ++opt) {
                    bool range = false;
                    uint64_t L_rot = 0;
                    CHECK(!rotate_error(L, h, &range, &L_rot) && L_rot % (1u << h) == 0 && L_rot >= L && L_rot - L < (1u << h));
                    through_bounce(rotate_args(N, L, L_rot, opt, false, false));
                    if (!opt) through_bounce(rotate_args(N, L_rot, L, false, false, false));
                    // flm_rotate_clip and flm_l2_clip: the optional outputs together or none of them
                    through_bounce(rotate_args(N, L, L_rot, opt, opt, opt));
                    through_bounce(l2_clip_args(N, L, opt, !opt));
                    through_bounce(round_select_args(N, L, opt ? 8 : 1));   // flm_round_select: nothing optional
                }
    const ArgList rs = round_select_args(3, 5, 4);
    CHECK(rs.n == 5 && rs.a[0].slot == rows && rs.a[0].in_place && !rs.a[0].is_out && rs.a[0].width == 20 && rs.a[0].rows == 3 &&
          rs.a[1].width == 3 * 4 * 32 && !rs.a[1].is_out && rs.a[2].is_out && rs.a[2].width == 3 * 4 * 8 && !rs.a[2].in_place &&
          rs.a[3].is_out && rs.a[3].width == 96 && rs.a[4].is_out && rs.a[4].width == 12 && !names_slot_twice(rs));
    const ArgList rc = rotate_args(3, 5, 16, true, true, false), lc = l2_clip_args(3, 5, false, true);
    CHECK(rc.n == 6 && rc.a[0].width == 20 && rc.a[1].width == 64 && rc.a[1].is_out && rc.a[3].present && rc.a[4].present &&
          rc.a[4].is_out && rc.a[4].width == 12 && rc.a[4].slot == ec_flags && !rc.a[5].present && !names_slot_twice(rc));
    CHECK(lc.n == 4 && lc.a[0].slot == rows && lc.a[1].slot == out && lc.a[1].in_place && lc.a[1].width == 20 && !lc.a[2].present &&
          lc.a[3].present && lc.a[3].is_out && lc.a[3].width == 24 && lc.a[3].slot == ec_dig && !names_slot_twice(lc));
    // the plain rotation: the clip's two outputs are in the list and absent
    const ArgList ro = rotate_args(3, 5, 16, true, false, false), ri = rotate_args(3, 16, 5, false, false, false);
    CHECK(ro.n == 6 && ro.a[0].slot == rows && ro.a[0].width == 20 && ro.a[0].rows == 3 && ro.a[0].in_place && !ro.a[0].is_out &&
          ro.a[1].slot == out && ro.a[1].width == 64 && ro.a[1].is_out && ro.a[1].in_place && ro.a[2].width == 32 &&
          ro.a[2].slot == seeds && ro.a[3].present && ro.a[3].is_out && ro.a[3].width == 12);
    CHECK(!ro.a[4].present && !ro.a[5].present && !ri.a[4].present && !ri.a[5].present && !names_slot_twice(ro));
    CHECK(ri.a[0].width == 64 && ri.a[1].width == 20 && !ri.a[3].present);
    // rows travel at the host forms' pitch; what is optional is exactly what the flags name
    const ArgList m = client_mask_args(3, 7, 5, false), e = client_encode_mask_args(3, 7, 5, 5, false, false, true);
    CHECK(host_row_pitch(1) == 256 && host_row_pitch(64) == 256 && host_row_pitch(65) == 512);
    CHECK(m.n == 4 && !m.a[0].present && m.a[3].is_out && m.a[3].in_place && m.a[3].rows == 3 && m.a[3].width == 20 &&
          m.a[3].h_pitch == 20 && m.a[3].d_pitch == 256 && m.a[1].width == 7 * 32 && m.a[2].width == 7);
    CHECK(e.n == 6 && e.a[0].present && !e.a[2].present && !e.a[3].present && e.a[5].present && e.a[5].is_out && e.a[5].width == 12);
    const ArgList z = client_mask_args(3, 0, 5, true);  // K = 0: seeds and signs declared, no bytes
    CHECK(z.a[1].present && z.a[2].present && !z.a[1].width && !z.a[2].width);
    CHECK(!aggregate_unmask_args(3, 5, false).a[2].present && aggregate_unmask_args(3, 5, true).a[2].width == 20);
    const ArgList acc = mask_accumulate_args(3, 1025);  // the rows first, the seeds after
    CHECK(acc.a[0].slot == rows && acc.a[1].slot == out && acc.a[1].is_out && acc.a[2].slot == seeds && acc.a[3].slot == signs);
}

// The codec's one rule as the three families of entry points call it: unpacked, packed (pack = 1 not admitted), noised.
static const char *unpacked_rule(int f, float clip, int64_t n, bool *range) { return codec_error(f, clip, 1, true, 0, n, 0, range); }
static const char *packed_rule(int f, float clip, int pack, int64_t n, bool *range, uint32_t *B) {
    return codec_error(f, clip, pack, false, 0, n, 0, range, B);
}
static const char *noise_rule(int f, float clip, int pack, int b, int64_t n, uint64_t L, bool *range, uint32_t *B, uint32_t *Bn) {
    return codec_error(f, clip, pack, true, b, n, L, range, B, Bn);
}

// The round path's rules at their edges.
static void check_round_rules() {
    int64_t K = -1;
    const int64_t seg_ok[4] = {0, 0, 2, 3}, seg_from1[2] = {1, 1}, seg_down[4] = {0, 2, 1, 3};
    const int64_t seg_max[2] = {0, 0x7fffffff}, seg_over[2] = {0, 0x80000000ll};
    const int8_t sg[3] = {1, -1, 1}, sg0[3] = {1, 0, 1}, sg2[3] = {1, 1, 2};
    CHECK(!seg_signs_error(3, seg_ok, sg, &K) && K == 3);
    CHECK(seg_signs_error(3, nullptr, sg, &K) && seg_signs_error(1, seg_from1, sg, &K) && seg_signs_error(3, seg_down, sg, &K));
    CHECK(seg_signs_error(3, seg_ok, nullptr, &K) && seg_signs_error(3, seg_ok, sg0, &K) && seg_signs_error(3, seg_ok, sg2, &K));
    CHECK(!seg_signs_error(2, seg_ok, sg2, &K) && K == 2);      // the first two clients: two seeds, signs[2] not read
    CHECK(!seg_signs_error(1, seg_ok, nullptr, &K) && K == 0);  // the first alone: none, and no signs needed
    // K = 2^31 - 1 passes the count (its signs are then read: none given here), 2^31 does not
    CHECK(std::strcmp(seg_signs_error(1, seg_max, nullptr, &K), "NULL seeds/signs") == 0);
    CHECK(std::strcmp(seg_signs_error(1, seg_over, nullptr, &K), "too many seeds") == 0);
    CHECK(!client_args_error(true, 3, seg_ok, sg, sg, &K) && client_args_error(false, 3, seg_ok, sg, sg, &K) &&
          client_args_error(true, 3, seg_ok, nullptr, sg, &K) && !client_args_error(true, 1, seg_ok, nullptr, nullptr, &K));
    // pitch = round_up(L, 4) and one less
    for (size_t L : {size_t(1), size_t(4), size_t(5), size_t(1025)}) {
        const size_t p = round_up(L, 4);
        CHECK(!row_pitch_error(p, L) && !row_pitch_error(p + 4, L) && row_pitch_error(p - 1, L) && row_pitch_error(p + 1, L));
        CHECK(p < 4 || row_pitch_error(p - 4, L));
    }
    CHECK(row_pitch_error(5, 5) && row_pitch_error(0, 1));
    alignas(16) static uint8_t buf[32];
    CHECK(!align16_error({buf, buf + 16, nullptr}) && align16_error({buf + 8}) && align16_error({buf, buf + 1}) &&
          align16_error({nullptr, buf + 24}) && !align16_error({}));
    CHECK(std::strstr(align16_error({buf + 8}), "16-byte aligned"));
    // the L2 calls' doubles at 8 bytes and factors at 4; NULL passes; without doubles the text names the factors alone
    CHECK(!l2_factors_align_error(buf + 8, nullptr, buf + 4) && !align4_error(buf + 12) && !align4_error(nullptr) &&
          l2_factors_align_error(buf, buf + 4, buf) && l2_factors_align_error(buf, nullptr, buf + 2) && align4_error(buf + 1));
    CHECK(!std::strcmp(l2_factors_align_error(buf + 4, nullptr, buf),
                       "work and sumsq must be 8-byte aligned, factors 4-byte aligned"));
    CHECK(!std::strcmp(align4_error(buf + 2), "factors must be 4-byte aligned"));
    // frac_bits 0, 30, 31; the clip; n ceil(clip 2^f) exactly 2^31 - 1 and one more
    bool range = true;
    CHECK(!unpacked_rule(0, 1.0f, 1, &range) && !range && !unpacked_rule(30, 1.0f, 1, &range) && !range);
    CHECK(unpacked_rule(31, 1.0f, 1, &range) && !range && unpacked_rule(-1, 1.0f, 1, &range) && !range);
    CHECK(unpacked_rule(16, 0.0f, 1, &range) && !range && unpacked_rule(16, -1.0f, 1, &range) && !range);
    CHECK(unpacked_rule(16, INFINITY, 1, &range) && !range && unpacked_rule(16, NAN, 1, &range) && !range);
    CHECK(unpacked_rule(16, 1.0f, 0, &range) && !range);
    CHECK(!unpacked_rule(0, 1.0f, 2147483647, &range) && !range);                       // n x 1 = 2^31 - 1
    CHECK(unpacked_rule(0, 1.0f, 2147483648ll, &range) && range);                       // ... and one more
    CHECK(!unpacked_rule(16, 0.5f, 65535, &range) && !range);                           // 65535 x 2^15 < 2^31 - 1
    CHECK(unpacked_rule(16, 0.5f, 65536, &range) && range);                             // 2^31
    CHECK(!unpacked_rule(4, 1.01f, 126322567, &range) && unpacked_rule(4, 1.01f, 126322568, &range) && range);  // m = 17
    CHECK(!unpacked_rule(30, 1.9999999f, 1, &range) && unpacked_rule(30, 2.0f, 1, &range) && range);  // m alone past 2^31 - 1
    // the packed codec: pack, then the unpacked rule's refusals, then n 2B <= 2^W - 1 at its edges
    uint32_t B = 0;
    for (int pack : {0, 1, 3, 8, -2}) CHECK(packed_rule(7, 1.0f, pack, 1, &range, &B) && !range);
    CHECK(packed_rule(31, 1.0f, 2, 1, &range, &B) && !range && packed_rule(7, 0.0f, 2, 1, &range, &B) && !range);
    CHECK(packed_rule(7, 1.0f, 2, 0, &range, &B) && !range);
    CHECK(!packed_rule(7, 1.0f, 2, 255, &range, &B) && !range && B == 128);
    CHECK(packed_rule(7, 1.0f, 2, 256, &range, &B) && range);
    CHECK(!packed_rule(4, 1.0f, 2, 2047, &range, &B) && B == 16 && packed_rule(4, 1.0f, 2, 2048, &range, &B) && range);
    CHECK(!packed_rule(2, 1.0f, 4, 31, &range, &B) && B == 4 && packed_rule(2, 1.0f, 4, 32, &range, &B) && range);
    CHECK(!packed_rule(0, 1.0f, 4, 127, &range, &B) && B == 1 && packed_rule(0, 1.0f, 4, 128, &range, &B) && range);
    CHECK(!packed_rule(6, 1.9f, 4, 1, &range, &B) && B == 122);                 // 244 <= 255
    CHECK(packed_rule(7, 1.0f, 4, 1, &range, &B) && range);                      // 2B = 256 alone past 2^8 - 1
    CHECK(packed_rule(30, 2.0f, 2, 1, &range, &B) && range);                     // the unpacked rule's refusal first
    CHECK(packed_words(1, 2) == 1 && packed_words(2, 2) == 1 && packed_words(3, 2) == 2 && packed_words(5, 4) == 2 &&
          packed_words(0, 4) == 0);
    const ArgList pe = client_encode_mask_args(3, 7, 5, 2, false, false, true), pd = decode_unpack_args(5, 2);
    CHECK(pe.n == 6 && pe.a[0].width == 20 && pe.a[4].width == 8 && pe.a[4].is_out && pe.a[4].in_place && !pe.a[2].present &&
          !pe.a[3].present);
    CHECK(pd.n == 2 && pd.a[0].width == 8 && pd.a[1].width == 20 && pd.a[1].is_out);
    // the noised codec: pack and noise_bits, then the rule of that pack, then the worst case with B_n = B + b / 2
    uint32_t Bn = 0;
    for (int b : {-2, 1, 31, 1026}) CHECK(noise_rule(4, 1.0f, 2, b, 1, 0, &range, &B, &Bn) && !range);
    for (int pack : {0, 3, 8}) CHECK(noise_rule(4, 1.0f, pack, 2, 1, 0, &range, &B, &Bn) && !range);
    CHECK(!noise_rule(4, 1.0f, 2, 30, 1057, 0, &range, &B, &Bn) && B == 16 && Bn == 31);
    CHECK(noise_rule(4, 1.0f, 2, 30, 1058, 0, &range, &B, &Bn) && range);
    CHECK(!noise_rule(2, 1.0f, 4, 2, 25, 0, &range, &B, &Bn) && Bn == 5 && noise_rule(2, 1.0f, 4, 2, 26, 0, &range, &B, &Bn) && range);
    CHECK(!noise_rule(7, 1.0f, 2, 0, 255, 0, &range, &B, &Bn) && noise_rule(7, 1.0f, 2, 2, 255, 0, &range, &B, &Bn) && range);
    CHECK(!noise_rule(16, 4.0f, 1, 1024, 8176, 0, &range, &B, &Bn) && Bn == 262656);  // 8176 * 262656 <= 2^31 - 1
    CHECK(noise_rule(16, 4.0f, 1, 1024, 8177, 0, &range, &B, &Bn) && range);
    CHECK(!noise_rule(16, 4.0f, 1, 0, 8177, 0, &range, &B, &Bn));                     // without noise: 8191 fit
    CHECK(!noise_rule(4, 1.0f, 1, 64, 1, 1ull << 35, &range, &B, &Bn));              // 2 * 2^31 blocks
    CHECK(noise_rule(4, 1.0f, 1, 64, 1, (1ull << 35) + 1, &range, &B, &Bn) && range);
    CHECK(!noise_rule(4, 1.0f, 1, 0, 1, ~0ull, &range, &B, &Bn));                    // no noise: no length rule
    const ArgList ne = client_encode_mask_args(3, 7, 5, 2, false, true, true);
    CHECK(ne.n == 6 && ne.a[3].present && ne.a[3].width == 96 && !ne.a[2].present && ne.a[4].is_out && ne.a[4].width == 8);
    // the table mode: tail 1..512, the codec's own refusals, B_n = B + tail (the binomial edges at tail = b / 2), the
    // stream of two blocks per parameter block, the table's order and the device pointer's alignment
    for (int t : {0, -1, 513}) CHECK(!std::strcmp(codec_gauss_error(4, 1.0f, 2, t, 1, 0, &range), "tail must be in 1..512") && !range);
    for (int pack : {0, 3, 8}) CHECK(codec_gauss_error(4, 1.0f, pack, 1, 1, 0, &range) && !range);
    CHECK(codec_gauss_error(31, 1.0f, 2, 1, 1, 0, &range) && !range && codec_gauss_error(4, 0.0f, 2, 1, 1, 0, &range) && !range);
    CHECK(!codec_gauss_error(4, 1.0f, 2, 15, 1057, 0, &range, &B, &Bn) && B == 16 && Bn == 31 && !range);
    CHECK(codec_gauss_error(4, 1.0f, 2, 15, 1058, 0, &range) && range);
    CHECK(!codec_gauss_error(2, 1.0f, 4, 1, 25, 0, &range, &B, &Bn) && Bn == 5 && codec_gauss_error(2, 1.0f, 4, 1, 26, 0, &range) && range);
    CHECK(codec_gauss_error(7, 1.0f, 2, 1, 255, 0, &range) && range);
    CHECK(!codec_gauss_error(16, 4.0f, 1, 512, 8176, 0, &range, &B, &Bn) && Bn == 262656);
    CHECK(codec_gauss_error(16, 4.0f, 1, 512, 8177, 0, &range) && range);
    CHECK(!codec_gauss_error(4, 1.0f, 1, 1, 1, 1ull << 35, &range) && !codec_gauss_error(4, 1.0f, 1, 512, 1, 1ull << 35, &range));
    CHECK(codec_gauss_error(4, 1.0f, 1, 1, 1, (1ull << 35) + 1, &range) && range);
    const uint64_t up[4] = {0, 5, 5, ~0ull}, down[4] = {0, 5, 4, 9};
    CHECK(!dgauss_table_error(up, 2) && !dgauss_table_error(up, 1) && !dgauss_table_error(down, 1));
    CHECK(!std::strcmp(dgauss_table_error(down, 2), "the table must be non-decreasing"));
    CHECK(dgauss_table_error(nullptr, 2) && dgauss_table_error(up, 0) && dgauss_table_error(up, 513));
    CHECK(!cdt_align_error(buf + 8) && !cdt_align_error(nullptr) && !std::strcmp(cdt_align_error(buf + 4), "cdt must be 8-byte aligned"));
    const ArgList ge = client_encode_gauss_mask_args(3, 7, 5, 2, false, 64, true);
    CHECK(ge.n == 7 && ge.a[3].present && ge.a[3].width == 96 && ge.a[4].width == 512 && ge.a[4].slot == ec_dig && !ge.a[4].is_out &&
          !ge.a[2].present && ge.a[5].is_out && ge.a[5].in_place && ge.a[5].width == 8 && ge.a[6].is_out && !names_slot_twice(ge));
    // the decode modulo the field: the codec's own refusals, pack 2 or 4 alone, then one contributor's field and the
    // count (both FLM_ERANGE); n B_n is free: every cohort the worst-case rule stops one short of is admitted
    for (int pack : {0, 1, 3, 8, -2}) CHECK(modular_error(4, 1.0f, pack, 0, 1, &range) && !range);
    for (int b : {-2, 1, 31, 1026}) CHECK(modular_error(4, 1.0f, 2, b, 1, &range) && !range);
    CHECK(modular_error(31, 1.0f, 2, 0, 1, &range) && !range && modular_error(-1, 1.0f, 2, 0, 1, &range) && !range);
    for (float c : {0.0f, -1.0f, INFINITY, NAN}) CHECK(modular_error(4, c, 2, 0, 1, &range) && !range);
    CHECK(modular_error(4, 1.0f, 2, 0, 0, &range) && !range && modular_error(4, 1.0f, 2, 0, -5, &range) && !range);
    CHECK(!modular_error(7, 1.0f, 2, 0, 256, &range, &Bn) && Bn == 128 && !range);          // the packed rule stops at 255
    CHECK(!modular_error(4, 1.0f, 2, 30, 1058, &range, &Bn) && Bn == 31 && !modular_error(4, 1.0f, 2, 64, 4096, &range, &Bn) && Bn == 48);
    CHECK(!modular_error(2, 1.0f, 4, 2, 26, &range, &Bn) && Bn == 5 && !modular_error(7, 1.0f, 2, 2, 255, &range, &Bn) && Bn == 129);
    CHECK(!modular_error(0, 1.0f, 4, 4, 2147483647ll, &range, &Bn) && Bn == 3 && !range);   // n B_n past 2^32
    CHECK(modular_error(0, 1.0f, 4, 4, 2147483648ll, &range) && range);
    CHECK(!modular_error(6, 1.9f, 4, 10, 1, &range, &Bn) && Bn == 127);                      // 254 <= 255
    CHECK(modular_error(6, 1.9f, 4, 12, 1, &range) && range && modular_error(7, 1.0f, 4, 0, 1, &range) && range);
    CHECK(!modular_error(14, 1.0f, 2, 1024, 1, &range, &Bn) && Bn == 16896);                 // 33792 <= 65535
    CHECK(modular_error(15, 1.0f, 2, 0, 1, &range) && range && modular_error(30, 2.0f, 2, 0, 1, &range) && range);
    // ... its guard in 1..H and its L within 32 bits; out may not overlap sum
    CHECK(!modular_decode_error(2, 1, 5, &range) && !modular_decode_error(2, 32768, 5, &range) && !modular_decode_error(4, 128, 0, &range));
    CHECK(modular_decode_error(2, 0, 5, &range) && !range && modular_decode_error(2, 32769, 5, &range) && !range);
    CHECK(modular_decode_error(4, 129, 5, &range) && !range && modular_decode_error(4, -1, 5, &range) && !range);
    CHECK(!modular_decode_error(2, 1, 0xFFFFFFFFull, &range) && modular_decode_error(2, 1, 0x100000000ull, &range) && range);
    CHECK(modular_alias_error(buf, buf, 8, 2) && modular_alias_error(buf + 16, buf, 8, 2) && modular_alias_error(buf, buf + 12, 8, 2));
    CHECK(!modular_alias_error(buf, buf + 16, 8, 2) && !modular_alias_error(buf + 16, buf, 4, 4) && modular_alias_error(buf + 16, buf, 5, 4));
    const ArgList md = decode_unpack_mod_args(5, 2, true), mn = decode_unpack_mod_args(5, 2, false);
    CHECK(md.n == 3 && md.a[0].width == 8 && md.a[0].in_place && md.a[1].width == 20 && md.a[1].is_out && md.a[1].in_place &&
          md.a[2].present && md.a[2].is_out && !md.a[2].in_place && md.a[2].width == 8 && md.a[2].slot == ec_flags &&
          !mn.a[2].present && !names_slot_twice(md));
    CHECK(!decode_error(0, 1) && !decode_error(30, 1) && decode_error(31, 1) && decode_error(-1, 1) && decode_error(16, 0));
    // the rotation's rule: h in 4..12, L > 0, L_rot = round_up(L, 2^h), L_rot / 32 sign words within 2^36 PRG slots
    uint64_t L_rot = 0;
    for (int h : {3, 13, 0, -1}) CHECK(rotate_error(100, h, &range, &L_rot) && !range);
    CHECK(rotate_error(0, 4, &range, &L_rot) && !range);
    CHECK(!rotate_error(1, 4, &range, &L_rot) && L_rot == 16 && !rotate_error(16, 4, &range, &L_rot) && L_rot == 16);
    CHECK(!rotate_error(17, 4, &range, &L_rot) && L_rot == 32 && !rotate_error(4001, 5, &range, &L_rot) && L_rot == 4032);
    CHECK(!rotate_error(4097, 12, &range, &L_rot) && L_rot == 8192 && !range);
    CHECK(!rotate_error(1ull << 41, 12, &range, &L_rot) && L_rot == 1ull << 41);          // 2^36 words exactly
    CHECK(!rotate_error((1ull << 41) - 4095, 12, &range, &L_rot) && L_rot == 1ull << 41);
    CHECK(rotate_error((1ull << 41) + 1, 4, &range, &L_rot) && range && rotate_error(~0ull, 12, &range, &L_rot) && range);
    CHECK(rotate_error(~0ull, 3, &range, &L_rot) && !range);                               // the block before the length
    CHECK(rotate_sign_words(16) == 1 && rotate_sign_words(32) == 1 && rotate_sign_words(48) == 2);
    CHECK(!rotate_launch_error(0x7fffffffull) && rotate_launch_error(0x80000000ull));
    // the L2 clip's rule: L > 0, N >= 1, a finite positive radius, N ceil(L / 4096) <= 2^31 - 1 tiles
    uint64_t work = 0;
    CHECK(!l2_clip_error(1, 1.0f, 1, &range, &work) && work == 1 && !l2_clip_error(4097, 0.5f, 3, &range, &work) && work == 6);
    CHECK(l2_clip_error(0, 1.0f, 1, &range, &work) && !range && l2_clip_error(5, 1.0f, 0, &range, &work) && !range);
    for (float c : {0.0f, -1.0f, INFINITY, NAN}) CHECK(l2_clip_error(5, c, 1, &range, &work) && !range);
    CHECK(!l2_clip_error(4096ull * 0x7fffffffull, 1.0f, 1, &range, &work) && work == 0x7fffffffull);
    CHECK(l2_clip_error(4096ull * 0x7fffffffull + 1, 1.0f, 1, &range, &work) && range);
    CHECK(l2_clip_error(~0ull, 1.0f, 1, &range, &work) && range && l2_clip_error(~0ull, 1.0f, 0, &range, &work) && !range);
    CHECK(l2_clip_error(4096ull << 20, 1.0f, 2048, &range, &work) && range);
    // conditional rounding's rule: L > 0, attempts in 1..8, the codec's rule for one client, L B^2 <= 2^64 - 1 and
    // ceil(L / 16) <= 2^32 (both FLM_ERANGE)
    CHECK(!round_error(4096, 7, 1.0f, 4, &range) && !range && !round_error(1, 0, 1000.0f, 1, &range) && !round_error(5, 30, 1.0f, 8, &range));
    CHECK(round_error(0, 7, 1.0f, 4, &range) && !range && round_error(5, 7, 1.0f, 0, &range) && !range && round_error(5, 7, 1.0f, 9, &range) && !range);
    CHECK(round_error(5, 31, 1.0f, 1, &range) && !range && round_error(5, 7, NAN, 1, &range) && !range && round_error(5, 30, 4.0f, 1, &range) && range);
    CHECK(!round_error(15, 30, 1.0f, 1, &range) && round_error(16, 30, 1.0f, 1, &range) && range);            // 16 2^60 = 2^64
    CHECK(!round_error(1ull << 36, 13, 1.0f, 1, &range) && round_error(1ull << 36, 14, 1.0f, 1, &range) && range);
    CHECK(!round_error(1ull << 36, 0, 1.0f, 8, &range) && round_error((1ull << 36) + 1, 0, 1.0f, 8, &range) && range);
    CHECK(round_error(~0ull, 0, 1.0f, 1, &range) && range);                                                  // B = 1: the block counter's
    CHECK(!round_launch_error(1, 4096ull * 0x7fffffffull) && round_launch_error(1, 4096ull * 0x7fffffffull + 1) &&
          round_launch_error(2048, 4096ull << 20) && !round_launch_error(0, ~0ull));
    // ... and its bound: float64 in a fixed order, FLM_ERANGE from 2^63
    uint64_t bound = 7;
    CHECK(!round_bound_error(1.0f, 0, 1, 0.0, &range, &bound) && bound == 1);       // s = 1 + 2^-19: min(4.000004, 1.250004)
    CHECK(!round_bound_error(2.28125f, 7, 4096, 1.0, &range, &bound) && bound > 292ull * 292 && bound < 356ull * 356);
    for (float c : {0.0f, -1.0f, INFINITY, NAN}) CHECK(round_bound_error(c, 7, 16, 1.0, &range, &bound) && !range);
    CHECK(round_bound_error(1.0f, -1, 16, 1.0, &range, &bound) && round_bound_error(1.0f, 31, 16, 1.0, &range, &bound) &&
          round_bound_error(1.0f, 7, 0, 1.0, &range, &bound) && round_bound_error(1.0f, 7, 16, -1.0, &range, &bound) &&
          round_bound_error(1.0f, 7, 16, NAN, &range, &bound) && round_bound_error(1.0f, 7, 16, INFINITY, &range, &bound) && !range);
    CHECK(round_bound_error(4.0f, 30, 1, 0.0, &range, &bound) && range && !round_bound_error(2.0f, 30, 1, 0.0, &range, &bound) && !range);
    CHECK(!slot0_error(0) && !slot0_error(16) && slot0_error(8) && slot0_error(1) && !slot0_error(1ull << 36));
    CHECK(!slot_range_error(0, 1ull << 36) && slot_range_error(16, 1ull << 36) && slot_range_error(1ull << 36, 1) &&
          !slot_range_error(1ull << 36, 0) && slot_range_error(~0ull, 2));
    CHECK(!prg_expand_error(buf, buf, 16) && prg_expand_error(nullptr, buf, 16) && prg_expand_error(buf, nullptr, 16) &&
          prg_expand_error(buf, buf, 8));
    CHECK(!encode_mask_launch_error(0x7fffffffull) && encode_mask_launch_error(0x80000000ull));
    CHECK(prg_expand_units(3, 1025) == 6 && !prg_expand_launch_error(0x7fffffff, 2048) &&
          prg_expand_launch_error(0x7fffffff, 2049) && !prg_expand_launch_error(1, 0xFFFFFFFFull * 1024));
    // the round's own: codes as the order of the checks gives them
    CHECK(!aggregate_error(buf, 8, 1, 0, 5, 0, 5, 0, buf + 16, &range) && !range);
    CHECK(aggregate_error(buf, 4, 1, 0, 5, 0, 5, 0, buf + 16, &range) && !range);       // pitch below round_up(L, 4)
    CHECK(!aggregate_error(nullptr, 0, 0, 0, 5, 0, 5, 0, buf, &range));                 // no rows: no pitch, no pointer
    CHECK(std::strstr(aggregate_error(buf + 8, 8, 1, 0, 5, 0, 5, 0, buf, &range), "16-byte aligned"));
    CHECK(aggregate_error(buf, 8, 1, 0, 5, 0, 6, 0, buf, &range) && aggregate_error(buf, 8, 1, 0, 5, 3, 2, 0, buf, &range));
    CHECK(aggregate_error(buf, 8, 1, 0, 5, 0, 5, 8, buf, &range) && !range);
    CHECK(aggregate_error(buf, 8, 1, 0, 5, 0, 5, 1ull << 36, buf, &range) && range);
    CHECK(aggregate_error(buf, 8, 1, 0, 5, 0, 5, 1ull << 36, nullptr, &range) && range);  // the range before the NULL
    CHECK(aggregate_error(buf, 8, 1, 0, 5, 0, 5, 0, nullptr, &range) && !range && aggregate_error(nullptr, 8, 1, 0, 5, 0, 5, 0, buf, &range));
    CHECK(aggregate_error(buf, 8, -1, 0, 5, 0, 5, 0, buf, &range) && aggregate_error(buf, 8, 1, -1, 5, 0, 5, 0, buf, &range));
}

static void check_deal() {
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
        const ArgList l = shamir_deal_args(d[0], d[1], d[2]);
        CHECK(bytes_are(l, {(size_t)d[0] * d[1] * 32, (size_t)d[2] * 4, (size_t)d[2] * d[1] * 32}));
        through_bounce(l);
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
                const ArgList l = aes_gcm_xor_args(nonce_len, len, n);
                CHECK(bytes_are(l, {(size_t)n * 16, (size_t)n * nonce_len, (size_t)n * len, (size_t)n * len}));
                if ((size_t)n * len >= kStageBytes) continue;  // 245,760 x 256 B streams through the ring instead
                through_bounce(l);
            }
}

static void check_gcm() {
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
                        const ArgList l = aes_gcm_auth_args(nonce_len, aad_len, len, n, open);
                        CHECK(bytes_are(l, {(size_t)n * 16, (size_t)n * nonce_len, (size_t)n * aad_len, (size_t)n * len,
                                            (size_t)n * len, (size_t)n * 16, (size_t)n}));
                        if ((size_t)n * len >= kStageBytes) continue;  // 245,760 x 256 B streams through the ring instead
                        through_bounce(l);
                    }
}

static void check_ecdsa() {
    CHECK(ecdsa_verify_dims_error(-1) && ecdsa_verify_dims_error(-0x7fffffff - 1));
    CHECK(ecdsa_verify_dims_error((1 << 26) + 1) && ecdsa_verify_dims_error(0x7fffffff));
    CHECK(!ecdsa_verify_dims_error(0) && !ecdsa_verify_dims_error(1) && !ecdsa_verify_dims_error(61));
    CHECK(!ecdsa_verify_dims_error(1 << 26));  // exactly the EC size limit
    CHECK(ecdsa_verify_aligned(0x1000, 0x2010, 0x30f0));
    CHECK(!ecdsa_verify_aligned(0x1001, 0x2000, 0x3000) && !ecdsa_verify_aligned(0x1000, 0x2008, 0x3000) &&
          !ecdsa_verify_aligned(0x1000, 0x2000, 0x300f));
    // no overflow at the limit
    CHECK(bytes_are(ecdsa_verify_args(1 << 26, true),
                    {size_t(1) << 32, size_t(1) << 31, size_t(1) << 32, size_t(1) << 26, size_t(1) << 28}));
    CHECK(bytes_are(ecdsa_verify_args(0, true), {0, 0, 0, 0, 0}));
    for (int n : {1, 2, 61, 63, 64, 65, 255, 256, 257, 3660, 4096, 245760}) {
        CHECK(!ecdsa_verify_dims_error(n));
        CHECK(bytes_are(ecdsa_verify_args(n, true), {(size_t)n * 64, (size_t)n * 32, (size_t)n * 64, (size_t)n, (size_t)n * 4}));
        through_bounce(ecdsa_verify_args(n, true));
        through_bounce(ecdsa_verify_args(n, false));
    }
}

static void check_feldman() {
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
    const uint32_t dl[4] = {0, 4, 5, 9};
    CHECK(feldman_bad_dealer(dl, 4, 10) == -1 && feldman_bad_dealer(dl, 4, 9) == 3 && feldman_bad_dealer(dl, 4, 5) == 2 &&
          feldman_bad_dealer(dl, 2, 5) == -1 && feldman_bad_dealer(nullptr, 4, 1) == -1 && feldman_bad_dealer(dl, 0, 1) == -1);
    CHECK(feldman_verify_aligned(0x1000, 0x2010, 0x30f0) && feldman_verify_aligned(0x1000, 0x2010, 0));
    CHECK(!feldman_verify_aligned(0x1001, 0x2000, 0x3000) && !feldman_verify_aligned(0x1000, 0x2008, 0x3000) &&
          !feldman_verify_aligned(0x1000, 0x2000, 0x300f));
    // no overflow at the limits
    CHECK(bytes_are(feldman_verify_args(1 << 14, 1 << 12, 1 << 26, true, true, true),
                    {size_t(1) << 32, size_t(1) << 28, size_t(1) << 28, size_t(1) << 31, size_t(1) << 26, size_t(1) << 32,
                     size_t(1) << 28}));
    CHECK(bytes_are(feldman_verify_args(3, 5, 0, true, true, true), {3 * 5 * 64, 0, 0, 0, 0, 0, 0}));
    const int shapes[][3] = {{1, 1, 1}, {3, 5, 25}, {4, 6, 36}, {22, 60, 60}, {22, 60, 3600}, {3, 7, 63}, {3, 7, 64},
                             {3, 7, 65}, {2, 129, 129}};
    for (const auto &s : shapes) {
        CHECK(!feldman_verify_dims_error(s[0], s[1], 6, s[2]));
        for (int opt = 0; opt < 8; ++opt) through_bounce(feldman_verify_args(s[0], s[1], s[2], opt & 1, opt & 2, opt & 4));
        // a dealer array the rule lets through reads inside the T x M commitments, as a row's lane does
        const int T = s[0], M = s[1], n = s[2];
        std::vector<uint32_t> dealer(n);
        for (int i = 0; i < n; ++i) dealer[i] = (uint32_t)((i * 5 + 2) % M);
        CHECK(feldman_bad_dealer(dealer.data(), n, M) == -1);
        const std::vector<uint8_t> com(feldman_verify_args(T, M, n, true, true, true).a[0].width, 1);
        uint32_t sum = 0;
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < T; ++k) sum += com[((size_t)k * M + dealer[i]) * 64 + 63];
        CHECK(sum == (uint32_t)n * T);
    }
}

int main() {
    check_lists();
    check_round_lists();
    check_round_rules();
    check_deal();
    check_gcm();
    check_ecdsa();
    check_feldman();
    std::printf(failures ? "%d checks failed\n" : "args_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
