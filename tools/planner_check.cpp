// planner_check.cpp -- the HIP-free half of the host runtime without a GPU or the library, for the
// host sanitizers:
//   c++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I flamingo_amd/csrc tools/planner_check.cpp -o build/planner_check && build/planner_check
//   c++ -std=c++17 -g -pthread -fsanitize=thread \
//       -I flamingo_amd/csrc tools/planner_check.cpp -o build/planner_check_tsan && build/planner_check_tsan copies
// ("copies" runs the CopyPool part alone.)  It plans aggregate rounds and client-mask calls with
// flm_planner.h and checks, slot by slot, that the items cover what the call asked for exactly once
// and stay inside the arrays; checks the pure rules (slot range, kernel variant, small-round width)
// against values written out here; cuts copies into staging pieces (flm_host_layout.h); and runs
// CopyPool::copy2d (flm_copy_pool.h) on real buffers with its worker threads.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "flm_copy_pool.h"
#include "flm_host_layout.h"
#include "flm_planner.h"

using namespace flm;
using namespace flm::plan;
using flm::rt::CopyPool;
using flm::rt::kStageBytes;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// ------------------------------------------------------------------ aggregate rounds
struct Round {
    int N, K;
    uint64_t L, lo, hi;
    int pairing, subtiles;
};

// [a, b) sub-ranges recorded per tile start: they must partition [0, n), and one tile has one width
struct TileParts {
    uint32_t valid = 0;
    std::vector<std::pair<uint32_t, uint32_t>> parts;
};
static void check_partition(std::map<uint64_t, TileParts> &tiles, uint32_t n) {
    for (auto &kv : tiles) {
        auto &p = kv.second.parts;
        std::sort(p.begin(), p.end());
        CHECK(p.front().first == 0 && p.back().second == n);
        for (size_t i = 1; i < p.size(); ++i) CHECK(p[i].first == p[i - 1].second);
    }
}

static void check_round(const Round &r) {
    const uint64_t pitch = (r.L + 63) / 64 * 64, slot0 = 4096;
    std::vector<Item> items;
    const PlanShape shape = build_aggregate_items(r.subtiles, r.pairing, pitch, r.N, r.K, r.L, r.lo, r.hi, slot0, items);
    CHECK(shape.subtiles == 1 || shape.subtiles == 4 || shape.subtiles == 16);
    if (r.subtiles > 0) CHECK(shape.subtiles == r.subtiles);
    std::vector<uint32_t> rows(r.L, 0), seeds(r.L, 0), bias(r.L, 0), writers(r.L, 0);
    std::map<uint64_t, TileParts> row_tiles, mask_tiles;
    for (const Item &it : items) {
        CHECK(it.flags & (kHasRows | kHasMask));
        CHECK(it.row_bias == 0 && it.mask_bias == 0);  // a round's only bias is the sign count
        if (it.flags & kHasRows) {
            CHECK(it.nrows > 0 && it.row_valid > 0 && it.row_valid <= (uint32_t)kWaveSlots * shape.subtiles);
            CHECK(it.row_out + it.row_valid <= r.L);                                                // inside out
            CHECK(it.row_in + (uint64_t)(it.nrows - 1) * pitch + it.row_valid <= r.N * pitch);      // inside rows
            if (it.row_out + it.row_valid > r.L) continue;
            CHECK(it.row_in >= it.row_out && (it.row_in - it.row_out) % pitch == 0);
            const uint32_t a = (uint32_t)((it.row_in - it.row_out) / pitch);
            TileParts &t = row_tiles[it.row_out];
            CHECK(t.parts.empty() || t.valid == it.row_valid);
            t.valid = it.row_valid;
            t.parts.push_back({a, a + it.nrows});
            for (uint32_t l = 0; l < it.row_valid; ++l) {
                rows[it.row_out + l] += it.nrows;
                if (!(it.flags & kSameTile)) ++writers[it.row_out + l];
            }
        }
        if (it.flags & kHasMask) {
            CHECK(it.nseeds > 0 && it.mask_valid > 0 && it.mask_valid <= (uint32_t)kWaveSlots * shape.subtiles);
            CHECK(it.mask_out + it.mask_valid <= r.L);
            CHECK(it.k0 + it.nseeds <= (uint32_t)r.K);
            CHECK(it.mask_out % 16 == 0 && it.mask_ctr == (slot0 + it.mask_out) / 16);
            if (it.flags & kSameTile)
                CHECK((it.flags & kHasRows) && it.row_out == it.mask_out && it.row_valid == it.mask_valid);
            if (it.mask_out + it.mask_valid > r.L) continue;
            TileParts &t = mask_tiles[it.mask_out];
            CHECK(t.parts.empty() || t.valid == it.mask_valid);
            t.valid = it.mask_valid;
            t.parts.push_back({it.k0, it.k0 + it.nseeds});
            for (uint32_t l = 0; l < it.mask_valid; ++l) {
                seeds[it.mask_out + l] += it.nseeds;
                ++writers[it.mask_out + l];
                if (it.flags & kMaskBiasNneg) ++bias[it.mask_out + l];
            }
        } else {
            CHECK(!(it.flags & (kSameTile | kMaskBiasNneg | kMaskAtomic)));
        }
    }
    // every row reaches every slot once: per tile the row parts partition [0, N), and the tiles
    // cover every slot with N rows in all, so no slot lies in two tiles or in none
    check_partition(row_tiles, (uint32_t)r.N);
    check_partition(mask_tiles, (uint32_t)r.K);
    bool many = false;
    for (uint64_t l = 0; l < r.L; ++l) {
        const bool masked = r.K > 0 && l >= r.lo && l < r.hi;
        CHECK(rows[l] == (uint32_t)r.N);
        CHECK(seeds[l] == (masked ? (uint32_t)r.K : 0u));
        CHECK(bias[l] == (masked ? 1u : 0u));
        many |= writers[l] > 1;
        if (failures) return;  // one slot's report is enough
    }
    // a slot with more than one writer: every one of them adds atomically, into a zeroed output
    if (many) CHECK(shape.needs_zero && shape.atomics);
    bool two_tiles = false;
    for (const Item &it : items) {
        uint32_t rw = 0, mw = 0;
        if (it.flags & kHasRows)
            for (uint32_t l = 0; l < it.row_valid; ++l) rw = std::max(rw, writers[it.row_out + l]);
        if (it.flags & kHasMask)
            for (uint32_t l = 0; l < it.mask_valid; ++l) mw = std::max(mw, writers[it.mask_out + l]);
        if (rw > 1) CHECK(it.flags & kRowAtomic);
        if (mw > 1) CHECK((it.flags & kMaskAtomic) && ((it.flags & kSameTile) ? (it.flags & kRowAtomic) : 1u));
        two_tiles |= (it.flags & kHasRows) && (it.flags & kHasMask) && !(it.flags & kSameTile);
    }
    if (two_tiles) CHECK(!shape.single_tile);
    for (uint64_t l = 0; l < r.L; ++l)
        if (writers[l] == 0) {  // nobody writes the slot: the zero-fill is its value
            CHECK(shape.needs_zero);
            break;
        }
}

static void check_aggregate_rounds() {
    const uint64_t M = 1u << 20;
    const Round cover[] = {  // tests/test_planner_cpu.py's shapes
        {1024, 1024, M, 0, M, 1, 0},           {1024, 1024, M / 4, 0, M / 4, 1, 0},     {1024, 1000, M / 4, 0, M / 4, 1, 0},
        {1024, 204, M, 0, M, 1, 0},            {1024, 8192, M, 3 << 17, 4 << 17, 1, 0}, {1024, 8192, M, 3 << 17, 4 << 17, 0, 0},
        {128, 128, 16384, 0, 16384, 1, 0},     {128, 156, 16000, 0, 16000, 1, 0},       {0, 7, 1000, 0, 1000, 1, 0},
        {5, 0, 1000, 0, 1000, 1, 0},           {33, 33, 4100, 1024, 3072, 1, 0},        {7, 3, 70000, 69984, 70000, 1, 0},
        {128, 1024, M, 7 << 17, 8 << 17, 2, 0}, {256, 1024, M, 1 << 18, 2 << 18, 2, 0},  {512, 1024, M, 0, 1 << 19, 2, 0},
        {1024, 8192, M, 3 << 17, 4 << 17, 2, 0}, {33, 40, 4100, 1024, 3072, 2, 0},       {7, 3, 70000, 69984, 70000, 2, 0},
        {5, 64, 70000, 4096, 69984, 2, 0},
    };
    for (const Round &r : cover) check_round(r);
    for (int subtiles : {1, 4, 16})
        for (int pairing : {0, 1, 2}) {
            check_round({33, 33, 4100, 1024, 3072, pairing, subtiles});
            check_round({7, 3, 70000, 69984, 70000, pairing, subtiles});
            // one row, one seed: nothing is cut into parts, so only the two items on the window's tile make it atomic
            check_round({1, 1, 2048, 1024, 2048, pairing, subtiles});
        }
}

// ------------------------------------------------------------------ client masks and expansion
// row i of N gets seeds [seg[i], seg[i+1]) (seg NULL: seed i) over all L slots, at PRG slot slot0
static void check_rows_jobs(bool have_x, int N, const int64_t *seg, const int8_t *signs, uint64_t L, uint64_t slot0) {
    const uint64_t pitch = (L + 63) / 64 * 64 + 64;  // rows further apart than they are long
    const uint32_t base = 7;
    const int K = seg ? (int)seg[N] : N;
    std::vector<Item> items;
    const PlanShape shape = plan_rows_jobs(have_x, pitch, N, seg, signs, K, base, L, slot0, items);
    CHECK(shape.subtiles == 16 && !shape.needs_zero && !shape.atomics && shape.single_tile && !shape.seed_light);
    std::vector<uint32_t> x(N * L, 0), masks(N * L, 0), bias(N * L, 0), writers(N * L, 0);
    for (const Item &it : items) {
        CHECK(!(it.flags & (kRowAtomic | kMaskAtomic | kMaskBiasNneg)));  // the bias is counted on the host
        const bool has_rows = it.flags & kHasRows, has_mask = it.flags & kHasMask;
        CHECK(has_rows || has_mask);
        const uint64_t out = has_mask ? it.mask_out : it.row_out;
        const uint32_t valid = has_mask ? it.mask_valid : it.row_valid;
        const uint64_t i = out / pitch, tile = out % pitch;
        CHECK(valid > 0 && valid <= 16u * kWaveSlots && tile % (16u * kWaveSlots) == 0);
        CHECK(i < (uint64_t)N && tile + valid <= L);  // no item crosses a row: it ends within row i's L slots
        if (i >= (uint64_t)N || tile + valid > L) continue;
        const uint32_t k0 = seg ? (uint32_t)seg[i] : (uint32_t)i, k1 = seg ? (uint32_t)seg[i + 1] : (uint32_t)i + 1;
        CHECK(has_mask == (k1 > k0));
        if (has_rows) {
            CHECK(it.row_out == out && it.row_valid == valid && it.row_in == it.row_out);  // x and out: one shape
            CHECK(it.nrows == (have_x ? 1u : 0u));
            CHECK(has_mask ? (it.flags & kSameTile) != 0 : true);
        }
        CHECK(has_rows == (have_x || !has_mask));
        if (has_mask) {
            CHECK(it.k0 == k0 && it.nseeds == k1 - k0);
            CHECK(it.mask_ctr == (slot0 + tile) / 16);
        }
        for (uint32_t l = 0; l < valid; ++l) {
            const size_t at = i * L + tile + l;
            ++writers[at];
            x[at] += has_rows ? it.nrows : 0;
            masks[at] += has_mask ? it.nseeds : 0;
            bias[at] += (has_rows ? it.row_bias : 0) + (has_mask ? it.mask_bias : 0);
        }
    }
    for (int i = 0; i < N; ++i) {
        const uint32_t k0 = seg ? (uint32_t)seg[i] : (uint32_t)i, k1 = seg ? (uint32_t)seg[i + 1] : (uint32_t)i + 1;
        uint32_t nneg = 0;
        for (uint32_t k = k0; signs && k < k1; ++k) nneg += signs[k] < 0;
        for (uint64_t l = 0; l < L; ++l) {
            const size_t at = i * L + l;
            CHECK(writers[at] == 1 && x[at] == (have_x ? 1u : 0u) && masks[at] == k1 - k0);
            CHECK(bias[at] == (have_x ? 0u : base) + nneg);
            if (failures) return;
        }
    }
}

static void check_client_masks() {
    const int64_t seg[] = {0, 0, 3, 3, 4, 9};  // clients with no seeds, with one and with several
    const int8_t mixed[] = {1, -1, -1, 1, -1, 1, 1, -1, 1};
    const uint64_t L = 40000;  // one full 16,384-slot tile twice over and a ragged tail
    for (bool have_x : {false, true})
        for (const int8_t *signs : {(const int8_t *)nullptr, mixed})
            for (uint64_t slot0 : {uint64_t(0), ((uint64_t(1) << 36) - L) / 16 * 16}) {
                check_rows_jobs(have_x, 5, seg, signs, L, slot0);
                check_rows_jobs(have_x, 3, nullptr, signs, 1000, slot0);  // seg NULL: one seed per row
            }
}

// ------------------------------------------------------------------ pure rules
static void check_rules() {
    const uint64_t top = 1ull << 36;
    // tests/test_planner_cpu.py test_plan_range_rule's values
    CHECK(!slot_range_ok(0ull - 16, 32) && !slot_range_ok(0ull - 2064, 2064) && !slot_range_ok(0ull - 16, 16));
    CHECK(slot_range_ok(top - 2064, 2064) && slot_range_ok(top - 16, 16) && slot_range_ok(top, 0));
    CHECK(!slot_range_ok(top - 2048, 2064) && !slot_range_ok(top + 16, 0) && !slot_range_ok(top, 16));
    CHECK(slot_range_ok(0, top) && !slot_range_ok(0, top + 1) && slot_range_ok(0, 0));

    // tune_variant -1 .. 8 by {single tile, single tile seed-light, dual tile, dual tile seed-light}
    static const int want[10][4] = {
        {kVarMerged, kVarMergedSpread, kVarBlock, kVarBlockSpread},  // auto
        {0, 0, 0, 0}, {1, 1, 1, 1}, {2, 2, 1, 1}, {3, 3, 1, 1}, {4, 4, 1, 1}, {5, 5, 1, 1}, {6, 6, 1, 1},
        {7, 7, 8, 8}, {8, 8, 8, 8},
    };
    for (int v = -1; v < kVarCount; ++v)
        for (int c = 0; c < 4; ++c) {
            PlanShape s;
            s.single_tile = c < 2;
            s.seed_light = c & 1;
            CHECK(pick_variant(v, s) == want[v + 1][c]);
        }

    const uint64_t q = 1ull << 22;
    CHECK(small_round_width(0, 1, 1, 64, 0, 64) == 0);                          // never
    CHECK(small_round_width(1, 128, 128, 16384, 0, 16384) == 2);                // c2
    CHECK(small_round_width(1, 256, 256, 16384, 0, 16384) == 2);                // rows and mask words at 2^22
    CHECK(small_round_width(1, 257, 1, 16384, 0, 16384) == 0);                  // rows beyond
    CHECK(small_round_width(1, 1, 257, 16384, 0, 16384) == 0);                  // mask words beyond
    CHECK(small_round_width(1, 1, 512, 16384, 0, 8192) == 2);                   // the window counts, not L
    CHECK(small_round_width(1, 1, 1, q, 0, q) == 4 && small_round_width(1, 1, 1, q + 16, 0, q) == 0);
    CHECK(small_round_width(2, 1024, 1024, 1 << 20, 0, 1 << 20) == 4);          // whenever legal
    CHECK(small_round_width(1, 64, 1, 1 << 16, 0, 16) == 4 && small_round_width(1, 64, 1, (1 << 16) - 16, 0, 16) == 2);
    for (int tune : {1, 2}) {
        CHECK(small_round_width(tune, 3, 3, 1000, 8, 1000) == 0);   // mask_lo off a block
        CHECK(small_round_width(tune, 3, 3, 1000, 16, 100) == 0);   // mask_hi off a block and not L
        CHECK(small_round_width(tune, 3, 3, 1000, 16, 1000) == 2);  // mask_hi == L may be ragged
        CHECK(small_round_width(tune, 3, 3, 1000, 16, 992) == 2);
    }
}

// ------------------------------------------------------------------ staging pieces
static void check_pieces() {
    const size_t S = kStageBytes;
    const size_t shapes[][2] = {{S - 1, 1}, {S - 1, 3}, {S, 1}, {S, 3}, {S + 1, 1},     {S + 1, 3}, {2 * S + 5, 3},
                                {3 * S, 1}, {1, 1},     {1, 2 * S + 7}, {S / 2 + 1, 3}, {S / 3, 7}, {4096, 1}};
    for (const auto &sh : shapes) {
        const size_t width = sh[0], rows = sh[1];
        size_t end = 0;  // the pieces in order are consecutive byte ranges of the packed rows x width rectangle
        for (const flm::rt::Piece &p : flm::rt::pieces(width, rows)) {
            CHECK(p.w > 0 && p.nr > 0 && p.w * p.nr <= S);
            CHECK(p.r + p.nr <= rows && p.c + p.w <= width);
            CHECK(p.nr == 1 || (p.c == 0 && p.w == width));  // several rows: whole ones
            CHECK(p.r * width + p.c == end);
            end += p.w * p.nr;
        }
        CHECK(end == width * rows);
    }
}

// ------------------------------------------------------------------ CopyPool
static void copy_once(CopyPool &pool, size_t width, size_t rows, size_t dpitch, size_t spitch) {
    std::vector<uint8_t> src(rows * spitch), dst(rows * dpitch, 0xEE);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(i * 131 + (i >> 8) + 1);
    pool.copy2d(dst.data(), dpitch, src.data(), spitch, width, rows);
    size_t bad = 0;
    for (size_t r = 0; r < rows; ++r) {
        bad += std::memcmp(dst.data() + r * dpitch, src.data() + r * spitch, width) != 0;
        for (size_t c = width; c < dpitch; ++c) bad += dst[r * dpitch + c] != 0xEE;  // padding untouched
    }
    CHECK(bad == 0);
}

static void check_copy_pool() {
    const size_t split = CopyPool::kMinSplit;
    { CopyPool untouched; }
    {
        CopyPool small;  // below kMinSplit the calling thread copies alone: destroyed with no worker started
        copy_once(small, 1000, 262, 1032, 1024);  // 262,000 bytes, just below
        copy_once(small, split - 1, 1, split + 7, split - 1);
        copy_once(small, 1, 1, 1, 1);
    }
    {
        CopyPool pool;
        copy_once(pool, 1000, 263, 1032, 1024);           // 263,000 bytes, just above: the workers start
        copy_once(pool, 1000, 4099, 1008, 1064);          // the second copy reuses them; slices end inside rows
        copy_once(pool, split, 1, split, split);          // exactly kMinSplit, one row
        copy_once(pool, split + 123, 1, split + 123, split + 200);  // one row, no multiple of 4096
        copy_once(pool, 4096, 64, 4096, 4096);            // packed both sides, slices on 4 KiB bounds
        copy_once(pool, 3 * split + 4097, 3, 3 * split + 4100, 3 * split + 4097);
        copy_once(pool, 10, 3, 16, 12);                   // a small copy between large ones
        copy_once(pool, 777, 1000, 800, 777);
    }
}

int main(int argc, char **argv) {
    const bool copies_only = argc > 1 && !std::strcmp(argv[1], "copies");
    if (!copies_only) {
        check_aggregate_rounds();
        check_client_masks();
        check_rules();
        check_pieces();
    }
    check_copy_pool();
    std::printf(failures ? "%d checks failed\n" : "planner_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
