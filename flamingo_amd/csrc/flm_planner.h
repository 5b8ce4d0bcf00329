// flm_planner.h -- the launch planner of the host runtime (flm_runtime.hip): it turns a round's shape
// into Items (flm_items.h) so that every workgroup carries an equal share of row streaming and mask
// generation, and holds the pure rules beside it (kernel variant, small-round width, the 2^36 slot range).
// Plain C++, no HIP and no device state: checked on the CPU (tools/planner_check.cpp, tests/test_planner_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "flm_items.h"

namespace flm {
namespace plan __attribute__((visibility("hidden"))) {  // the library exports nothing of this header

constexpr int kDefaultMinItems = 1024;   // flm_set_tuning("min_items") default
constexpr uint64_t kUnsplitTiles = 1024;  // 4 tiles per MI355X CU: from this many a whole-vector round is not split
constexpr uint64_t kSplitItems = 2048;    // item target of a split whole-vector round (8 per CU)
constexpr int kWindowItems = 512;         // item target of a windowed (slot-sharded) round: 2 per CU

// What a launch needs to know of a list of items (the runtime's Plan adds the device copy and its events).
struct PlanShape {
    int subtiles = 1;
    bool needs_zero = false;
    int atomics = 0;
    bool single_tile = true;  // every item writes one tile (merged accumulator legal)
    bool seed_light = false;  // mask work small next to row streaming
};

// One contiguous job of the planner: out[out_base + l] for l in [0, L) gets the
// sum of `nrows` rows (rows_base + r*pitch + l) and, for l in [mask_lo, mask_hi),
// seeds [k0, k0+nseeds) at PRG slot prg_slot0 + l, plus mask_bias.
struct Job {
    uint64_t out_base = 0, rows_base = 0;
    uint32_t nrows = 0;
    uint64_t L = 0;
    uint32_t k0 = 0, nseeds = 0;
    uint64_t mask_lo = 0, mask_hi = 0, prg_slot0 = 0;
    uint32_t mask_bias = 0;
    bool bias_nneg = false;
};

// plan_job splits a job into row units (tiles x row parts) and mask units (tiles x seed
// parts) of equal weight, then pairs unit i of each list into one Item, so one
// workgroup streams rows (HBM) while it generates masks (VALU).
struct Unit {
    uint64_t tile;  // out slot of the tile start (relative to job)
    uint32_t a, n;  // row or seed sub-range
    uint32_t valid;
    uint32_t part;
};

// The row unit u of job j as the row half of an item (`extra`: its atomic flag, if any).
inline void fill_rows(Item &it, const Job &j, uint64_t pitch, const Unit &u, uint32_t extra) {
    it.flags |= kHasRows | extra;
    it.row_in = j.rows_base + (uint64_t)u.a * pitch + u.tile;
    it.nrows = u.n;
    it.row_out = j.out_base + u.tile;
    it.row_valid = u.valid;
}

// The mask unit u of job j as the mask half of an item (`extra`: atomic and same-tile flags).
inline void fill_mask(Item &it, const Job &j, const Unit &u, uint32_t extra) {
    it.flags |= kHasMask | extra;
    it.k0 = j.k0 + u.a;
    it.nseeds = u.n;
    it.mask_out = j.out_base + u.tile;
    it.mask_ctr = (j.prg_slot0 + u.tile) / 16;
    it.mask_valid = u.valid;
    if (u.part == 0) {  // per-slot constants are added exactly once
        it.mask_bias = j.mask_bias;
        if (j.bias_nneg) it.flags |= kMaskBiasNneg;
    }
}

// Appends the job's items and folds what they need into `shape` (whose subtiles set the tile).
inline void plan_job(const Job &j, uint64_t pitch, int parts_r, int parts_m, bool dual_tile, std::vector<Item> &items,
                     PlanShape &shape) {
    const uint64_t W = (uint64_t)kWaveSlots * shape.subtiles;
    // the tiles of slots [lo, hi), each with the n rows or seeds cut into `parts` sub-ranges
    auto units = [W](uint64_t lo, uint64_t hi, uint32_t n, int parts) {
        std::vector<Unit> v;
        for (uint64_t t = lo; n > 0 && t < hi; t += W)
            for (int p = 0; p < parts; ++p) {
                const uint32_t a = (uint32_t)((uint64_t)n * p / parts), b = (uint32_t)((uint64_t)n * (p + 1) / parts);
                if (b > a) v.push_back({t, a, b - a, (uint32_t)std::min<uint64_t>(W, hi - t), (uint32_t)p});
            }
        return v;
    };
    const std::vector<Unit> R = units(0, j.L, j.nrows, parts_r), M = units(j.mask_lo, j.mask_hi, j.nseeds, parts_m);
    // A tile written by exactly one Item is stored; otherwise every contributor
    // adds atomically into a zeroed output.  Rows and masks share one Item per
    // tile ("same tile") in whole-vector rounds whose rows and seeds are cut into
    // the same number of parts: unit i of each list then covers the same tile, and
    // the item keeps the merged single-accumulator kernel (atomic when parts > 1).
    const bool both = !R.empty() && !M.empty();
    bool paired_same = both && parts_r == parts_m && j.mask_lo == 0 && j.mask_hi == j.L && R.size() == M.size();
    for (size_t i = 0; paired_same && i < R.size(); ++i) paired_same = R[i].tile == M[i].tile;
    const bool atomic = parts_r > 1 || parts_m > 1 || (both && !paired_same);
    if (atomic) shape.needs_zero = true;
    if (R.empty() && (j.mask_lo > 0 || j.mask_hi < j.L || M.empty())) shape.needs_zero = true;
    shape.atomics |= atomic ? 1 : 0;

    // Rows and masks on different tiles: either pair them into dual-tile items
    // (one workgroup streams rows of tile A while generating masks of tile B), or
    // emit single-kind items interleaved R0 M0 R1 M1 ... so row and mask
    // workgroups share CUs and each can use the merged-accumulator kernel.
    const bool interleave = both && !paired_same && !dual_tile;
    if (both && !paired_same && dual_tile) shape.single_tile = false;
    const uint32_t row_at = atomic ? kRowAtomic : 0u, mask_at = atomic ? kMaskAtomic : 0u;
    const size_t n = std::max(R.size(), M.size());
    for (size_t i = 0; i < n; ++i) {
        Item it{};
        if (i < R.size()) fill_rows(it, j, pitch, R[i], row_at);
        if (interleave && i < R.size() && i < M.size()) {  // the row unit is an item of its own
            items.push_back(it);
            it = Item{};
        }
        if (i < M.size())
            fill_mask(it, j, M[i], mask_at | (paired_same && i < R.size() && R[i].tile == M[i].tile ? kSameTile : 0u));
        items.push_back(it);
    }
}

inline void choose_parts(uint64_t tiles_r, uint64_t tiles_m, uint32_t nrows, uint32_t nseeds, int &pr, int &pm,
                         uint64_t kTarget = kDefaultMinItems) {
    // Balance mask units against row units, then split both until the grid
    // has a few workgroups per CU (16 waves each), keeping >= 16 rows/seeds
    // per item so every wave of a workgroup has work.
    pr = 1;
    pm = 1;
    if (tiles_r && tiles_m && tiles_r > tiles_m) pm = (int)std::min<uint64_t>(nseeds, (tiles_r + tiles_m - 1) / tiles_m);
    if (tiles_r && tiles_m && tiles_m > tiles_r) pr = (int)std::min<uint64_t>(nrows, (tiles_m + tiles_r - 1) / tiles_r);
    auto units = [&] { return std::max(tiles_r * pr, tiles_m * pm); };
    while (units() < kTarget) {
        bool grew = false;
        if (tiles_r && (uint64_t)pr * 2 * 16 <= nrows) { pr *= 2; grew = true; }
        if (tiles_m && (uint64_t)pm * 2 * 16 <= nseeds) { pm *= 2; grew = true; }
        if (!grew) break;
    }
}

// A rank of the slot-sharded round as same-tile items (pairing 2).  The shard's 1024-slot tiles
// carry rows AND seeds, cut into P matching parts (part p of a tile: rows [N p/P, N (p+1)/P) and
// seeds [K p/P, K (p+1)/P), atomics when P > 1); every other tile is one rows-only item, spread
// evenly between the heavy items so that row streaming runs beside the ChaCha work from the
// start.  Every item writes one tile, so the merged single-accumulator kernel runs (63 VGPRs,
// 8 waves/SIMD) instead of the dual-tile kernel (104 VGPRs, 4 waves/SIMD).  Measured slower than
// the dual-tile items at G = 2 / 4 / 8 (0.78 / 0.42 / 0.228 ms against 0.69 / 0.36 / 0.188 ms,
// profiles/r02_ab_window_same.log): a tuning option (flm_set_tuning "pairing" 2), not the default.
inline PlanShape plan_window_same(uint64_t pitch, int N, int K, uint64_t L, uint64_t mask_lo, uint64_t mask_hi,
                                  uint64_t prg_slot0, uint64_t heavy_target, std::vector<Item> &items) {
    const uint64_t W = kWaveSlots;
    const uint64_t tm = (mask_hi - mask_lo + W - 1) / W;
    uint64_t P = tm ? (heavy_target + tm - 1) / tm : 1;
    while (P > 1 && (uint64_t)K < 16 * P) P /= 2;  // >= 16 seeds per part: every wave has work
    if (P < 1) P = 1;
    Job j;
    j.prg_slot0 = prg_slot0;
    j.bias_nneg = true;
    std::vector<Item> heavy, light;
    for (uint64_t t = mask_lo; t < mask_hi; t += W) {
        const uint32_t valid = (uint32_t)std::min<uint64_t>(W, mask_hi - t);
        for (uint64_t p = 0; p < P; ++p) {
            Item it{};
            const uint32_t ra = (uint32_t)((uint64_t)N * p / P), rb = (uint32_t)((uint64_t)N * (p + 1) / P);
            const uint32_t sa = (uint32_t)((uint64_t)K * p / P), sb = (uint32_t)((uint64_t)K * (p + 1) / P);
            const uint32_t at = P > 1 ? (kRowAtomic | kMaskAtomic) : 0u;
            if (rb > ra) fill_rows(it, j, pitch, {t, ra, rb - ra, valid, (uint32_t)p}, at);
            if (sb > sa) fill_mask(it, j, {t, sa, sb - sa, valid, (uint32_t)p}, at | (rb > ra ? kSameTile : 0u));
            if (it.flags) heavy.push_back(it);
        }
    }
    auto rows_only = [&](uint64_t a, uint64_t b) {
        for (uint64_t t = a; t < b; t += W) {
            Item it{};
            fill_rows(it, j, pitch, {t, 0, (uint32_t)N, (uint32_t)std::min<uint64_t>(W, b - t), 0}, 0u);
            light.push_back(it);
        }
    };
    rows_only(0, mask_lo);
    rows_only(mask_hi, L);
    // interleave: light item j goes after heavy item floor((j + 1) * H / (Lt + 1))
    const size_t H = heavy.size(), Lt = light.size();
    items.reserve(H + Lt);
    size_t l = 0;
    for (size_t h = 0; h < H; ++h) {
        items.push_back(heavy[h]);
        while (l < Lt && (l + 1) * H <= (h + 1) * (Lt + 1)) items.push_back(light[l++]);
    }
    while (l < Lt) items.push_back(light[l++]);
    PlanShape shape;
    shape.needs_zero = P > 1;
    shape.atomics = P > 1 ? 1 : 0;
    return shape;
}

// Host-only planning of one aggregate round (no device state): fills `items`
// and returns the plan's flags.  Shared by the runtime's aggregate_plan and the
// flm_plan_aggregate diagnostic entry point.
inline PlanShape build_aggregate_items(int tune_subtiles, int pairing, uint64_t pitch, int N, int K, uint64_t L,
                                       uint64_t mask_lo, uint64_t mask_hi, uint64_t prg_slot0, std::vector<Item> &items,
                                       int min_items = kDefaultMinItems) {
    // ChaCha-heavy rounds keep 1024-slot tiles (16 waves split one tile's seeds);
    // row-streaming-heavy rounds (few seeds per slot) prefer 4 sub-tiles per
    // workgroup: 4096-slot tiles, fewer LDS combines (measured 5.77 vs 5.26 TB/s).
    const bool seed_light = (uint64_t)K * (mask_hi - mask_lo) * 2 < (uint64_t)N * L;
    // A rank of the slot-sharded round (rows over all of L, masks over a window): 4096-slot
    // tiles and kWindowItems items, one generation of workgroups on the chip.  One rank of the
    // strong-scaled c4 round, G = 8: 0.179 -> 0.169 ms; G = 4: 0.364 -> 0.350-0.360 ms; G = 2 the
    // same (profiles/r02_ab_strong_plan.log).
    const bool windowed = N > 0 && K > 0 && (mask_lo > 0 || mask_hi < L);
    if (pairing == 2 && windowed && !seed_light && tune_subtiles <= 0)
        return plan_window_same(pitch, N, K, L, mask_lo, mask_hi, prg_slot0, (uint64_t)min_items, items);
    PlanShape shape;
    shape.subtiles = tune_subtiles > 0 ? tune_subtiles : ((seed_light || windowed) ? 4 : 1);
    shape.seed_light = seed_light;
    const uint64_t W = (uint64_t)kWaveSlots * shape.subtiles;
    Job j;
    j.nrows = (uint32_t)N;
    j.L = L;
    j.nseeds = (uint32_t)K;
    j.mask_lo = mask_lo;
    j.mask_hi = mask_hi;
    j.prg_slot0 = prg_slot0;
    j.bias_nneg = true;
    const uint64_t tr = N > 0 ? (L + W - 1) / W : 0;
    const uint64_t tm = (K > 0 && mask_hi > mask_lo) ? (mask_hi - mask_lo + W - 1) / W : 0;
    int pr, pm;
    if (!seed_light && min_items == kDefaultMinItems && mask_lo == 0 && mask_hi == L && tr == tm && tm > 0) {
        // A whole-vector ChaCha-heavy round: rows and seeds are cut into the same number of parts P,
        // so part p of both lands in one item and the merged single-accumulator kernel runs
        // (plan_job).  From kUnsplitTiles tiles (4 per CU: c4 / c5, 1024 tiles) one item per tile --
        // no atomics, no zero-fill; 2048 items measured no faster there.  Fewer tiles (c3, N=1024,
        // L=2^18: 256 tiles) are split until kSplitItems items: 0.389 ms at P=8 against 0.414 ms
        // unsplit (one 4-wave/SIMD generation) and 0.410 at P=2 (profiles/r02_ab_split.log).
        pr = pm = 1;
        while (tm < kUnsplitTiles && tm * (uint64_t)pr < kSplitItems && (uint64_t)pr * 2 * 16 <= (uint64_t)N &&
               (uint64_t)pr * 2 * 16 <= (uint64_t)K)
            pr = pm = pr * 2;
    } else {
        const int target = (windowed && !seed_light && tune_subtiles <= 0 && min_items == kDefaultMinItems)
                               ? kWindowItems : min_items;
        choose_parts(tr, tm, (uint32_t)N, (uint32_t)K, pr, pm, (uint64_t)target);
    }
    plan_job(j, pitch, pr, pm, pairing != 0, items, shape);
    return shape;
}

// Client masking / expansion plan: one job per output row, 16 sub-tiles per
// workgroup (each wave its own 1024 slots, all of the row's seeds).
// out[i] = (x[i] or base_bias) + sum of row i's seeds (+1 per negative seed).
// seg NULL: row i has seed i alone.  signs: K host signs, or NULL for all +1 (expansion).
inline PlanShape plan_rows_jobs(bool have_x, uint64_t pitch, int N, const int64_t *seg, const int8_t *signs, int /*K*/,
                                uint32_t base_bias, uint64_t L, uint64_t slot0, std::vector<Item> &items) {
    PlanShape shape;
    shape.subtiles = 16;
    const uint64_t W = (uint64_t)kWaveSlots * shape.subtiles;
    for (int i = 0; i < N; ++i) {
        Job j;
        j.out_base = j.rows_base = (uint64_t)i * pitch;  // x and out have one shape
        j.nrows = have_x ? 1 : 0;
        j.L = L;
        const uint32_t k0 = seg ? (uint32_t)seg[i] : (uint32_t)i;
        const uint32_t k1 = seg ? (uint32_t)seg[i + 1] : (uint32_t)i + 1;
        uint32_t nneg = 0;
        if (signs)
            for (uint32_t k = k0; k < k1; ++k) nneg += signs[k] < 0;
        const uint32_t bias = (have_x ? 0u : base_bias) + nneg;
        if (k1 == k0) {
            // no seeds: out = x (copy) or the constant bias, as a rows-only item
            for (uint64_t t = 0; t < L; t += W) {
                Item it{};
                fill_rows(it, j, pitch, {t, 0, j.nrows, (uint32_t)std::min<uint64_t>(W, L - t), 0}, 0u);
                it.row_bias = bias;
                items.push_back(it);
            }
            continue;
        }
        j.k0 = k0;
        j.nseeds = k1 - k0;
        j.mask_hi = L;
        j.prg_slot0 = slot0;
        j.mask_bias = bias;
        plan_job(j, pitch, 1, 1, false, items, shape);
    }
    return shape;
}

// The items_kernel variant for a plan: the tuned one (-1 = auto), made legal for the plan.
inline int pick_variant(int tune_variant, const PlanShape &shape) {
    int v = tune_variant;
    // measured (tools/ab/ab_items.py, profiles/r01_ab_items*.log): merged accumulator
    // fastest where legal (seeds spread over the rows when seed-light), block next
    if (v < 0)
        v = shape.single_tile ? (shape.seed_light ? kVarMergedSpread : kVarMerged)
                              : (shape.seed_light ? kVarBlockSpread : kVarBlock);
    if (!shape.single_tile && v >= kVarMerged) v = (v == kVarMergedSpread || v == kVarBlockSpread)
                                                       ? kVarBlockSpread : kVarBlock;
    return v;
}

// Workgroup width B (16*B slots) of the one-launch small-round kernel for this round, or 0 to
// take the seed-schedule + items_kernel path.  Auto (tune_small 1): rounds whose rows and mask
// words are both <= 2^22 (c2: 2^21 each), where items_kernel's fixed ~10 us dominates.
inline int small_round_width(int tune_small, int N, int K, uint64_t L, uint64_t mask_lo, uint64_t mask_hi) {
    if (tune_small == 0) return 0;
    if (mask_lo % 16 || (mask_hi % 16 && mask_hi != L)) return 0;
    if (tune_small == 1 && ((uint64_t)N * L > (1ull << 22) || (uint64_t)K * (mask_hi - mask_lo) > (1ull << 22)))
        return 0;
    // 2 blocks per 256-thread workgroup keeps 128 seeds per pass (c2: one pass, every lane busy);
    // longer vectors take 4 (64 slots) so the grid stays near 1024 workgroups
    return L >= (1ull << 16) ? 4 : 2;
}

// The one rule for a PRG window of n slots from slot0: it must end at or below 2^36 (slot / 16 is the
// 32-bit block counter).  Compared without forming slot0 + n, which wraps for a slot0 near 2^64.
inline bool slot_range_ok(uint64_t slot0, uint64_t n) {
    constexpr uint64_t kSlotLimit = 1ull << 36;
    return slot0 <= kSlotLimit && n <= kSlotLimit - slot0;
}

}  // namespace plan
}  // namespace flm
