// flm_items.h -- the work-item and seed-schedule records the host planner (flm_planner.h) writes and the gfx950
// kernels (flm_kernels.hip) read.  Plain C++, no HIP, so the planner is checked on the CPU (tools/planner_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace flm {

// One wave owns a 1024-slot sub-tile: 64 lanes x one 16-word ChaCha block.
constexpr int kWaveSlots = 1024;
constexpr int kWavesPerGroup = 16;          // 1024-thread workgroups
constexpr int kThreads = 64 * kWavesPerGroup;

// The float front end (rotate_kernel, the L2 clip's kernels): one workgroup per 4096-parameter tile of a row.
constexpr uint64_t kFloatTile = 4096;
constexpr uint64_t float_tiles(uint64_t L) { return L / kFloatTile + (L % kFloatTile ? 1 : 0); }

// Per-seed schedule, built on the device by seed_schedule_kernel: the key, the
// sign folded into an XOR constant, and everything of ChaCha's first double
// round that does not depend on the block counter (block counter high word is
// 0 for every slot < 2^36, nonce is zero).  128 bytes, read with scalar loads.
struct SeedRec {
    uint32_t k[8];     // key words (LE32 of the 32 seed bytes)
    uint32_t xorc;     // 0x64636261 for sign +1, ~0x64636261 for sign -1
    uint32_t a0;       // sigma0 + k0 (first add of column 0)
    uint32_t col1[4];  // x1, x5, x9, x13 after round-1 column QR(1,5,9,13)
    uint32_t col2[4];  // x2, x6, x10, x14 after QR(2,6,10,14)
    uint32_t col3[4];  // x3, x7, x11, x15 after QR(3,7,11,15)
    uint32_t pad[10];
};
static_assert(sizeof(SeedRec) == 128, "SeedRec must be 128 bytes");

enum ItemFlags : uint32_t {
    kHasRows = 1u,
    kHasMask = 2u,
    kSameTile = 4u,       // row tile == mask tile: combine before writing
    kRowAtomic = 8u,      // row (or combined) tile written with u32 atomic adds
    kMaskAtomic = 16u,
    kMaskBiasNneg = 32u,  // add the device-side count of negative signs to the mask tile
};

// One workgroup's work: a row unit (sum of `nrows` rows over one tile) and/or a
// mask unit (sum of seeds [k0, k0+nseeds) over one tile).  64 bytes.
struct Item {
    uint64_t row_in;     // element offset into rows: first row of the unit, tile start slot
    uint64_t row_out;    // element offset into out of the row tile
    uint64_t mask_out;   // element offset into out of the mask tile
    uint64_t mask_ctr;   // ChaCha block counter at the mask tile start (PRG slot / 16)
    uint32_t nrows;
    uint32_t k0;
    uint32_t nseeds;
    uint32_t row_valid;  // valid slots in the row tile (tail)
    uint32_t mask_valid;
    uint32_t flags;
    uint32_t row_bias;   // added once per slot of the row tile
    uint32_t mask_bias;  // added once per slot of the mask tile
};
static_assert(sizeof(Item) == 64, "Item must be 64 bytes");

// items_kernel variants (see flm_kernels.hip): row load layout / accumulator form.
enum ItemsVariant : int {
    kVarCoalesced = 0,  // coalesced rows, separate row/mask accumulators (any plan)
    kVarBlock = 1,      // block-layout rows, separate accumulators (any plan)
    kVarMerged = 2,     // block-layout rows added into the mask accumulator (single-tile plans)
    kVarMergedW8 = 3,   // kVarMerged at >= 8 waves/SIMD register budget
    kVarMergedRU4 = 4,  // kVarMerged, 4 rows in flight in the rows-only loop
    kVarMergedNT = 5,   // kVarMerged, non-temporal row loads
    kVarMergedRU4NT = 6,
    kVarMergedSpread = 7,  // kVarMerged, seeds spread evenly over the row stream
    kVarBlockSpread = 8,   // kVarBlock (dual-tile plans), seeds spread over the row stream
    kVarCount = 9,
};

}  // namespace flm
