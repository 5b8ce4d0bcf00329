// flm_runtime.hip -- host runtime and C ABI of libflamingo_hip.so (include/flamingo_hip.h).
//
// Owns one GPU per context: its stream, grow-on-demand device buffers, the
// per-shape launch plans (work-item tables), their stream-ordering bookkeeping
// (StreamMarks) and the error string.  What needs no device is in HIP-free headers:
// the launch planner (flm_planner.h: a round's shape into Items), the CPU side of
// the host copies (flm_copy_pool.h) and their layout (flm_host_layout.h).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/flamingo_hip.h"
#include "flm_call_args.h"
#include "flm_copy_pool.h"
#include "flm_internal.h"
#include "flm_planner.h"

using flm::Item;
using flm::SeedRec;
using flm::plan::PlanShape;
using flm::rt::CopyPool;

namespace {

thread_local std::string g_last_error;
constexpr int kCopyStreams = 4;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = flm::rt::grow_bytes(std::max<size_t>(bytes, 256));
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {  // no room for the slack: exactly what was asked
            (void)hipGetLastError();
            want = std::max<size_t>(bytes, 256);
            e = hipMalloc(&p, want);
        }
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};

// True when the event has completed (or was never recorded); false while it is pending.  The one
// place that queries an event.  After a not-ready query it clears the thread's last error, the
// caller's sticky one included (fixable here, for every user at once).
bool event_done(hipEvent_t e) {
    if (!e) return true;
    const hipError_t q = hipEventQuery(e);
    if (q == hipSuccess) return true;
    (void)hipGetLastError();  // hipErrorNotReady (an error status would surface at the next launch)
    return false;
}

// The last use of one thing (a plan's items, a seed table) on every stream that used it: one
// event per stream, recorded after each use there and reused.  Adds no dependency between the
// streams by itself; the owner asks, waits or synchronises when it wants to rewrite the thing.
class StreamMarks {
  public:
    StreamMarks() = default;
    StreamMarks(const StreamMarks &) = delete;
    StreamMarks &operator=(const StreamMarks &) = delete;
    ~StreamMarks() { for (auto &m : marks_) (void)hipEventDestroy(m.second); }
    // The work enqueued on s so far is the thing's last use on s.  Many streams over time: from
    // kPrune entries a new stream first drops the entries already completed.
    hipError_t record(hipStream_t s) {
        hipEvent_t ev = event_of(s);
        if (!ev) {
            if (marks_.size() >= kPrune) {
                size_t kept = 0;
                for (const Mark &m : marks_) {
                    if (event_done(m.second)) (void)hipEventDestroy(m.second);
                    else marks_[kept++] = m;
                }
                marks_.erase(marks_.begin() + kept, marks_.end());
            }
            const hipError_t c = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (c != hipSuccess) return c;
            marks_.emplace_back(s, ev);
        }
        return hipEventRecord(ev, s);
    }
    // the event of the last use on s, or NULL
    hipEvent_t event_of(hipStream_t s) const {
        for (const auto &m : marks_)
            if (m.first == s) return m.second;
        return nullptr;
    }
    // a use on a stream other than s has not completed yet
    bool pending_elsewhere(hipStream_t s) const {
        for (const auto &m : marks_)
            if (m.first != s && !event_done(m.second)) return true;
        return false;
    }
    // s waits, on the device, for the uses on every other stream
    hipError_t wait_elsewhere(hipStream_t s) const {
        hipError_t e = hipSuccess;
        for (const auto &m : marks_)
            if (e == hipSuccess && m.first != s) e = hipStreamWaitEvent(s, m.second, 0);
        return e;
    }
    // the host waits for every use (up to the first error: the device has failed then)
    hipError_t sync_all() const {
        hipError_t e = hipSuccess;
        for (const auto &m : marks_)
            if (e == hipSuccess) e = hipEventSynchronize(m.second);
        return e;
    }
    void swap(StreamMarks &o) { marks_.swap(o.marks_); }

  private:
    using Mark = std::pair<hipStream_t, hipEvent_t>;
    static constexpr size_t kPrune = 8;
    std::vector<Mark> marks_;
};

struct Plan {
    DevBuf items;
    int n_items = 0;
    PlanShape shape;  // what the planner said of the items (flm_planner.h)
    // a cached plan's items are copied in on the stream of its first launch; a launch on
    // another stream waits for that copy (`ready`) until it is known to have completed
    hipEvent_t ready = nullptr;
    hipStream_t up_stream = nullptr;
    bool ready_known = true;
    // the plan's last launch on each stream it ran on (recorded by run_plan), and when it was last
    // used: the cache recycles its least recently used plan's buffers once those have completed
    StreamMarks done;
    uint64_t last_use = 0;
};

// Pinned host + device staging for the small per-call tables the *_dev entry points upload
// (packed seg + signs, signs, work items).  A slot goes back into use only once the launch that
// read its device copy has completed (its event), so a *_dev call never waits for earlier work:
// a busy pool grows (up to kStageSlots slots) instead of blocking the host.
constexpr size_t kStageSlots = 32;
struct StageSlot {
    void *host = nullptr;
    size_t cap = 0;
    DevBuf dev;
    hipEvent_t done = nullptr;
    bool busy = false;
    uint64_t last = 0;
};

using PlanKey = std::tuple<int, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t>;

// A device seed table: the per-seed schedule seed_schedule_kernel builds (SeedRec per seed) and
// its sign counts (meta), read by items_kernel / pair_units_kernel.  A context keeps a ring of
// them so that a call on one stream never rewrites a table that launches queued on other streams
// still read (the r05 cross-stream hazard): each table records its write
// stream (`w_stream`) and its last read on every stream (`readers`: one reused event per stream).
// A write followed at once by a read on the same stream (every fused call) is covered by that read's
// event; only a published table (flm_seed_table_dev: its reads may come on other streams) records
// `written` itself -- one event record per call on the hot path.  A table is rebuilt on stream s
// only once every read and write of it on other streams has completed; when all kSeedTables tables
// are still in use elsewhere, s waits on the device for the least recently used one's events
// (hipStreamWaitEvent, never a host wait).  Reads on the writing stream are in order by
// construction; a read on another stream waits for `written` first.
constexpr size_t kSeedTables = 8;
struct SeedTable {
    DevBuf recs, meta;
    hipEvent_t written = nullptr;
    bool written_valid = false;  // `written` was recorded after the last write (else a read on w_stream covers it)
    hipStream_t w_stream = nullptr;
    StreamMarks readers;
    uint64_t last_use = 0;
};

}  // namespace

// flm_last_plan's variant for a round run by small_round_kernel (items = its workgroups)
constexpr int kSmallRoundVariant = 100;
// flm_last_plan's variant after a PRG expansion by prg_expand_kernel (items = its workgroups)
constexpr int kExpandVariant = 101;

struct flm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    DevBuf rows, out, seeds, signs, bytes_in, bytes_out;
    std::vector<SeedTable *> tables;  // ring of device seed tables (SeedTable)
    SeedTable *cur_table = nullptr;   // the table the last seed-schedule / small-round launch wrote
    SeedTable *pub_table = nullptr;   // the table flm_seed_table_dev published for flm_aggregate_dev
    DevBuf rot_signs;                 // flm_rotate's sign words: PRG(key), in no call's array list (flm_call_args.h)
    DevBuf l2_work;                   // flm_l2_clip's and flm_rotate_clip's tile partials (and factors nobody asked for)
    DevBuf small_meta;                // sign counts of the one-launch small round (no seed table)
    bool last_small = false;          // the last sign counts came from a small round (flm_check_signs)
    uint64_t table_clock = 0;
    std::vector<StageSlot *> slots;  // staging pool of the *_dev uploads (StageSlot)
    uint64_t slot_clock = 0;
    DevBuf ec_in, ec_base, ec_scal, ec_jac, ec_out, ec_dig, ec_flags;  // P-256 batches
    // pinned staging ring for pageable host rows: two buffers, each reused once
    // the DMA that read it has completed (event per buffer)
    void *stage[2] = {nullptr, nullptr};
    size_t stage_cap = 0;
    hipEvent_t stage_done[2] = {nullptr, nullptr};
    // host->device streams for page-locked rows (several SDMA engines)
    hipStream_t copy[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t copy_done[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t copy_start = nullptr;
    std::map<PlanKey, Plan *> plans;
    uint64_t plan_clock = 0;
    int last_items = 0, last_tile = 0, last_atomics = 0, last_variant = 0;
    int table_k = -1;  // seeds in the published device seed table (pub_table), -1 = none
    int tune_variant = -1;   // items_kernel variant, -1 = auto
    int tune_subtiles = 0;   // aggregate sub-tiles per workgroup, 0 = auto
    int tune_min_items = flm::plan::kDefaultMinItems;  // planner target for work items per aggregate launch
    int tune_ec_threads = 64;   // ec_mul workgroup size (64/128/256; 64 measured best, 3.29 vs 3.43 ms)
    int tune_ec_waves = 1;      // ec_mul register budget as min waves/SIMD (1 = uncapped, 4, 8)
    int tune_ec_spread = 0;     // KiB of LDS reserved per 64-lane EC workgroup (0 = none): caps EC waves per CU
                                // so a CU-masked dispatch spreads them one per SIMD instead of packing two
    int tune_ec_terms = 1;      // combine terms per lane (1, 2, 4: Straus, shared doublings)
    int tune_ec_coop = -1;      // 1: four waves per 64 scalar multiplications (ec_mul_coop_kernel); 2: four
                                // waves per 4, each element on a 16-lane row (ec_mul_row_kernel); 0: one
                                // lane each; -1 (auto): cooperative when the batch fits one pass of the chip
    int tune_small = 1;      // one-launch small_round_kernel: 0 never, 1 small rounds (auto), 2 whenever legal
    int tune_pairing = 1;    // rows/masks on different tiles: 0 interleaved items, 1 dual-tile items (measured 1.97 vs 3.46 ms),
                             // 2 same-tile window items (plan_window_same; 0.228 vs 0.188 ms at G = 8, r02_ab_window_same.log)
    int tune_expand_waves = 128;  // prg_expand_kernel one-wave workgroups per CU: 16 / 32 / 64 / 128 -> 1.57 / 1.43 /
                                  // 1.37 / 1.34 ms at K = 962, L = 2^20 (profiles/r06_expand_probe_waves*.log); ~9 fit
                                  // a SIMD at once, the rest queue behind them and even out the runs' ends
    int n_cus = 0;               // the device's CU count (flm_init)
    void *bounce = nullptr;      // pinned bounce buffer of the host-pointer entry points (HostCopies)
    void *bounce_dev = nullptr;  // its address for kernels (hipHostGetDevicePointer)
    size_t bounce_cap = 0;
    CopyPool copies;             // the CPU side of HostCopies' bounce-buffer copies
    void *comm = nullptr;    // RCCL communicator state (flm_comm.hip), owned by the context
};

namespace {

int fail(flm_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    g_last_error = buf;
    return code;
}

// Select the context's device for the rest of this entry point; the caller's comes back on return.
#define FLM_ON_DEVICE(ctx)                 \
    flm::rt::DeviceScope dev_scope_;       \
    FLM_HIP((ctx), dev_scope_.set((ctx)->device))

#define FLM_HIP(ctx, expr)                                                                            \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail((ctx), FLM_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                    \
    } while (0)

using flm::rt::round_up;

// A rule's answer (flm_call_args.h) as a refusal: 0, or `code` with the rule's text as the error.
int refuse(flm_ctx *ctx, const char *why, int code = FLM_EINVAL) { return why ? fail(ctx, code, "%s", why) : 0; }
int check_range(flm_ctx *ctx, uint64_t slot0, uint64_t n) {
    return refuse(ctx, flm::rt::slot_range_error(slot0, n), FLM_ERANGE);
}
// c's frac_bits, clip, pack and noise_bits against the codec's rule for n contributors; fills c.bias, and *bias_n
int check_codec(flm_ctx *ctx, flm::CodecParams &c, bool unpacked_ok, int64_t n, uint64_t L_params, uint32_t *bias_n = nullptr) {
    bool range = false;
    const char *why = flm::rt::codec_error(c.frac_bits, c.clip, c.pack, unpacked_ok, c.noise_bits, n, L_params, &range,
                                           &c.bias, bias_n);
    return refuse(ctx, why, range ? FLM_ERANGE : FLM_EINVAL);
}
// the same for the table mode of the noise (tail, and the stream of two blocks per parameter block)
int check_codec_gauss(flm_ctx *ctx, flm::CodecParams &c, int tail, int64_t n, uint64_t L_params) {
    bool range = false;
    const char *why = flm::rt::codec_gauss_error(c.frac_bits, c.clip, c.pack, tail, n, L_params, &range, &c.bias);
    return refuse(ctx, why, range ? FLM_ERANGE : FLM_EINVAL);
}
int check_aggregate_args(flm_ctx *ctx, const uint32_t *d_rows, size_t row_pitch, int N, int K, size_t L, size_t mask_lo,
                         size_t mask_hi, uint64_t prg_slot0, const uint32_t *d_out) {
    bool range = false;
    const char *why = flm::rt::aggregate_error(d_rows, row_pitch, N, K, L, mask_lo, mask_hi, prg_slot0, d_out, &range);
    return refuse(ctx, why, range ? FLM_ERANGE : FLM_EINVAL);
}

// The tuning keys: the context member behind each, the values it takes and the refusal of any
// other (which may print the value).  flm_set_tuning and flm_get_tuning read this one table.
struct TuneKey {
    const char *name;
    int flm_ctx::*member;
    bool (*accepts)(int);
    const char *refusal;
};
template <int Lo, int Hi> bool within(int v) { return v >= Lo && v <= Hi; }
template <int... V> bool one_of(int v) { return ((v == V) || ...); }
const TuneKey kTuneKeys[] = {
    {"variant", &flm_ctx::tune_variant, within<-1, flm::kVarCount - 1>, "variant %d out of range"},
    {"pairing", &flm_ctx::tune_pairing, within<0, 2>, "pairing must be 0, 1 or 2"},
    {"subtiles", &flm_ctx::tune_subtiles, one_of<0, 1, 4, 16>, "subtiles must be 0 (auto), 1, 4 or 16"},
    {"ec_waves", &flm_ctx::tune_ec_waves, one_of<1, 4, 8>, "ec_waves must be 1, 4 or 8"},
    {"small", &flm_ctx::tune_small, within<0, 2>, "small must be 0 (never), 1 (auto) or 2 (when legal)"},
    {"min_items", &flm_ctx::tune_min_items, within<64, 1 << 20>, "min_items must be in [64, 2^20]"},
    {"ec_spread", &flm_ctx::tune_ec_spread, within<0, 64>, "ec_spread must be in [0, 64] KiB"},
    {"ec_terms", &flm_ctx::tune_ec_terms, one_of<1, 2, 4>, "ec_terms must be 1, 2 or 4"},
    {"ec_coop", &flm_ctx::tune_ec_coop, within<-1, 2>, "ec_coop must be -1, 0, 1 or 2"},
    {"expand_waves", &flm_ctx::tune_expand_waves, within<1, 256>, "expand_waves must be in [1, 256]"},
    {"ec_threads", &flm_ctx::tune_ec_threads, one_of<64, 128, 256>, "ec_threads must be 64, 128 or 256"},
};
const TuneKey *tune_key(const char *key) {
    for (const TuneKey &t : kTuneKeys)
        if (!std::strcmp(key, t.name)) return &t;
    return nullptr;
}

// What flm_last_plan reports: the launch just enqueued.
void set_last_plan(flm_ctx *ctx, int items, int tile_slots, int atomics, int variant) {
    ctx->last_items = items, ctx->last_tile = tile_slots, ctx->last_atomics = atomics, ctx->last_variant = variant;
}

// A staging slot of >= `bytes` that no queued work reads any more (StageSlot).  The host
// waits only when all kStageSlots slots are still queued: then for the oldest.
StageSlot *stage_acquire(flm_ctx *ctx, size_t bytes, int *rc) {
    StageSlot *best = nullptr, *free_small = nullptr, *oldest = nullptr;
    for (StageSlot *s : ctx->slots) {
        if (s->busy && event_done(s->done)) s->busy = false;
        if (s->busy) {
            if (!oldest || s->last < oldest->last) oldest = s;
        } else if (s->cap >= bytes) {
            if (!best || s->cap < best->cap) best = s;
        } else if (!free_small) {
            free_small = s;
        }
    }
    if (!best) {
        if (ctx->slots.size() < kStageSlots) {
            best = new StageSlot();
            if (hipEventCreateWithFlags(&best->done, hipEventDisableTiming) != hipSuccess) {
                delete best;
                *rc = fail(ctx, FLM_EHIP, "staging slot: hipEventCreate failed");
                return nullptr;
            }
            ctx->slots.push_back(best);
        } else if (free_small) {
            best = free_small;
        } else {
            if (hipEventSynchronize(oldest->done) != hipSuccess) {
                *rc = fail(ctx, FLM_EHIP, "staging slot: hipEventSynchronize failed");
                return nullptr;
            }
            oldest->busy = false;
            best = oldest;
        }
        if (best->cap < bytes) {
            const size_t want = std::max<size_t>(round_up(bytes, 4096), 4096);
            if (best->host) (void)hipHostFree(best->host);
            best->host = nullptr;
            best->cap = 0;
            hipError_t e = hipHostMalloc(&best->host, want, hipHostMallocDefault);
            if (e == hipSuccess) e = best->dev.reserve(want);
            if (e != hipSuccess) {
                *rc = fail(ctx, FLM_ENOMEM, "staging slot of %zu bytes: %s", want, hipGetErrorString(e));
                return nullptr;
            }
            best->cap = want;
        }
    }
    best->last = ++ctx->slot_clock;
    *rc = 0;
    return best;
}

// A few slots made at flm_init, so the first *_dev calls of a context do not pay the pinned and
// device allocations (c2's client masks: 0.196 ms with a slot allocated in the call, 0.065 ms without).
constexpr int kStagePrealloc = 4;
constexpr size_t kStagePreallocBytes = 256u << 10;

void stage_prealloc(flm_ctx *ctx) {
    for (int i = 0; i < kStagePrealloc; ++i) {
        auto *s = new StageSlot();
        if (hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess ||
            hipHostMalloc(&s->host, kStagePreallocBytes, hipHostMallocDefault) != hipSuccess ||
            s->dev.reserve(kStagePreallocBytes) != hipSuccess) {
            if (s->host) (void)hipHostFree(s->host);
            s->dev.release();
            if (s->done) (void)hipEventDestroy(s->done);
            delete s;
            (void)hipGetLastError();
            return;  // the pool fills lazily instead
        }
        s->cap = kStagePreallocBytes;
        ctx->slots.push_back(s);
    }
}

// The slot is free again once the work enqueued on `s` so far (its readers) has completed.
hipError_t stage_commit(StageSlot *slot, hipStream_t s) {
    hipError_t e = hipEventRecord(slot->done, s);
    if (e == hipSuccess) slot->busy = true;
    return e;
}

// The small tables a *_dev call's kernels read (seg, signs, work items), each `bytes` bytes from `host` or,
// with host NULL, of the byte `fill`.  stage_put packs them back to back into a staging slot that no
// queued work reads (stage_acquire: the host does not wait while the pool can grow) and uploads them on
// `s` as one copy; dev[i] is the device address of piece i.
struct StagePiece {
    const void *host;
    size_t bytes;
    uint8_t fill;
};
struct Staged {
    StageSlot *slot = nullptr;
    const uint8_t *dev[2] = {nullptr, nullptr};
};
int stage_put(flm_ctx *ctx, std::initializer_list<StagePiece> pieces, hipStream_t s, Staged *up) {
    assert(pieces.size() <= 2);
    size_t total = 0;
    for (const StagePiece &p : pieces) total += p.bytes;
    int rc = 0;
    up->slot = stage_acquire(ctx, std::max<size_t>(total, 1), &rc);  // an empty table still has an address
    if (!up->slot) return rc;
    uint8_t *h = static_cast<uint8_t *>(up->slot->host);
    size_t at = 0, i = 0;
    for (const StagePiece &p : pieces) {
        up->dev[i++] = up->slot->dev.as<uint8_t>() + at;
        if (p.bytes && p.host) std::memcpy(h + at, p.host, p.bytes);
        else if (p.bytes) std::memset(h + at, p.fill, p.bytes);
        at += p.bytes;
    }
    if (total) FLM_HIP(ctx, hipMemcpyAsync(up->slot->dev.p, h, total, hipMemcpyHostToDevice, s));
    return 0;
}
// After the launches that read the tables, with `rc` what became of them: the slot is busy until the work
// enqueued so far has run, whether or not it all got enqueued.  -> rc, or the failure to mark the slot.
int stage_done(flm_ctx *ctx, const Staged &up, hipStream_t s, int rc) {
    FLM_HIP(ctx, stage_commit(up.slot, s));
    return rc;
}

// The items go through a staging slot on `s` and the plan records `ready` for launches on
// other streams (run_plan).
int upload_plan(flm_ctx *ctx, Plan &plan, std::vector<Item> &items, hipStream_t s) {
    plan.n_items = (int)items.size();
    if (items.empty()) return 0;
    const size_t bytes = items.size() * sizeof(Item);
    FLM_HIP(ctx, plan.items.reserve(bytes));
    int rc = 0;
    StageSlot *slot = stage_acquire(ctx, bytes, &rc);
    if (!slot) return rc;
    std::memcpy(slot->host, items.data(), bytes);
    FLM_HIP(ctx, hipMemcpyAsync(plan.items.p, slot->host, bytes, hipMemcpyHostToDevice, s));
    FLM_HIP(ctx, stage_commit(slot, s));
    if (!plan.ready) FLM_HIP(ctx, hipEventCreateWithFlags(&plan.ready, hipEventDisableTiming));
    FLM_HIP(ctx, hipEventRecord(plan.ready, s));
    plan.up_stream = s;
    plan.ready_known = false;
    return 0;
}

void plan_free(Plan *plan) {
    plan->items.release();
    if (plan->ready) (void)hipEventDestroy(plan->ready);
    delete plan;  // and with it the events of its launches (StreamMarks)
}

constexpr size_t kPlanCache = 64;        // launch plans kept per context (shapes)

Plan *aggregate_plan(flm_ctx *ctx, uint64_t pitch, int N, int K, uint64_t L, uint64_t mask_lo, uint64_t mask_hi,
                     uint64_t prg_slot0, hipStream_t s, int *rc) {
    PlanKey key{ctx->tune_subtiles + 100 * ctx->tune_pairing + 1000 * ctx->tune_min_items, pitch, (uint64_t)N,
                (uint64_t)K, L, mask_lo, mask_hi, prg_slot0};
    auto f = ctx->plans.find(key);
    if (f != ctx->plans.end()) {
        f->second->last_use = ++ctx->plan_clock;
        *rc = 0;
        return f->second;
    }
    // A full cache (kPlanCache shapes; a server whose seed count changes every round makes a new
    // shape every round) hands its least recently used plan's item buffer and events to the new
    // plan once that plan's last launch has completed -- no hipFree, which would wait for the
    // whole device, and no hipMalloc while the buffer is big enough.
    Plan *plan = nullptr;
    if (ctx->plans.size() >= kPlanCache) {
        auto lru = ctx->plans.begin();
        for (auto it = ctx->plans.begin(); it != ctx->plans.end(); ++it)
            if (it->second->last_use < lru->second->last_use) lru = it;
        Plan *old = lru->second;
        hipError_t e = old->done.sync_all();  // long done, as a rule
        if (e == hipSuccess && old->ready) e = hipEventSynchronize(old->ready);
        if (e != hipSuccess) {
            *rc = fail(ctx, FLM_EHIP, "plan cache: waiting for a recycled plan failed: %s", hipGetErrorString(e));
            return nullptr;
        }
        ctx->plans.erase(lru);
        plan = new Plan();
        plan->items = old->items;  // the buffers move; the old Plan object goes
        plan->ready = old->ready;
        plan->done.swap(old->done);  // (stream, event) pairs: the events are reused per stream
        delete old;
    } else {
        plan = new Plan();
    }
    std::vector<Item> items;
    plan->shape = flm::plan::build_aggregate_items(ctx->tune_subtiles, ctx->tune_pairing, pitch, N, K, L, mask_lo, mask_hi,
                                                   prg_slot0, items, ctx->tune_min_items);
    *rc = upload_plan(ctx, *plan, items, s);
    if (*rc) { plan_free(plan); return nullptr; }
    plan->last_use = ++ctx->plan_clock;
    ctx->plans[key] = plan;
    return plan;
}

// No read or write of `t` on a stream other than s is still pending: s may rewrite it at once.
bool table_free_on(const SeedTable *t, hipStream_t s) {
    if (t->w_stream != s && t->written_valid && !event_done(t->written)) return false;
    return !t->readers.pending_elsewhere(s);
}

// A seed table stream s may overwrite, grown to hold K records and `meta_words` sign-count words
// (SeedTable).  The write launch follows on s; table_written() records it.
SeedTable *table_acquire(flm_ctx *ctx, int K, size_t meta_words, hipStream_t s, int *rc) {
    SeedTable *t = nullptr;
    for (SeedTable *c : ctx->tables)  // the least recently used of the tables s may rewrite at once
        if (table_free_on(c, s) && (!t || c->last_use < t->last_use)) t = c;
    if (!t && ctx->tables.size() < kSeedTables) {
        t = new SeedTable();
        if (hipEventCreateWithFlags(&t->written, hipEventDisableTiming) != hipSuccess) {
            delete t;
            *rc = fail(ctx, FLM_EHIP, "seed table: hipEventCreate failed");
            return nullptr;
        }
        ctx->tables.push_back(t);
    }
    if (!t) {  // every table is still in use on other streams: s waits (on the device) for the oldest
        t = ctx->tables.front();
        for (SeedTable *c : ctx->tables)
            if (c->last_use < t->last_use) t = c;
        hipError_t e = hipSuccess;
        if (t->w_stream != s && t->written_valid) e = hipStreamWaitEvent(s, t->written, 0);
        if (e == hipSuccess) e = t->readers.wait_elsewhere(s);
        if (e != hipSuccess) {
            *rc = fail(ctx, FLM_EHIP, "seed table: hipStreamWaitEvent failed: %s", hipGetErrorString(e));
            return nullptr;
        }
    }
    // growing frees the old buffer: hipFree waits for the device, so no pending launch reads it
    hipError_t e = t->recs.reserve(std::max<size_t>(1, (size_t)K) * sizeof(SeedRec));
    if (e == hipSuccess) e = t->meta.reserve(sizeof(uint32_t) * std::max<size_t>(4, meta_words));
    if (e != hipSuccess) {
        *rc = fail(ctx, FLM_ENOMEM, "seed table of %d seeds: %s", K, hipGetErrorString(e));
        return nullptr;
    }
    t->last_use = ++ctx->table_clock;
    if (ctx->pub_table == t) {  // never left published while it holds other seeds
        ctx->pub_table = nullptr;
        ctx->table_k = -1;
    }
    *rc = 0;
    return t;
}

// The table's write launch has been enqueued on s.  record: mark it with `written` (a published
// table); otherwise the caller's read launch on s follows and table_read() covers both -- or, when
// the read cannot be enqueued, table_cover() records `written` after all.
hipError_t table_written(flm_ctx *ctx, SeedTable *t, hipStream_t s, bool record) {
    t->w_stream = s;
    t->written_valid = record;
    ctx->cur_table = t;
    ctx->last_small = false;
    return record ? hipEventRecord(t->written, s) : hipSuccess;
}

void table_cover(SeedTable *t, hipStream_t s) {
    if (t && !t->written_valid && hipEventRecord(t->written, s) == hipSuccess) t->written_valid = true;
    (void)hipGetLastError();
}

// Before a launch on s that reads t: order it after t's write when that ran on another stream.
hipError_t table_before_read(SeedTable *t, hipStream_t s) {
    if (t->w_stream == s) return hipSuccess;
    if (t->written_valid) return event_done(t->written) ? hipSuccess : hipStreamWaitEvent(s, t->written, 0);
    // (not reached: a write recorded no event only when a read followed)
    const hipEvent_t read = t->readers.event_of(t->w_stream);
    return read ? hipStreamWaitEvent(s, read, 0) : hipSuccess;
}

// A launch that reads t has been enqueued on s: record it as the table's last read on s.
hipError_t table_read(SeedTable *t, hipStream_t s) { return t->readers.record(s); }

void table_free(SeedTable *t) {
    if (t->written && t->written_valid) (void)hipEventSynchronize(t->written);
    (void)t->readers.sync_all();
    t->recs.release();
    t->meta.release();
    if (t->written) (void)hipEventDestroy(t->written);
    delete t;  // and with it the readers' events (StreamMarks)
}

// The one-launch small round builds no seed table: it reads the raw seeds and only WRITES its sign
// counts, into a buffer of its own (flm_check_signs reads them; small rounds racing on several
// streams can only race on that diagnostic, never on a sum).  It unpublishes the table like every
// other entry point that takes seeds, so flm_aggregate_dev cannot pair with its seeds.  No event:
// c2's whole round is ~7 us of host time.
int run_small_round(flm_ctx *ctx, int B, const uint32_t *d_rows, uint64_t pitch, int N, const uint8_t *d_seeds,
                    const int8_t *d_signs, int K, uint64_t L, uint64_t mask_lo, uint64_t mask_hi, uint64_t prg_slot0,
                    uint32_t *d_out, hipStream_t s) {
    FLM_HIP(ctx, ctx->small_meta.reserve(4 * sizeof(uint32_t)));
    FLM_HIP(ctx, flm::launch_small_round(B, d_rows, pitch, N, d_seeds, d_signs, K, L, mask_lo, mask_hi,
                                         (uint32_t)(prg_slot0 / 16), d_out, ctx->small_meta.as<uint32_t>(), s));
    ctx->last_small = true;
    ctx->pub_table = nullptr;
    ctx->table_k = -1;
    return 0;
}

// Build a seed table on s (returned in *out).  zero_out (optional): the round's output,
// zero-filled by the same launch (zero_n words).  Only flm_seed_table_dev publishes the table for a
// later flm_aggregate_dev (publish = true); every other entry point that builds one (prg expansion,
// client masking, pair units, the fused round) withdraws the publication, so aggregate_dev only
// ever unmasks against the seeds of the latest flm_seed_table_dev call, and only until another
// entry point runs.
int run_seed_schedule(flm_ctx *ctx, const uint8_t *d_seeds, const int8_t *d_signs, int K, hipStream_t s,
                      SeedTable **out, uint32_t *zero_out = nullptr, uint64_t zero_n = 0, bool publish = false) {
    const int groups = flm::seed_schedule_groups(K, zero_out ? zero_n : 0);
    int rc = 0;
    SeedTable *t = table_acquire(ctx, K, 2 + 2 * (size_t)groups, s, &rc);
    if (!t) return rc;
    const hipError_t e = flm::launch_seed_schedule(d_seeds, d_signs, K, t->recs.as<SeedRec>(), t->meta.as<uint32_t>(),
                                                   s, zero_out, zero_n);
    if (e != hipSuccess) {
        table_cover(t, s);  // whatever part of it got enqueued
        return fail(ctx, FLM_EHIP, "seed schedule launch: %s", hipGetErrorString(e));
    }
    FLM_HIP(ctx, table_written(ctx, t, s, /*record=*/publish));
    ctx->pub_table = publish ? t : nullptr;
    ctx->table_k = publish ? K : -1;
    *out = t;
    return 0;
}

// zeroed: the output was already zero-filled on this stream (by the seed-schedule launch)
int run_plan(flm_ctx *ctx, Plan &plan, SeedTable *table, const uint32_t *d_rows, uint64_t pitch, uint32_t *d_out,
             size_t out_elems, hipStream_t s, bool zeroed = false) {
    if (!plan.ready_known) {  // the items' copy was enqueued on another stream: order after it
        if (event_done(plan.ready)) plan.ready_known = true;
        else if (s != plan.up_stream) FLM_HIP(ctx, hipStreamWaitEvent(s, plan.ready, 0));
    }
    if (plan.shape.needs_zero && !zeroed) FLM_HIP(ctx, hipMemsetAsync(d_out, 0, out_elems * sizeof(uint32_t), s));
    const int variant_id = flm::plan::pick_variant(ctx->tune_variant, plan.shape);
    FLM_HIP(ctx, table_before_read(table, s));
    FLM_HIP(ctx, flm::launch_items(plan.shape.subtiles, variant_id, plan.items.as<Item>(), plan.n_items, d_rows, pitch,
                                   table->recs.as<SeedRec>(), table->meta.as<uint32_t>(), d_out, s));
    FLM_HIP(ctx, table_read(table, s));
    // one event per stream the plan ran on, after its last launch there: the cache recycles the
    // items only once all of them have completed (no dependency is added between the streams)
    FLM_HIP(ctx, plan.done.record(s));
    set_last_plan(ctx, plan.n_items, flm::kWaveSlots * plan.shape.subtiles, plan.shape.atomics, variant_id);
    return 0;
}

bool host_pinned(const void *p) {
    hipPointerAttribute_t a;
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // pageable memory is not an error here
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// Upload N host rows into the context's row buffer at `pitch`.  Page-locked
// rows (e.g. from flm_host_alloc / PinnedArena) are DMA'd directly; pageable
// rows are packed into a pinned staging ring (kStageBytes per buffer, two
// buffers) so the copy engine sees few large transfers while the CPU fills
// the other buffer.  The VECTOR bodies of the reference are pageable numpy
// arrays (SA_ServiceAgent.py:210).  No pageable row is ever handed to a HIP copy
// (HostCopies below says why).
using flm::rt::kStageBytes;  // flm_host_layout.h
using flm::rt::Piece;
using flm::rt::pieces;

// The two kStageBytes pinned staging buffers of the context (upload_rows, HostCopies' large copies).
int ensure_stage(flm_ctx *ctx) {
    if (ctx->stage_cap >= kStageBytes) return 0;
    for (int b = 0; b < 2; ++b) {
        if (ctx->stage[b]) (void)hipHostFree(ctx->stage[b]);
        ctx->stage[b] = nullptr;
        FLM_HIP(ctx, hipHostMalloc(&ctx->stage[b], kStageBytes, hipHostMallocDefault));
        if (!ctx->stage_done[b]) FLM_HIP(ctx, hipEventCreateWithFlags(&ctx->stage_done[b], hipEventDisableTiming));
    }
    ctx->stage_cap = kStageBytes;
    return 0;
}

int upload_rows(flm_ctx *ctx, const uint32_t *const *rows, int N, size_t L, uint64_t pitch) {
    FLM_HIP(ctx, ctx->rows.reserve(std::max<size_t>(1, (size_t)N) * pitch * sizeof(uint32_t)));
    uint32_t *dst = ctx->rows.as<uint32_t>();
    const size_t row_bytes = L * sizeof(uint32_t);
    const size_t slot_bytes = pitch * sizeof(uint32_t);
    std::vector<int> pageable, pinned;
    for (int i = 0; i < N; ++i) {
        if (!rows[i]) return fail(ctx, FLM_EINVAL, "row %d is NULL", i);
        (host_pinned(rows[i]) ? pinned : pageable).push_back(i);
    }
    if (!pinned.empty()) {
        // Page-locked rows go straight to the device, spread over kCopyStreams
        // streams (several SDMA engines: one stream tops out near 49 GB/s, four
        // reach the link's ~57 GB/s, tools/probes/h2d_probe.hip).  Runs of rows that are
        // contiguous on the host (an arena) move as one copy of up to 16 rows.
        if (!ctx->copy[0]) {
            for (int c = 0; c < kCopyStreams; ++c) {
                FLM_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy[c], hipStreamNonBlocking));
                FLM_HIP(ctx, hipEventCreateWithFlags(&ctx->copy_done[c], hipEventDisableTiming));
            }
            FLM_HIP(ctx, hipEventCreateWithFlags(&ctx->copy_start, hipEventDisableTiming));
        }
        // the row buffer may still be read by the previous round on ctx->stream
        FLM_HIP(ctx, hipEventRecord(ctx->copy_start, ctx->stream));
        for (int c = 0; c < kCopyStreams; ++c) FLM_HIP(ctx, hipStreamWaitEvent(ctx->copy[c], ctx->copy_start, 0));
        int next = 0;
        for (size_t k = 0; k < pinned.size();) {
            const int first = pinned[k];
            size_t n = 1;
            while (pitch == L && n < 16 && k + n < pinned.size() && pinned[k + n] == first + (int)n &&
                   rows[first + n] == rows[first] + n * L)
                ++n;
            FLM_HIP(ctx, hipMemcpyAsync(dst + (size_t)first * pitch, rows[first], (n - 1) * slot_bytes + row_bytes,
                                        hipMemcpyHostToDevice, ctx->copy[next]));
            next = (next + 1) % kCopyStreams;
            k += n;
        }
        for (int c = 0; c < kCopyStreams; ++c) {
            FLM_HIP(ctx, hipEventRecord(ctx->copy_done[c], ctx->copy[c]));
            FLM_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->copy_done[c], 0));
        }
    }
    if (pageable.empty()) return 0;
    if (int rc = ensure_stage(ctx)) return rc;
    size_t k = 0;
    int b = 0;
    bool used[2] = {false, false};
    if (slot_bytes > kStageBytes) {  // very long rows: each in kStageBytes pieces through the same ring
        const std::vector<Piece> ps = pieces(row_bytes, 1);
        for (int i : pageable)
            for (const Piece &p : ps) {
                if (used[b]) FLM_HIP(ctx, hipEventSynchronize(ctx->stage_done[b]));
                ctx->copies.copy2d(ctx->stage[b], p.w, reinterpret_cast<const uint8_t *>(rows[i]) + p.c, p.w, p.w, 1);
                FLM_HIP(ctx, hipMemcpyAsync(reinterpret_cast<uint8_t *>(dst + (size_t)i * pitch) + p.c, ctx->stage[b], p.w,
                                            hipMemcpyHostToDevice, ctx->stream));
                FLM_HIP(ctx, hipEventRecord(ctx->stage_done[b], ctx->stream));
                used[b] = true;
                b ^= 1;
            }
        return 0;
    }
    const size_t per_buf = kStageBytes / slot_bytes;  // rows per staging buffer
    while (k < pageable.size()) {
        if (used[b]) FLM_HIP(ctx, hipEventSynchronize(ctx->stage_done[b]));  // DMA out of this buffer done
        uint8_t *st = static_cast<uint8_t *>(ctx->stage[b]);
        // a run of consecutive row indices packs into one contiguous device range
        const int first = pageable[k];
        size_t n = 0;
        while (k + n < pageable.size() && n < per_buf && pageable[k + n] == first + (int)n) {
            ctx->copies.copy2d(st + n * slot_bytes, row_bytes, rows[pageable[k + n]], row_bytes, row_bytes, 1);
            ++n;
        }
        FLM_HIP(ctx, hipMemcpyAsync(dst + (size_t)first * pitch, st, n * slot_bytes - (slot_bytes - row_bytes),
                                    hipMemcpyHostToDevice, ctx->stream));
        FLM_HIP(ctx, hipEventRecord(ctx->stage_done[b], ctx->stream));
        used[b] = true;
        k += n;
        b ^= 1;
    }
    return 0;
}

// The host-pointer entry points move the caller's arrays through the context's pinned bounce
// buffer (ctx->bounce), never straight between a HIP copy and the caller's pageable pages.  For a
// large pageable copy the HIP runtime pins those pages for the DMA (a KFD userptr allocation; its log:
// "HSA Copy Using Pinned resource"); when the process later unmaps them (a numpy array freed), the
// driver evicts ALL of the process's GPU queues while it revalidates: 20-40 ms in which nothing of
// ours runs.  That was the agent run's unmask stall (the driver's per-process
// evicted_ms grows by exactly the stall, and the stalls go away when the runtime never pins,
// GPU_PINNED_MIN_XFER_SIZE).  The runtime's rect path (hipMemcpy2DAsync straight on the caller's
// array) logs no pinning but brings the evictions back all the same (5 of 5 runs,
// profiles/r06_rect_path_evictions.log), so every caller array, small or large, goes through the
// bounce buffer; the CPU side of the copies is split over the context's CopyPool, and a call whose
// arrays fit may run its kernel on the bounce buffer in place.  One bounce buffer per context: these
// calls are synchronous (or, for a group's ranks, synchronised before the call returns), so a call
// reuses it only after the last call's copies out of it have completed.
// Copies of kStageBytes or more skip it and stream through the context's two staging buffers instead
// (inputs in begin(), outputs in finish()), so no call pins more host memory than its small copies
// plus 2 x 32 MiB, whatever its size (a 962 x 2^20 prg_expand returns 4 GiB).
// A call declares the arrays it moves, as its list in flm_call_args.h (declare()), then begin(), then runs
// its *_dev twin on the arrays' device pointers and pitches, then finish().  The routes and the bounce layout
// come from the list alone (flm::rt::host_layout): no call site adds up bytes, picks a buffer or chooses a path.
class HostCopies {
  public:
    // A declared array.  After begin(): `dev`, rows `pitch` bytes apart, is where the kernel reads or
    // writes it -- the named DevBuf at the declared pitch, or the bounce buffer itself in place.
    struct Span {
        void *dev = nullptr;
        size_t pitch = 0;
        template <class T>
        T *as() const { return static_cast<T *>(dev); }
    };
    HostCopies(flm_ctx *ctx, hipStream_t s) : ctx_(ctx), s_(s) {}
    // an error return between begin() and finish() leaves nothing queued on the bounce buffer
    ~HostCopies() { if (open_) (void)hipStreamSynchronize(s_); }
    // Every array of the call's list (flm_call_args.h) that is present, with the host pointer at the same
    // position: rows x width bytes, host rows at h_pitch; through device memory they land in the list's
    // scratch buffer at d_pitch.  After begin(), dev<T>(i) is where the kernel finds array i (NULL: absent)
    // and pitch(i) the bytes between its rows there.
    void declare(const flm::rt::ArgList &l, std::initializer_list<const void *> host) {
        assert((int)host.size() == l.n);
        twice_ = flm::rt::names_slot_twice(l);
        for (int i = 0; i < l.n; ++i) {
            const flm::rt::Arg &a = l.a[i];
            arg_[i] = !a.present ? nullptr
                                 : add(const_cast<void *>(host.begin()[i]), a.h_pitch, a.width, a.rows, ctx_->*kSlot[a.slot],
                                       a.d_pitch, a.is_out, a.in_place ? kMayRunInPlace : kDevice);
        }
    }
    template <class T>
    T *dev(int i) const { return arg_[i] ? arg_[i]->as<T>() : nullptr; }
    size_t pitch(int i) const { return arg_[i]->pitch; }
    // Lays the call out, grows the bounce buffer and the DevBufs, copies the inputs into pinned memory
    // and enqueues their DMAs (large ones stream through the staging ring at once).
    int begin() {
        if (n_ > kMaxSpans) return fail(ctx_, FLM_EINVAL, "host copies: more than %d arrays declared", kMaxSpans);
        if (twice_) return fail(ctx_, FLM_EINVAL, "host copies: two arrays of the call share a scratch buffer");
        const size_t total = flm::rt::host_layout(lay_, n_);
        if (total > ctx_->bounce_cap) {
            if (ctx_->bounce) (void)hipHostFree(ctx_->bounce);  // waits for the device: nothing reads it after
            ctx_->bounce = nullptr;
            ctx_->bounce_cap = 0;
            const size_t want = flm::rt::grow_bytes(total);
            const hipError_t e = hipHostMalloc(&ctx_->bounce, want, hipHostMallocDefault);
            if (e != hipSuccess) return fail(ctx_, FLM_ENOMEM, "pinned bounce buffer of %zu bytes: %s", want, hipGetErrorString(e));
            ctx_->bounce_cap = want;
            FLM_HIP(ctx_, hipHostGetDevicePointer(&ctx_->bounce_dev, ctx_->bounce, 0));
        }
        for (int i = 0; i < n_; ++i)
            if (lay_[i].route != flm::rt::kRouteInPlace)
                FLM_HIP(ctx_, spans_[i].buf->reserve(std::max<size_t>(1, lay_[i].rows * spans_[i].d_pitch)));
        open_ = n_ > 0;
        for (int i = 0; i < n_; ++i) {
            Decl &sp = spans_[i];
            const flm::rt::HostSpan &l = lay_[i];
            const bool in_place = l.route == flm::rt::kRouteInPlace;
            sp.b = static_cast<uint8_t *>(ctx_->bounce) + l.offset;
            sp.dev = in_place ? static_cast<uint8_t *>(ctx_->bounce_dev) + l.offset : sp.buf->p;
            sp.pitch = in_place ? l.pitch : sp.d_pitch;
            if (sp.is_out || !l.width || !l.rows) continue;
            if (l.route == flm::rt::kRouteRing) {
                if (int rc = stream_in(sp, l)) return rc;
                continue;
            }
            ctx_->copies.copy2d(sp.b, l.pitch, sp.host, sp.h_pitch, l.width, l.rows);
            if (!in_place) FLM_HIP(ctx_, dma(sp.dev, sp.d_pitch, sp.b, l.pitch, l, hipMemcpyHostToDevice));
        }
        return 0;
    }
    // DMA the outputs that went through device memory into the bounce buffer, wait for the stream, then
    // copy every output to the caller (large ones through the staging ring)
    int finish() {
        for (int i = 0; i < n_; ++i)
            if (spans_[i].is_out && lay_[i].route == flm::rt::kRouteBounce && lay_[i].width && lay_[i].rows)
                FLM_HIP(ctx_, dma(spans_[i].b, lay_[i].pitch, spans_[i].dev, spans_[i].d_pitch, lay_[i], hipMemcpyDeviceToHost));
        FLM_HIP(ctx_, hipStreamSynchronize(s_));
        open_ = false;
        for (int i = 0; i < n_; ++i) {
            const Decl &sp = spans_[i];
            const flm::rt::HostSpan &l = lay_[i];
            if (!sp.is_out || !l.width || !l.rows) continue;
            if (l.route != flm::rt::kRouteRing) ctx_->copies.copy2d(sp.host, sp.h_pitch, sp.b, l.pitch, l.width, l.rows);
            else if (int rc = stream_out(sp, l)) return rc;
        }
        return 0;
    }
    // the caller synchronises the stream itself before the bounce buffer's next use (a group's ranks)
    void hand_over() { open_ = false; }

  private:
    enum Place { kDevice, kMayRunInPlace };
    static constexpr int kMaxSpans = flm::rt::kMaxArgs;
    // flm::rt::Slot -> the context's buffer of that name
    static constexpr DevBuf flm_ctx::*kSlot[flm::rt::kSlots] = {
        &flm_ctx::ec_in,  &flm_ctx::ec_base,  &flm_ctx::ec_scal,  &flm_ctx::ec_out,
        &flm_ctx::ec_dig, &flm_ctx::ec_flags, &flm_ctx::bytes_in, &flm_ctx::bytes_out,
        &flm_ctx::rows,   &flm_ctx::out,      &flm_ctx::seeds,    &flm_ctx::signs};
    struct Decl : Span {  // a declaration behind its handle; its width, rows and route are lay_[i], as host_layout takes them
        void *host;
        size_t h_pitch, d_pitch;
        DevBuf *buf;
        bool is_out;
        uint8_t *b;
    };
    const Span *add(void *h, size_t h_pitch, size_t width, size_t rows, DevBuf &buf, size_t d_pitch, bool is_out, Place p) {
        if (n_ >= kMaxSpans) {  // one too many: begin() refuses the call
            n_ = kMaxSpans + 1;
            return &spans_[0];
        }
        lay_[n_] = {width, rows, p == kMayRunInPlace};
        Decl &sp = spans_[n_++];
        sp.host = h, sp.h_pitch = h_pitch, sp.d_pitch = d_pitch, sp.buf = &buf, sp.is_out = is_out;
        return &sp;
    }
    // l.rows x l.width bytes between the bounce buffer and device memory, enqueued on the stream
    hipError_t dma(void *dst, size_t d_pitch, const void *src, size_t s_pitch, const flm::rt::HostSpan &l, hipMemcpyKind k) {
        return l.rows == 1 ? hipMemcpyAsync(dst, src, l.width, k, s_)
                           : hipMemcpy2DAsync(dst, d_pitch, src, s_pitch, l.width, l.rows, k, s_);
    }
    // a large input: each piece copied into the next free staging buffer, then DMA'd from it
    int stream_in(const Decl &sp, const flm::rt::HostSpan &l) {
        if (int rc = ensure_stage(ctx_)) return rc;
        const auto *src = static_cast<const uint8_t *>(sp.host);
        auto *dst = static_cast<uint8_t *>(sp.dev);
        int b = 0;
        for (const Piece &p : pieces(l.width, l.rows)) {
            FLM_HIP(ctx_, hipEventSynchronize(ctx_->stage_done[b]));  // the DMA out of this buffer is done
            auto *st = static_cast<uint8_t *>(ctx_->stage[b]);
            ctx_->copies.copy2d(st, p.w, src + p.r * sp.h_pitch + p.c, sp.h_pitch, p.w, p.nr);
            FLM_HIP(ctx_, hipMemcpy2DAsync(dst + p.r * sp.d_pitch + p.c, sp.d_pitch, st, p.w, p.w, p.nr, hipMemcpyHostToDevice, s_));
            FLM_HIP(ctx_, hipEventRecord(ctx_->stage_done[b], s_));
            b ^= 1;
        }
        return 0;
    }
    // a large output, after the stream has drained: piece i + 1 lands in one staging buffer while
    // piece i is copied out of the other
    int stream_out(const Decl &sp, const flm::rt::HostSpan &l) {
        if (int rc = ensure_stage(ctx_)) return rc;
        const std::vector<Piece> ps = pieces(l.width, l.rows);
        auto issue = [&](size_t i) -> int {
            const Piece &p = ps[i];
            FLM_HIP(ctx_, hipMemcpy2DAsync(ctx_->stage[i & 1], p.w, sp.as<const uint8_t>() + p.r * sp.d_pitch + p.c, sp.d_pitch,
                                           p.w, p.nr, hipMemcpyDeviceToHost, s_));
            FLM_HIP(ctx_, hipEventRecord(ctx_->stage_done[i & 1], s_));
            return 0;
        };
        for (size_t i = 0; i < ps.size() && i < 2; ++i)
            if (int rc = issue(i)) return rc;
        for (size_t i = 0; i < ps.size(); ++i) {
            const Piece &p = ps[i];
            FLM_HIP(ctx_, hipEventSynchronize(ctx_->stage_done[i & 1]));
            ctx_->copies.copy2d(static_cast<uint8_t *>(sp.host) + p.r * sp.h_pitch + p.c, sp.h_pitch, ctx_->stage[i & 1], p.w,
                                p.w, p.nr);
            if (i + 2 < ps.size())
                if (int rc = issue(i + 2)) return rc;
        }
        return 0;
    }
    flm_ctx *ctx_;
    hipStream_t s_;
    Decl spans_[kMaxSpans + 1];
    flm::rt::HostSpan lay_[kMaxSpans + 1];  // spans_[i]'s width, rows and may-run-in-place; its route after begin()
    const Span *arg_[kMaxSpans] = {};  // declare()'s arrays by their place in the list
    int n_ = 0;
    bool twice_ = false;  // declare()'s list names a scratch buffer twice: begin() refuses the call
    bool open_ = false;  // begin() has queued work or handed out in-place memory, finish() has not waited yet
};

// Client masking / expansion (flm::plan::plan_rows_jobs plans it): stages the items and the signs
// (stage_put), builds the seed table and launches.  signs: K host signs, or NULL for all +1 (expansion).
int run_rows_jobs(flm_ctx *ctx, const uint32_t *d_x, uint64_t pitch, int N, const int64_t *seg, const int8_t *signs,
                  const uint8_t *d_seeds, int K, uint32_t base_bias, size_t L, uint64_t slot0, uint32_t *d_out,
                  hipStream_t s) {
    std::vector<Item> items;
    const PlanShape shape = flm::plan::plan_rows_jobs(d_x != nullptr, pitch, N, seg, signs, K, base_bias, L, slot0, items);
    const int n_items = (int)items.size();
    Staged up;
    if (int rc = stage_put(ctx, {{items.data(), items.size() * sizeof(Item), 0}, {signs, (size_t)K, 1}}, s, &up)) return rc;
    SeedTable *table = nullptr;
    int rc = run_seed_schedule(ctx, d_seeds, reinterpret_cast<const int8_t *>(up.dev[1]), K, s, &table);
    if (!rc && shape.needs_zero) {
        const hipError_t e = hipMemsetAsync(d_out, 0, (size_t)N * pitch * sizeof(uint32_t), s);
        if (e != hipSuccess) rc = fail(ctx, FLM_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    const int variant_id = flm::plan::pick_variant(ctx->tune_variant, shape);
    if (!rc && n_items) {
        hipError_t e = flm::launch_items(shape.subtiles, variant_id, reinterpret_cast<const Item *>(up.dev[0]), n_items, d_x,
                                         pitch, table->recs.as<SeedRec>(), table->meta.as<uint32_t>(), d_out, s);
        if (e == hipSuccess) e = table_read(table, s);
        if (e != hipSuccess) rc = fail(ctx, FLM_EHIP, "items launch: %s", hipGetErrorString(e));
    }
    if (table && (rc || !n_items)) table_cover(table, s);  // no read recorded after the table's write
    if ((rc = stage_done(ctx, up, s, rc))) return rc;
    set_last_plan(ctx, n_items, flm::kWaveSlots * shape.subtiles, shape.atomics, variant_id);
    return 0;
}

// A round on host rows: flm_aggregate_unmask (out: the caller's array; the call returns with it written)
// and one rank's share of a group's round (out NULL: the sum stays in d_out on the device, and the group
// synchronises every rank before its call returns).
int host_round(flm_ctx *ctx, const uint32_t *const *rows, int N, const uint8_t *seeds, const int8_t *signs, int K,
               size_t L, size_t mask_lo, size_t mask_hi, uint32_t *out, uint32_t *d_out) {
    if (N < 0 || K < 0) return fail(ctx, FLM_EINVAL, "negative N or K");
    if ((N > 0 && !rows) || (!out && !d_out)) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (K > 0 && (!seeds || !signs)) return fail(ctx, FLM_EINVAL, "NULL seeds/signs");
    if (int rc = refuse(ctx, flm::rt::signs_error(signs, K))) return rc;
    if (int rc = check_range(ctx, 0, L)) return rc;
    FLM_ON_DEVICE(ctx);
    const uint64_t pitch = round_up(L, 64);
    if (int rc = upload_rows(ctx, rows, N, L, pitch)) return rc;
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::aggregate_unmask_args(K, L, out != nullptr), {seeds, signs, out});
    if (int rc = hc.begin()) return rc;
    if (int rc = flm_aggregate_unmask_dev(ctx, ctx->rows.as<uint32_t>(), pitch, N, hc.dev<uint8_t>(0), hc.dev<int8_t>(1), K,
                                          L, mask_lo, mask_hi, 0, out ? hc.dev<uint32_t>(2) : d_out, ctx->stream))
        return rc;
    if (out) return hc.finish();
    hc.hand_over();
    return 0;
}

}  // namespace

namespace flm {
namespace rt {
int set_error(flm_ctx *ctx, int code, const char *msg) { return fail(ctx, code, "%s", msg); }
int device_of(const flm_ctx *ctx) { return ctx->device; }
hipStream_t stream_of(const flm_ctx *ctx) { return ctx->stream; }
void **comm_slot(flm_ctx *ctx) { return &ctx->comm; }
void host_copy(flm_ctx *ctx, void *dst, const void *src, size_t n) { ctx->copies.copy2d(dst, n, src, n, n, 1); }

int host_round_async(flm_ctx *ctx, const uint32_t *const *rows, int N, const uint8_t *seeds, const int8_t *signs,
                     int K, size_t L, size_t mask_lo, size_t mask_hi, uint32_t *d_out) {
    return host_round(ctx, rows, N, seeds, signs, K, L, mask_lo, mask_hi, nullptr, d_out);
}

}  // namespace rt
}  // namespace flm

// ======================================================================= ABI
extern "C" {

int flm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *flm_version(void) { return "flamingo_hip 0.6 gfx950 items_kernel<S={1,4,16}> (0.4 + shamir_deal, aes_gcm_xor, aes_gcm_seal, aes_gcm_open) + feldman_verify + codec + pack{2,4} + dp_noise + rotate + l2_clip + round_bound + dp_gauss + modular"; }

int flm_init(flm_ctx **out, int device) {
    if (!out) return fail(nullptr, FLM_EINVAL, "flm_init: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, FLM_EHIP, "flm_init: no HIP device visible (%s)", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(nullptr, FLM_EINVAL, "flm_init: device %d out of range [0,%d)", device, n);
    flm::rt::DeviceScope dev_scope_;
    e = dev_scope_.set(device);
    if (e != hipSuccess) return fail(nullptr, FLM_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    flm_ctx *ctx = new flm_ctx();
    ctx->device = device;
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;
        return fail(nullptr, FLM_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    if (hipDeviceGetAttribute(&ctx->n_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        (void)hipGetLastError();
        ctx->n_cus = 256;  // MI355X
    }
    stage_prealloc(ctx);
    *out = ctx;
    return 0;
}

void flm_free(flm_ctx *ctx) {
    if (!ctx) return;
    flm::rt::DeviceScope dev_scope_(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    // collectives may sit on a caller's stream (a torch comm stream), not the context's: the whole
    // device completes before the communicator is finalised (flm_comm_destroy does the same)
    if (ctx->comm) (void)hipDeviceSynchronize();
    flm::comm_release(ctx);
    for (StageSlot *s : ctx->slots) (void)hipEventSynchronize(s->done);  // launches on other streams
    for (auto &kv : ctx->plans) plan_free(kv.second);
    for (SeedTable *t : ctx->tables) table_free(t);  // waits for the table's readers on every stream
    if (ctx->small_meta.p) (void)hipDeviceSynchronize();  // small rounds on any stream may still write it
    ctx->small_meta.release();
    for (DevBuf *b : {&ctx->rows, &ctx->out, &ctx->seeds, &ctx->signs, &ctx->bytes_in, &ctx->bytes_out, &ctx->ec_in,
                      &ctx->ec_base, &ctx->ec_scal, &ctx->ec_jac, &ctx->ec_out, &ctx->ec_dig, &ctx->ec_flags, &ctx->rot_signs, &ctx->l2_work})
        b->release();
    for (StageSlot *s : ctx->slots) {
        if (s->host) (void)hipHostFree(s->host);
        s->dev.release();
        (void)hipEventDestroy(s->done);
        delete s;
    }
    if (ctx->bounce) (void)hipHostFree(ctx->bounce);
    for (int i = 0; i < 2; ++i) {
        if (ctx->stage[i]) (void)hipHostFree(ctx->stage[i]);
        if (ctx->stage_done[i]) (void)hipEventDestroy(ctx->stage_done[i]);
    }
    for (int c = 0; c < 4; ++c) {
        if (ctx->copy[c]) (void)hipStreamSynchronize(ctx->copy[c]);
        if (ctx->copy[c]) (void)hipStreamDestroy(ctx->copy[c]);
        if (ctx->copy_done[c]) (void)hipEventDestroy(ctx->copy_done[c]);
    }
    if (ctx->copy_start) (void)hipEventDestroy(ctx->copy_start);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

void *flm_ctx_stream(flm_ctx *ctx) { return ctx ? static_cast<void *>(ctx->stream) : nullptr; }

const char *flm_last_error(const flm_ctx *ctx) {
    if (ctx) return ctx->err.c_str();
    return g_last_error.c_str();
}

int flm_aggregate_unmask(flm_ctx *ctx, const uint32_t *const *rows, int N, const uint8_t *seeds, const int8_t *signs,
                         int K, size_t L, uint32_t *out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (N >= 0 && K >= 0 && L == 0) return 0;  // no slots: nothing read, nothing written
    if (!out) return fail(ctx, FLM_EINVAL, "NULL argument");
    return host_round(ctx, rows, N, seeds, signs, K, L, 0, L, out, nullptr);
}

int flm_seed_table_dev(flm_ctx *ctx, const uint8_t *d_seeds, const int8_t *d_signs, int K, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (K < 0) return fail(ctx, FLM_EINVAL, "negative K");
    if (K > 0 && (!d_seeds || !d_signs)) return fail(ctx, FLM_EINVAL, "NULL seeds/signs");
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
    FLM_ON_DEVICE(ctx);
    SeedTable *t = nullptr;
    return run_seed_schedule(ctx, d_seeds, d_signs, K, s, &t, nullptr, 0, /*publish=*/true);
}

int flm_aggregate_dev(flm_ctx *ctx, const uint32_t *d_rows, size_t row_pitch, int N, int K, size_t L, size_t mask_lo,
                      size_t mask_hi, uint64_t prg_slot0, uint32_t *d_out, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (L == 0) return 0;
    if (int rc = check_aggregate_args(ctx, d_rows, row_pitch, N, K, L, mask_lo, mask_hi, prg_slot0, d_out)) return rc;
    if (!ctx->pub_table || K != ctx->table_k)
        return fail(ctx, FLM_EINVAL, "K=%d does not match the seed table (%d)", K, ctx->table_k);
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
    FLM_ON_DEVICE(ctx);
    int rc = 0;
    Plan *plan = aggregate_plan(ctx, row_pitch, N, K, L, mask_lo, mask_hi, prg_slot0, s, &rc);
    if (!plan) return rc;
    return run_plan(ctx, *plan, ctx->pub_table, d_rows, row_pitch, d_out, L, s);
}

int flm_aggregate_unmask_dev(flm_ctx *ctx, const uint32_t *d_rows, size_t row_pitch, int N, const uint8_t *d_seeds,
                             const int8_t *d_signs, int K, size_t L, size_t mask_lo, size_t mask_hi,
                             uint64_t prg_slot0, uint32_t *d_out, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (L == 0) return 0;
    if (int rc = check_aggregate_args(ctx, d_rows, row_pitch, N, K, L, mask_lo, mask_hi, prg_slot0, d_out)) return rc;
    if (K > 0 && (!d_seeds || !d_signs)) return fail(ctx, FLM_EINVAL, "NULL seeds/signs");
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
    FLM_ON_DEVICE(ctx);
    int rc = 0;
    if (const int B = flm::plan::small_round_width(ctx->tune_small, N, K, L, mask_lo, mask_hi)) {
        // one submission; the device seed table is not built, so flm_aggregate_dev must not reuse it
        if ((rc = run_small_round(ctx, B, d_rows, row_pitch, N, d_seeds, d_signs, K, L, mask_lo, mask_hi, prg_slot0,
                                  d_out, s)))
            return rc;
        const int slots = flm::small_round_slots(B);
        set_last_plan(ctx, (int)((L + slots - 1) / slots), slots, 0, kSmallRoundVariant);
        return 0;
    }
    Plan *plan = aggregate_plan(ctx, row_pitch, N, K, L, mask_lo, mask_hi, prg_slot0, s, &rc);
    if (!plan) return rc;
    // two submissions: seed schedule (+ the zero-fill an atomics plan needs), then the items
    SeedTable *table = nullptr;
    if ((rc = run_seed_schedule(ctx, d_seeds, d_signs, K, s, &table, plan->shape.needs_zero ? d_out : nullptr, L))) return rc;
    if ((rc = run_plan(ctx, *plan, table, d_rows, row_pitch, d_out, L, s, plan->shape.needs_zero))) table_cover(table, s);
    return rc;
}

// The round path's calls in their two forms.  Each host form: the rule it shares with its twin, its own
// checks (what it must know before it reads an array or returns for an empty call), then its list of
// arrays (flm_call_args.h) through HostCopies around the *_dev twin on the context's stream.  Which
// sizes count as empty is one line per form (DESIGN.md has the table).

int flm_client_mask(flm_ctx *ctx, const uint32_t *x, int N, const int64_t *seg, const uint8_t *seeds,
                    const int8_t *signs, size_t L, uint32_t *out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (N < 0) return fail(ctx, FLM_EINVAL, "negative N");
    if (N == 0 || L == 0) return 0;
    int64_t K = 0;
    if (int rc = refuse(ctx, flm::rt::client_args_error(out != nullptr, N, seg, seeds, signs, &K))) return rc;
    if (int rc = check_range(ctx, 0, L)) return rc;
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::client_mask_args(N, K, L, x), {x, seeds, signs, out});
    if (int rc = hc.begin()) return rc;
    assert(!x || hc.pitch(0) == hc.pitch(3));
    if (int rc = flm_client_mask_dev(ctx, hc.dev<uint32_t>(0), hc.pitch(3) / 4, N, seg, hc.dev<uint8_t>(1), signs, L,
                                     hc.dev<uint32_t>(3), ctx->stream))
        return rc;
    return hc.finish();
}

int flm_client_mask_dev(flm_ctx *ctx, const uint32_t *d_x, size_t pitch, int N, const int64_t *seg,
                        const uint8_t *d_seeds, const int8_t *signs, size_t L, uint32_t *d_out, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (N <= 0 || L == 0) return 0;
    int64_t K = 0;  // seg sizes the launch
    if (int rc = refuse(ctx, flm::rt::client_args_error(d_out != nullptr, N, seg, d_seeds, signs, &K))) return rc;
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(pitch, L))) return rc;
    if (int rc = refuse(ctx, flm::rt::align16_error({d_x, d_out}))) return rc;
    if (int rc = check_range(ctx, 0, L)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
    FLM_ON_DEVICE(ctx);
    // small batches (c2: 128 clients x ~15 seeds x 16384 slots): one launch of the small-round
    // kernel, one workgroup per (client, 256-slot tile), instead of a seed schedule + one 1024-thread
    // workgroup per client row.  seg and signs travel in ONE host-to-device copy.
    if (N <= 65535 /* grid.y */ && (ctx->tune_small == 2 || (ctx->tune_small == 1 && (uint64_t)K * L <= (1ull << 26)))) {
        Staged up;
        if (int rc = stage_put(ctx, {{seg, (size_t)(N + 1) * sizeof(int64_t), 0}, {signs, (size_t)K, 0}}, s, &up)) return rc;
        const hipError_t e = flm::launch_small_client_mask(d_x, pitch, N, reinterpret_cast<const int64_t *>(up.dev[0]), d_seeds,
                                                           reinterpret_cast<const int8_t *>(up.dev[1]), L, d_x ? 0u : 1u,
                                                           d_out, s);
        if (int rc = stage_done(ctx, up, s, 0)) return rc;
        FLM_HIP(ctx, e);
        set_last_plan(ctx, (int)(((L + 255) / 256) * (uint64_t)N), 256, 0, kSmallRoundVariant);
        return 0;
    }
    // signs go to the device with the work items (the schedule folds them into xorc)
    return run_rows_jobs(ctx, d_x, pitch, N, seg, signs, d_seeds, (int)K, 1u, L, 0, d_out, s);
}

// ---- the fixed-point codec: float rows in, ring rows of ceil(L / pack) words out, and the mean of a sum back
// (flm_call_args.h has the rule).  One body per call shape; an entry point fixes its pack and noise_bits and whether
// it admits pack = 1 (the packed calls do not: pack = 1 is the unpacked calls' job).

namespace {

// The table mode of the noise (flm_client_encode_gauss_mask[_dev]): the tail and the table, on the host or the device
// as the call's other arrays are.  The calls without it pass none.
struct GaussNoise {
    int tail;
    const uint64_t *cdt;
};

int encode_mask_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, const int64_t *seg, const uint8_t *d_seeds,
                    const int8_t *signs, size_t L, flm::CodecParams c, bool unpacked_ok, const uint8_t *d_dither,
                    const uint8_t *d_noise, const GaussNoise *gauss, uint32_t *d_out, size_t out_pitch, uint32_t *d_clipped,
                    void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = gauss ? check_codec_gauss(ctx, c, gauss->tail, 1, L) : check_codec(ctx, c, unpacked_ok, 1, L)) return rc;
    if (c.noise_bits && !d_noise) return fail(ctx, FLM_EINVAL, "noise_bits > 0 needs the clients' noise seeds");
    if (gauss && (!d_noise || !gauss->cdt)) return fail(ctx, FLM_EINVAL, "the table mode needs the clients' noise seeds and the table");
    if (gauss)
        if (int rc = refuse(ctx, flm::rt::cdt_align_error(gauss->cdt))) return rc;
    if (N <= 0 || L == 0) return 0;
    const size_t Lw = flm::rt::packed_words(L, c.pack);
    int64_t K = 0;
    if (int rc = refuse(ctx, flm::rt::client_args_error(d_x && d_out, N, seg, d_seeds, signs, &K))) return rc;
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(x_pitch, L))) return rc;
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(out_pitch, Lw))) return rc;
    if (int rc = refuse(ctx, flm::rt::align16_error({d_x, d_out}))) return rc;
    if (int rc = check_range(ctx, 0, L)) return rc;  // the dither stream is indexed by parameter
    if (int rc = refuse(ctx, flm::rt::encode_mask_launch_error(flm::encode_mask_groups(N, Lw)))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
    FLM_ON_DEVICE(ctx);
    Staged up;  // seg and signs in one host-to-device copy, as flm_client_mask_dev's
    if (int rc = stage_put(ctx, {{seg, (size_t)(N + 1) * sizeof(int64_t), 0}, {signs, (size_t)K, 0}}, s, &up)) return rc;
    hipError_t e = d_clipped ? hipMemsetAsync(d_clipped, 0, (size_t)N * sizeof(uint32_t), s) : hipSuccess;
    const int64_t *d_seg = reinterpret_cast<const int64_t *>(up.dev[0]);
    const int8_t *d_signs = reinterpret_cast<const int8_t *>(up.dev[1]);
    if (e == hipSuccess)
        e = gauss ? flm::launch_encode_gauss_mask(d_x, x_pitch, N, d_seg, d_seeds, d_signs, d_dither, d_noise, gauss->cdt,
                                                  gauss->tail, L, c, d_out, out_pitch, d_clipped, s)
                  : flm::launch_encode_mask(d_x, x_pitch, N, d_seg, d_seeds, d_signs, d_dither, d_noise, L, c, d_out,
                                            out_pitch, d_clipped, s);
    if (int rc = stage_done(ctx, up, s, 0)) return rc;
    FLM_HIP(ctx, e);
    return 0;
}

// the codec before N < 0 (the plain and packed entry points refuse a negative N first, themselves); the noise
// seeds are wanted, and travel, only when noise_bits > 0; in the table mode they and the table always do, the table
// checked here, where it can be seen
int encode_mask_host(flm_ctx *ctx, const float *x, int N, const int64_t *seg, const uint8_t *seeds, const int8_t *signs,
                     size_t L, flm::CodecParams c, bool unpacked_ok, const uint8_t *dither, const uint8_t *noise,
                     const GaussNoise *gauss, uint32_t *out, uint32_t *clipped) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = gauss ? check_codec_gauss(ctx, c, gauss->tail, 1, L) : check_codec(ctx, c, unpacked_ok, 1, L)) return rc;
    if (N < 0) return fail(ctx, FLM_EINVAL, "negative N");
    if (c.noise_bits && !noise) return fail(ctx, FLM_EINVAL, "noise_bits > 0 needs the clients' noise seeds");
    if (gauss && !noise) return fail(ctx, FLM_EINVAL, "the table mode needs the clients' noise seeds and the table");
    if (gauss)
        if (int rc = refuse(ctx, flm::rt::dgauss_table_error(gauss->cdt, gauss->tail))) return rc;
    if (N == 0 || L == 0) return 0;
    int64_t K = 0;
    if (int rc = refuse(ctx, flm::rt::client_args_error(x && out, N, seg, seeds, signs, &K))) return rc;
    if (int rc = check_range(ctx, 0, L)) return rc;
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    const size_t Lw = flm::rt::packed_words(L, c.pack);
    if (gauss)
        hc.declare(flm::rt::client_encode_gauss_mask_args(N, K, L, Lw, dither, 2 * (size_t)gauss->tail, clipped),
                   {x, seeds, dither, noise, gauss->cdt, out, clipped});
    else
        hc.declare(flm::rt::client_encode_mask_args(N, K, L, Lw, dither, c.noise_bits, clipped),
                   {x, seeds, dither, noise, out, clipped});
    if (int rc = hc.begin()) return rc;
    const int o = gauss ? 5 : 4;  // out's place in the list: behind the table where there is one
    const GaussNoise d_gauss = {gauss ? gauss->tail : 0, gauss ? hc.dev<uint64_t>(4) : nullptr};
    if (int rc = encode_mask_dev(ctx, hc.dev<float>(0), hc.pitch(0) / 4, N, seg, hc.dev<uint8_t>(1), signs, L, c, unpacked_ok,
                                 hc.dev<uint8_t>(2), hc.dev<uint8_t>(3), gauss ? &d_gauss : nullptr, hc.dev<uint32_t>(o),
                                 hc.pitch(o) / 4, hc.dev<uint32_t>(o + 1), ctx->stream))
        return rc;
    return hc.finish();
}

// The decode's rule.  pack = 1 where admitted is flm_decode_sum, whose rule knows no clip; packed, the codec's rule
// for `count` contributors, and *bias_n gets B_n = B + noise_bits / 2.
int check_decode(flm_ctx *ctx, flm::CodecParams &c, bool unpacked_ok, int64_t count, uint32_t *bias_n) {
    if (unpacked_ok && c.pack == 1) return refuse(ctx, flm::rt::decode_error(c.frac_bits, count));
    return check_codec(ctx, c, unpacked_ok, count, 0, bias_n);
}

// Unpacked, the kernel may run in place.  Packed, the noise only changes the bias: count B_n in count B's place.
int decode_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, flm::CodecParams c, bool unpacked_ok, int64_t count,
               float *d_out, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    uint32_t bias_n = 0;
    if (int rc = check_decode(ctx, c, unpacked_ok, count, &bias_n)) return rc;
    if (L == 0) return 0;
    if (!d_sum || !d_out) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (int rc = refuse(ctx, flm::rt::align16_error({d_sum, d_out}))) return rc;
    FLM_ON_DEVICE(ctx);
    const double denom = (double)count * std::ldexp(1.0, c.frac_bits);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FLM_HIP(ctx, c.pack == 1 ? flm::launch_decode_sum(d_sum, L, denom, d_out, s)
                             : flm::launch_decode_unpack(d_sum, L, c.pack, count * (int64_t)bias_n, denom, d_out, s));
    return 0;
}

int decode_host(flm_ctx *ctx, const uint32_t *sum, size_t L, flm::CodecParams c, bool unpacked_ok, int64_t count, float *out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = check_decode(ctx, c, unpacked_ok, count, nullptr)) return rc;
    if (L == 0) return 0;
    if (!sum || !out) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::decode_unpack_args(L, flm::rt::packed_words(L, c.pack)), {sum, out});
    if (int rc = hc.begin()) return rc;
    if (int rc = decode_dev(ctx, hc.dev<uint32_t>(0), L, c, unpacked_ok, count, hc.dev<float>(1), ctx->stream)) return rc;
    return hc.finish();
}

// The modular decode's rules (flm_call_args.h): the admission, then guard and L; *bias_n gets B_n.
int check_modular(flm_ctx *ctx, const flm::CodecParams &c, int64_t count, uint32_t *bias_n = nullptr) {
    bool range = false;
    const char *why = flm::rt::modular_error(c.frac_bits, c.clip, c.pack, c.noise_bits, count, &range, bias_n);
    return refuse(ctx, why, range ? FLM_ERANGE : FLM_EINVAL);
}
int check_modular_decode(flm_ctx *ctx, const flm::CodecParams &c, int64_t count, int64_t guard, size_t L, uint32_t *bias_n) {
    if (int rc = check_modular(ctx, c, count, bias_n)) return rc;
    bool range = false;
    const char *why = flm::rt::modular_decode_error(c.pack, guard, L, &range);
    return refuse(ctx, why, range ? FLM_ERANGE : FLM_EINVAL);
}

// The packed decode of a sum taken modulo the field: count B_n mod 2^32 in the bias's place, and the two words of
// near-wrap evidence, zeroed on the stream first, where the caller wants them.
int decode_mod_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, flm::CodecParams c, int64_t count, int64_t guard,
                   float *d_out, uint32_t *d_stats, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    uint32_t bias_n = 0;
    if (int rc = check_modular_decode(ctx, c, count, guard, L, &bias_n)) return rc;
    if ((uintptr_t)d_stats & 3) return fail(ctx, FLM_EINVAL, "stats must be 4-byte aligned");
    if (L > 0) {
        if (!d_sum || !d_out) return fail(ctx, FLM_EINVAL, "NULL argument");
        if (int rc = refuse(ctx, flm::rt::align16_error({d_sum, d_out}))) return rc;
        if (int rc = refuse(ctx, flm::rt::modular_alias_error(d_sum, d_out, L, c.pack))) return rc;
    }
    if (L == 0 && !d_stats) return 0;
    FLM_ON_DEVICE(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d_stats) FLM_HIP(ctx, hipMemsetAsync(d_stats, 0, 2 * sizeof(uint32_t), s));
    const double denom = (double)count * std::ldexp(1.0, c.frac_bits);
    const uint32_t cb = (uint32_t)((uint64_t)count * (uint64_t)bias_n);  // count < 2^31, B_n < 2^31: exact, then mod 2^32
    FLM_HIP(ctx, flm::launch_decode_unpack_mod(d_sum, L, c.pack, cb, denom, (uint32_t)guard, d_out, d_stats, s));
    return 0;
}

int decode_mod_host(flm_ctx *ctx, const uint32_t *sum, size_t L, flm::CodecParams c, int64_t count, int64_t guard, float *out,
                    uint32_t *stats) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = check_modular_decode(ctx, c, count, guard, L, nullptr)) return rc;
    if (L == 0) {
        if (stats) stats[0] = stats[1] = 0;
        return 0;
    }
    if (!sum || !out) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::decode_unpack_mod_args(L, flm::rt::packed_words(L, c.pack), stats != nullptr), {sum, out, stats});
    if (int rc = hc.begin()) return rc;
    if (int rc = decode_mod_dev(ctx, hc.dev<uint32_t>(0), L, c, count, guard, hc.dev<float>(1), hc.dev<uint32_t>(2), ctx->stream))
        return rc;
    return hc.finish();
}

}  // namespace

int flm_codec_check(int frac_bits, float clip, int64_t n_clients) {
    flm::CodecParams c{frac_bits, clip, 1, 0, 0};
    return check_codec(nullptr, c, true, n_clients, 0);
}
int flm_codec_check_packed(int frac_bits, float clip, int pack, int64_t n_clients) {
    flm::CodecParams c{frac_bits, clip, pack, 0, 0};
    return check_codec(nullptr, c, false, n_clients, 0);
}
int flm_codec_check_noise(int frac_bits, float clip, int pack, int noise_bits, int64_t n_clients, uint64_t L_params) {
    flm::CodecParams c{frac_bits, clip, pack, noise_bits, 0};
    return check_codec(nullptr, c, true, n_clients, L_params);
}

int flm_client_encode_mask(flm_ctx *ctx, const float *x, int N, const int64_t *seg, const uint8_t *seeds,
                           const int8_t *signs, size_t L, int frac_bits, float clip, const uint8_t *dither,
                           uint32_t *out, uint32_t *clipped) {
    if (ctx && N < 0) return fail(ctx, FLM_EINVAL, "negative N");
    return encode_mask_host(ctx, x, N, seg, seeds, signs, L, {frac_bits, clip, 1, 0, 0}, true, dither, nullptr, nullptr, out, clipped);
}
int flm_client_encode_mask_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, const int64_t *seg,
                               const uint8_t *d_seeds, const int8_t *signs, size_t L, int frac_bits, float clip,
                               const uint8_t *d_dither, uint32_t *d_out, size_t out_pitch, uint32_t *d_clipped,
                               void *stream) {
    return encode_mask_dev(ctx, d_x, x_pitch, N, seg, d_seeds, signs, L, {frac_bits, clip, 1, 0, 0}, true, d_dither, nullptr,
                           nullptr, d_out, out_pitch, d_clipped, stream);
}
int flm_client_encode_pack_mask(flm_ctx *ctx, const float *x, int N, const int64_t *seg, const uint8_t *seeds,
                                const int8_t *signs, size_t L, int frac_bits, float clip, int pack, const uint8_t *dither,
                                uint32_t *out, uint32_t *clipped) {
    if (ctx && N < 0) return fail(ctx, FLM_EINVAL, "negative N");
    return encode_mask_host(ctx, x, N, seg, seeds, signs, L, {frac_bits, clip, pack, 0, 0}, false, dither, nullptr, nullptr, out, clipped);
}
int flm_client_encode_pack_mask_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, const int64_t *seg,
                                    const uint8_t *d_seeds, const int8_t *signs, size_t L, int frac_bits, float clip,
                                    int pack, const uint8_t *d_dither, uint32_t *d_out, size_t out_pitch,
                                    uint32_t *d_clipped, void *stream) {
    return encode_mask_dev(ctx, d_x, x_pitch, N, seg, d_seeds, signs, L, {frac_bits, clip, pack, 0, 0}, false, d_dither, nullptr,
                           nullptr, d_out, out_pitch, d_clipped, stream);
}
int flm_client_encode_noise_mask(flm_ctx *ctx, const float *x, int N, const int64_t *seg, const uint8_t *seeds,
                                 const int8_t *signs, size_t L, int frac_bits, float clip, int pack, const uint8_t *dither,
                                 int noise_bits, const uint8_t *noise, uint32_t *out, uint32_t *clipped) {
    return encode_mask_host(ctx, x, N, seg, seeds, signs, L, {frac_bits, clip, pack, noise_bits, 0}, true, dither, noise, nullptr,
                            out, clipped);
}
int flm_client_encode_noise_mask_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, const int64_t *seg,
                                     const uint8_t *d_seeds, const int8_t *signs, size_t L, int frac_bits, float clip,
                                     int pack, const uint8_t *d_dither, int noise_bits, const uint8_t *d_noise,
                                     uint32_t *d_out, size_t out_pitch, uint32_t *d_clipped, void *stream) {
    return encode_mask_dev(ctx, d_x, x_pitch, N, seg, d_seeds, signs, L, {frac_bits, clip, pack, noise_bits, 0}, true, d_dither,
                           d_noise, nullptr, d_out, out_pitch, d_clipped, stream);
}

int flm_codec_check_gauss(int frac_bits, float clip, int pack, int tail, int64_t n_clients, uint64_t L_params) {
    flm::CodecParams c{frac_bits, clip, pack, 0, 0};
    return check_codec_gauss(nullptr, c, tail, n_clients, L_params);
}
int flm_dgauss_check_table(const uint64_t *cdt, int tail) { return refuse(nullptr, flm::rt::dgauss_table_error(cdt, tail)); }
int flm_client_encode_gauss_mask(flm_ctx *ctx, const float *x, int N, const int64_t *seg, const uint8_t *seeds,
                                 const int8_t *signs, size_t L, int frac_bits, float clip, int pack, const uint8_t *dither,
                                 int tail, const uint64_t *cdt, const uint8_t *noise, uint32_t *out, uint32_t *clipped) {
    const GaussNoise g = {tail, cdt};
    return encode_mask_host(ctx, x, N, seg, seeds, signs, L, {frac_bits, clip, pack, 0, 0}, true, dither, noise, &g, out, clipped);
}
int flm_client_encode_gauss_mask_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, const int64_t *seg,
                                     const uint8_t *d_seeds, const int8_t *signs, size_t L, int frac_bits, float clip,
                                     int pack, const uint8_t *d_dither, int tail, const uint64_t *d_cdt,
                                     const uint8_t *d_noise, uint32_t *d_out, size_t out_pitch, uint32_t *d_clipped,
                                     void *stream) {
    const GaussNoise g = {tail, d_cdt};
    return encode_mask_dev(ctx, d_x, x_pitch, N, seg, d_seeds, signs, L, {frac_bits, clip, pack, 0, 0}, true, d_dither, d_noise,
                           &g, d_out, out_pitch, d_clipped, stream);
}

int flm_decode_sum(flm_ctx *ctx, const uint32_t *sum, size_t L, int frac_bits, int64_t count, float *out) {
    return decode_host(ctx, sum, L, {frac_bits, 0.0f, 1, 0, 0}, true, count, out);
}
int flm_decode_sum_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, int frac_bits, int64_t count, float *d_out,
                       void *stream) {
    return decode_dev(ctx, d_sum, L, {frac_bits, 0.0f, 1, 0, 0}, true, count, d_out, stream);
}
int flm_decode_unpack(flm_ctx *ctx, const uint32_t *sum, size_t L, int frac_bits, float clip, int pack, int64_t count,
                      float *out) {
    return decode_host(ctx, sum, L, {frac_bits, clip, pack, 0, 0}, false, count, out);
}
int flm_decode_unpack_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, int frac_bits, float clip, int pack, int64_t count,
                          float *d_out, void *stream) {
    return decode_dev(ctx, d_sum, L, {frac_bits, clip, pack, 0, 0}, false, count, d_out, stream);
}
// pack = 1 is refused here, as the packed calls refuse it; any other pack by the noise rule
int flm_decode_unpack_noise(flm_ctx *ctx, const uint32_t *sum, size_t L, int frac_bits, float clip, int pack, int noise_bits,
                            int64_t count, float *out) {
    if (ctx && pack == 1) return fail(ctx, FLM_EINVAL, "pack must be 2 or 4");
    return decode_host(ctx, sum, L, {frac_bits, clip, pack, noise_bits, 0}, true, count, out);
}
int flm_decode_unpack_noise_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, int frac_bits, float clip, int pack,
                                int noise_bits, int64_t count, float *d_out, void *stream) {
    if (ctx && pack == 1) return fail(ctx, FLM_EINVAL, "pack must be 2 or 4");
    return decode_dev(ctx, d_sum, L, {frac_bits, clip, pack, noise_bits, 0}, true, count, d_out, stream);
}

int flm_codec_check_modular(int frac_bits, float clip, int pack, int noise_bits, int64_t n_clients) {
    return check_modular(nullptr, {frac_bits, clip, pack, noise_bits, 0}, n_clients);
}
int flm_decode_unpack_mod(flm_ctx *ctx, const uint32_t *sum, size_t L, int frac_bits, float clip, int pack, int noise_bits,
                          int64_t count, int guard, float *out, uint32_t *stats) {
    return decode_mod_host(ctx, sum, L, {frac_bits, clip, pack, noise_bits, 0}, count, guard, out, stats);
}
int flm_decode_unpack_mod_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, int frac_bits, float clip, int pack,
                              int noise_bits, int64_t count, int guard, float *d_out, uint32_t *d_stats, void *stream) {
    return decode_mod_dev(ctx, d_sum, L, {frac_bits, clip, pack, noise_bits, 0}, count, guard, d_out, d_stats, stream);
}

int flm_prg_expand(flm_ctx *ctx, const uint8_t *seeds, int K, size_t L, uint64_t slot0, uint32_t *out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (K < 0) return fail(ctx, FLM_EINVAL, "negative K");
    if (K == 0 || L == 0) return 0;
    if (int rc = refuse(ctx, flm::rt::prg_expand_error(seeds, out, slot0))) return rc;
    if (int rc = check_range(ctx, slot0, L)) return rc;
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::prg_expand_args(K, L), {seeds, out});
    if (int rc = hc.begin()) return rc;
    if (int rc = flm_prg_expand_dev(ctx, hc.dev<uint8_t>(0), K, L, slot0, hc.dev<uint32_t>(1), hc.pitch(1) / 4, ctx->stream))
        return rc;
    return hc.finish();
}

int flm_prg_expand_dev(flm_ctx *ctx, const uint8_t *d_seeds, int K, size_t L, uint64_t slot0, uint32_t *d_out,
                       size_t pitch, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (K <= 0 || L == 0) return 0;
    if (int rc = refuse(ctx, flm::rt::prg_expand_error(d_seeds, d_out, slot0))) return rc;
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(pitch, L))) return rc;
    if (int rc = refuse(ctx, flm::rt::align16_error({d_out}))) return rc;
    if (int rc = check_range(ctx, slot0, L)) return rc;
    if (int rc = refuse(ctx, flm::rt::prg_expand_launch_error(K, L))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
    FLM_ON_DEVICE(ctx);
    // +1 signs through a staging slot, the seed schedule, then prg_expand_kernel
    Staged up;
    if (int rc = stage_put(ctx, {{nullptr, (size_t)K, 1}}, s, &up)) return rc;
    SeedTable *table = nullptr;
    const int groups = std::max(1, ctx->n_cus * ctx->tune_expand_waves);
    int rc = run_seed_schedule(ctx, d_seeds, reinterpret_cast<const int8_t *>(up.dev[0]), K, s, &table);
    if (!rc) {
        hipError_t e = flm::launch_prg_expand(table->recs.as<SeedRec>(), K, L, pitch, (uint32_t)(slot0 / 16), d_out,
                                              groups, s);
        if (e == hipSuccess) e = table_read(table, s);
        if (e != hipSuccess) rc = fail(ctx, FLM_EHIP, "prg_expand launch: %s", hipGetErrorString(e));
        if (rc) table_cover(table, s);
    }
    if ((rc = stage_done(ctx, up, s, rc))) return rc;
    set_last_plan(ctx, (int)std::min<uint64_t>(flm::rt::prg_expand_units(K, L), (uint64_t)groups), flm::kWaveSlots, 0,
                  kExpandVariant);
    return 0;
}

// ---- the randomised block Hadamard rotation and the L2 clip in front of it (flm_call_args.h has the rules)

namespace {
int check_rotate(flm_ctx *ctx, uint64_t L, int log2_block, uint64_t *L_rot) {
    bool range = false;
    const char *why = flm::rt::rotate_error(L, log2_block, &range, L_rot);
    return refuse(ctx, why, range ? FLM_ERANGE : FLM_EINVAL);
}
int check_l2(flm_ctx *ctx, uint64_t L, float clip_norm, int N, uint64_t *work_doubles) {
    bool range = false;
    const char *why = flm::rt::l2_clip_error(L, clip_norm, N, &range, work_doubles);
    return refuse(ctx, why, range ? FLM_ERANGE : FLM_EINVAL);
}

// flm_rotate_dev, and flm_rotate_clip_dev (clip: forward, d_factors required and multiplied into the load).  The
// factors come from elsewhere, so the L2 rule is not consulted.
int rotate_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, int log2_block, const uint32_t *d_sign_bits,
               bool inverse, bool clip, const float *d_factors, float *d_out, size_t out_pitch, uint32_t *d_nonfinite,
               void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    uint64_t L_rot = 0;
    if (int rc = check_rotate(ctx, L, log2_block, &L_rot)) return rc;
    if (N < 0) return fail(ctx, FLM_EINVAL, "negative N");
    if (inverse && d_nonfinite) return fail(ctx, FLM_EINVAL, "the inverse rotation counts nothing: nonfinite must be NULL");
    if (N == 0) return 0;
    if (!d_x || !d_out || !d_sign_bits || (clip && !d_factors)) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(x_pitch, inverse ? L_rot : L))) return rc;
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(out_pitch, inverse ? L : L_rot))) return rc;
    if (int rc = refuse(ctx, flm::rt::align16_error({d_x, d_out, d_sign_bits}))) return rc;
    if (int rc = refuse(ctx, flm::rt::align4_error(d_factors))) return rc;
    if (int rc = refuse(ctx, flm::rt::rotate_launch_error(flm::rotate_groups(N, L_rot)))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
    FLM_ON_DEVICE(ctx);
    if (d_nonfinite) FLM_HIP(ctx, hipMemsetAsync(d_nonfinite, 0, (size_t)N * sizeof(uint32_t), s));
    FLM_HIP(ctx, flm::launch_rotate(d_x, x_pitch, N, L, L_rot, log2_block, d_sign_bits, inverse, d_out, out_pitch, d_nonfinite,
                                    d_factors, s));
    return 0;
}

// the context's tile partials for N rows of L, and behind them N factors for a caller who wants none back
int reserve_l2_work(flm_ctx *ctx, uint64_t work_doubles, int N, double **work, float **spare_factors) {
    FLM_HIP(ctx, ctx->l2_work.reserve(work_doubles * sizeof(double) + (size_t)N * sizeof(float)));
    *work = ctx->l2_work.as<double>();
    *spare_factors = reinterpret_cast<float *>(*work + work_doubles);
    return 0;
}

// flm_rotate, and flm_rotate_clip (clip_norm given: forward, the L2 rule after the rotation's, the factors computed
// in front of the rotation and with sumsq handed back where asked).  The L2 rule wants N >= 1; the plain rotation
// takes N = 0 as nothing to do.
int rotate_host(flm_ctx *ctx, const float *x, int N, size_t L, int log2_block, const uint8_t *key, bool inverse,
                const float *clip_norm, float *out, uint32_t *nonfinite, float *factors, double *sumsq) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    uint64_t L_rot = 0, wd = 0;
    if (int rc = check_rotate(ctx, L, log2_block, &L_rot)) return rc;
    if (clip_norm) {
        if (int rc = check_l2(ctx, L, *clip_norm, N, &wd)) return rc;
    } else {
        if (N < 0) return fail(ctx, FLM_EINVAL, "negative N");
        if (inverse && nonfinite) return fail(ctx, FLM_EINVAL, "the inverse rotation counts nothing: nonfinite must be NULL");
        if (N == 0) return 0;
    }
    if (!x || !out || !key) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    const size_t L_in = inverse ? L_rot : L, L_out = inverse ? L : L_rot, words = flm::rt::rotate_sign_words(L_rot);
    FLM_HIP(ctx, ctx->rot_signs.reserve(round_up(words, 4) * sizeof(uint32_t)));
    double *work = nullptr;
    float *d_factors = nullptr;
    if (clip_norm)
        if (int rc = reserve_l2_work(ctx, wd, N, &work, &d_factors)) return rc;
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::rotate_args(N, L_in, L_out, nonfinite != nullptr, factors != nullptr, sumsq != nullptr),
               {x, out, key, nonfinite, factors, sumsq});
    if (int rc = hc.begin()) return rc;
    if (factors) d_factors = hc.dev<float>(4);
    if (int rc = flm_prg_expand_dev(ctx, hc.dev<uint8_t>(2), 1, words, 0, ctx->rot_signs.as<uint32_t>(), round_up(words, 4),
                                    ctx->stream))
        return rc;
    if (clip_norm)
        if (int rc = flm_l2_factors_dev(ctx, hc.dev<float>(0), hc.pitch(0) / 4, N, L, *clip_norm, work, d_factors,
                                        hc.dev<double>(5), ctx->stream))
            return rc;
    if (int rc = rotate_dev(ctx, hc.dev<float>(0), hc.pitch(0) / 4, N, L, log2_block, ctx->rot_signs.as<uint32_t>(), inverse,
                            clip_norm != nullptr, d_factors, hc.dev<float>(1), hc.pitch(1) / 4, hc.dev<uint32_t>(3), ctx->stream))
        return rc;
    return hc.finish();
}
}  // namespace

int flm_rotate_check(uint64_t L, int log2_block, uint64_t *L_rot) {
    uint64_t lr = 0;
    if (int rc = check_rotate(nullptr, L, log2_block, &lr)) return rc;
    if (L_rot) *L_rot = lr;
    return 0;
}
int flm_rotate_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, int log2_block,
                   const uint32_t *d_sign_bits, int inverse, float *d_out, size_t out_pitch, uint32_t *d_nonfinite,
                   void *stream) {
    return rotate_dev(ctx, d_x, x_pitch, N, L, log2_block, d_sign_bits, inverse != 0, false, nullptr, d_out, out_pitch,
                      d_nonfinite, stream);
}
int flm_rotate_clip_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, int log2_block,
                        const uint32_t *d_sign_bits, const float *d_factors, float *d_out, size_t out_pitch,
                        uint32_t *d_nonfinite, void *stream) {
    return rotate_dev(ctx, d_x, x_pitch, N, L, log2_block, d_sign_bits, false, true, d_factors, d_out, out_pitch, d_nonfinite,
                      stream);
}
int flm_rotate(flm_ctx *ctx, const float *x, int N, size_t L, int log2_block, const uint8_t key[32], int inverse,
               float *out, uint32_t *nonfinite) {
    return rotate_host(ctx, x, N, L, log2_block, key, inverse != 0, nullptr, out, nonfinite, nullptr, nullptr);
}
int flm_rotate_clip(flm_ctx *ctx, const float *x, int N, size_t L, int log2_block, const uint8_t key[32], float clip_norm,
                    float *out, uint32_t *nonfinite, float *factors, double *sumsq) {
    return rotate_host(ctx, x, N, L, log2_block, key, false, &clip_norm, out, nonfinite, factors, sumsq);
}

int flm_l2_clip_check(uint64_t L, float clip_norm, int N, uint64_t *work_doubles) {
    uint64_t wd = 0;
    if (int rc = check_l2(nullptr, L, clip_norm, N, &wd)) return rc;
    if (work_doubles) *work_doubles = wd;
    return 0;
}

int flm_l2_factors_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, float clip_norm, double *d_work,
                       float *d_factors, double *d_sumsq, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    uint64_t wd = 0;
    if (int rc = check_l2(ctx, L, clip_norm, N, &wd)) return rc;
    if (!d_x || !d_work || !d_factors) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(x_pitch, L))) return rc;
    if (int rc = refuse(ctx, flm::rt::align16_error({d_x}))) return rc;
    if (int rc = refuse(ctx, flm::rt::l2_factors_align_error(d_work, d_sumsq, d_factors))) return rc;
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_l2_factors(d_x, x_pitch, N, L, clip_norm, d_work, d_factors, d_sumsq,
                                        static_cast<hipStream_t>(stream)));
    return 0;
}

int flm_scale_rows_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, const float *d_factors,
                       float *d_out, size_t out_pitch, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    uint64_t wd = 0;
    if (int rc = check_l2(ctx, L, 1.0f, N, &wd)) return rc;
    if (!d_x || !d_factors || !d_out) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(x_pitch, L))) return rc;
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(out_pitch, L))) return rc;
    if (int rc = refuse(ctx, flm::rt::align16_error({d_x, d_out}))) return rc;
    if (int rc = refuse(ctx, flm::rt::align4_error(d_factors))) return rc;
    if (d_out == d_x && out_pitch != x_pitch) return fail(ctx, FLM_EINVAL, "in place needs equal pitches");
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_scale_rows(d_x, x_pitch, N, L, d_factors, d_out, out_pitch, static_cast<hipStream_t>(stream)));
    return 0;
}

int flm_l2_clip(flm_ctx *ctx, const float *x, int N, size_t L, float clip_norm, float *out, float *factors, double *sumsq) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    uint64_t wd = 0;
    if (int rc = check_l2(ctx, L, clip_norm, N, &wd)) return rc;
    if (!x || !out) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    double *work = nullptr;
    float *spare = nullptr;
    if (int rc = reserve_l2_work(ctx, wd, N, &work, &spare)) return rc;
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::l2_clip_args(N, L, factors != nullptr, sumsq != nullptr), {x, out, factors, sumsq});
    if (int rc = hc.begin()) return rc;
    float *d_factors = factors ? hc.dev<float>(2) : spare;
    if (int rc = flm_l2_factors_dev(ctx, hc.dev<float>(0), hc.pitch(0) / 4, N, L, clip_norm, work, d_factors, hc.dev<double>(3),
                                    ctx->stream))
        return rc;
    if (int rc = flm_scale_rows_dev(ctx, hc.dev<float>(0), hc.pitch(0) / 4, N, L, d_factors, hc.dev<float>(1), hc.pitch(1) / 4,
                                    ctx->stream))
        return rc;
    return hc.finish();
}

// ---- conditional stochastic rounding in front of the encode (flm_call_args.h has the rules)

namespace {
int check_round(flm_ctx *ctx, uint64_t L, int frac_bits, float clip, int attempts) {
    bool range = false;
    const char *why = flm::rt::round_error(L, frac_bits, clip, attempts, &range);
    return refuse(ctx, why, range ? FLM_ERANGE : FLM_EINVAL);
}
}  // namespace

int flm_round_check(uint64_t L, int frac_bits, float clip, int attempts) {
    return check_round(nullptr, L, frac_bits, clip, attempts);
}

int flm_round_bound(float clip_norm, int frac_bits, uint64_t d, double tail, uint64_t *max_sumsq) {
    bool range = false;
    uint64_t b = 0;
    const char *why = flm::rt::round_bound_error(clip_norm, frac_bits, d, tail, &range, &b);
    if (int rc = refuse(nullptr, why, range ? FLM_ERANGE : FLM_EINVAL)) return rc;
    if (max_sumsq) *max_sumsq = b;
    return 0;
}

int flm_round_select_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, int frac_bits, float clip,
                         const uint8_t *d_candidates, int attempts, uint64_t max_sumsq, uint64_t *d_sumsq,
                         uint8_t *d_dither, uint32_t *d_chosen, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = check_round(ctx, L, frac_bits, clip, attempts)) return rc;
    if (N < 0) return fail(ctx, FLM_EINVAL, "negative N");
    if (N == 0) return 0;
    if (!d_x || !d_candidates || !d_sumsq || !d_dither || !d_chosen) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (int rc = refuse(ctx, flm::rt::row_pitch_error(x_pitch, L))) return rc;
    if (int rc = refuse(ctx, flm::rt::align16_error({d_x}))) return rc;
    if ((uintptr_t)d_sumsq & 7 || (uintptr_t)d_chosen & 3)
        return fail(ctx, FLM_EINVAL, "sumsq must be 8-byte aligned, chosen 4-byte aligned");
    if (int rc = refuse(ctx, flm::rt::round_launch_error(N, L), FLM_ERANGE)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, hipMemsetAsync(d_sumsq, 0, (size_t)N * (size_t)attempts * sizeof(uint64_t), s));  // the kernel adds into it
    FLM_HIP(ctx, flm::launch_round_select(d_x, x_pitch, N, L, frac_bits, clip, d_candidates, attempts, max_sumsq, d_sumsq,
                                          d_dither, d_chosen, s));
    return 0;
}

int flm_round_select(flm_ctx *ctx, const float *x, int N, size_t L, int frac_bits, float clip, const uint8_t *candidates,
                     int attempts, uint64_t max_sumsq, uint64_t *sumsq, uint8_t *dither, uint32_t *chosen) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = check_round(ctx, L, frac_bits, clip, attempts)) return rc;
    if (N < 0) return fail(ctx, FLM_EINVAL, "negative N");
    if (N == 0) return 0;
    if (!x || !candidates || !sumsq || !dither || !chosen) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::round_select_args(N, L, attempts), {x, candidates, sumsq, dither, chosen});
    if (int rc = hc.begin()) return rc;
    if (int rc = flm_round_select_dev(ctx, hc.dev<float>(0), hc.pitch(0) / 4, N, L, frac_bits, clip, hc.dev<uint8_t>(1), attempts,
                                      max_sumsq, hc.dev<uint64_t>(2), hc.dev<uint8_t>(3), hc.dev<uint32_t>(4), ctx->stream))
        return rc;
    return hc.finish();
}

int flm_mask_accumulate(flm_ctx *ctx, const uint8_t *seeds, const int8_t *signs, int K, uint32_t *acc, size_t L,
                        uint64_t slot0) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (K < 0) return fail(ctx, FLM_EINVAL, "negative K");
    if (L == 0) return 0;
    if (!acc) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (K > 0 && (!seeds || !signs)) return fail(ctx, FLM_EINVAL, "NULL seeds/signs");
    if (int rc = refuse(ctx, flm::rt::slot0_error(slot0))) return rc;
    if (int rc = refuse(ctx, flm::rt::signs_error(signs, K))) return rc;
    if (int rc = check_range(ctx, slot0, L)) return rc;
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::mask_accumulate_args(K, L), {acc, acc, seeds, signs});
    if (int rc = hc.begin()) return rc;
    if (int rc = flm_aggregate_unmask_dev(ctx, hc.dev<uint32_t>(0), hc.pitch(0) / 4, 1, hc.dev<uint8_t>(2), hc.dev<int8_t>(3),
                                          K, L, 0, L, slot0, hc.dev<uint32_t>(1), ctx->stream))
        return rc;
    return hc.finish();
}

int flm_chacha20_xor(flm_ctx *ctx, const uint8_t key[32], const uint8_t nonce[8], uint64_t counter, const uint8_t *in,
                     uint8_t *out, size_t n) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!key || !nonce || !in || !out) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    uint32_t k[8], nn[2];
    for (int i = 0; i < 8; ++i)
        k[i] = (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) |
               ((uint32_t)key[4 * i + 3] << 24);
    for (int i = 0; i < 2; ++i)
        nn[i] = (uint32_t)nonce[4 * i] | ((uint32_t)nonce[4 * i + 1] << 8) | ((uint32_t)nonce[4 * i + 2] << 16) |
                ((uint32_t)nonce[4 * i + 3] << 24);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::chacha20_xor_args(n), {in, out});
    if (int rc = hc.begin()) return rc;
    FLM_HIP(ctx, flm::launch_chacha20_xor(k, nn, counter, hc.dev<uint8_t>(0), hc.dev<uint8_t>(1), n, ctx->stream));
    return hc.finish();
}

int flm_plan_aggregate(int subtiles, int pairing, size_t row_pitch, int N, int K, size_t L, size_t mask_lo,
                       size_t mask_hi, uint64_t prg_slot0, void *items_out, int max_items, int *n_items,
                       int *plan_flags) {
    if (N < 0 || K < 0 || mask_hi > L || mask_lo > mask_hi || !n_items)
        return fail(nullptr, FLM_EINVAL, "flm_plan_aggregate: bad arguments");
    if (int rc = check_range(nullptr, prg_slot0, mask_hi)) return rc;
    std::vector<Item> items;
    const PlanShape plan = flm::plan::build_aggregate_items(subtiles, pairing, row_pitch, N, K, L, mask_lo, mask_hi,
                                                            prg_slot0, items);
    *n_items = (int)items.size();
    if (plan_flags)
        *plan_flags = (plan.needs_zero ? 1 : 0) | (plan.atomics ? 2 : 0) | (plan.single_tile ? 4 : 0) |
                      (plan.seed_light ? 8 : 0) | (plan.subtiles << 8);
    if (items_out && max_items > 0)
        std::memcpy(items_out, items.data(), sizeof(Item) * (size_t)std::min<int>(max_items, (int)items.size()));
    return 0;
}

int flm_host_layout(int n, const uint64_t *width, const uint64_t *rows, const int *may_in_place, int *route,
                    uint64_t *pitch, uint64_t *offset, uint64_t *total) {
    if (n < 0 || (n > 0 && (!width || !rows || !may_in_place || !route || !pitch || !offset)) || !total)
        return fail(nullptr, FLM_EINVAL, "flm_host_layout: bad arguments");
    std::vector<flm::rt::HostSpan> s(n);
    for (int i = 0; i < n; ++i) s[i] = {(size_t)width[i], (size_t)rows[i], may_in_place[i] != 0};
    *total = flm::rt::host_layout(s.data(), n);
    for (int i = 0; i < n; ++i) route[i] = s[i].route, pitch[i] = s[i].pitch, offset[i] = s[i].offset;
    return 0;
}

int flm_set_tuning(flm_ctx *ctx, const char *key, int value) {
    if (!ctx || !key) return fail(ctx, FLM_EINVAL, "NULL argument");
    const TuneKey *t = tune_key(key);
    if (!t) return fail(ctx, FLM_EINVAL, "unknown tuning key '%s'", key);
    if (!t->accepts(value)) return fail(ctx, FLM_EINVAL, t->refusal, value);
    ctx->*t->member = value;
    return 0;
}

int flm_get_tuning(const flm_ctx *ctx, const char *key, int *value) {
    flm_ctx *c = const_cast<flm_ctx *>(ctx);  // only its error string is written
    if (!ctx || !key || !value) return fail(c, FLM_EINVAL, "NULL argument");
    const TuneKey *t = tune_key(key);
    if (!t) return fail(c, FLM_EINVAL, "unknown tuning key '%s'", key);
    *value = ctx->*t->member;
    return 0;
}

int flm_check_signs(flm_ctx *ctx, int *bad_count) {
    if (!ctx || !bad_count) return fail(ctx, FLM_EINVAL, "NULL argument");
    *bad_count = 0;
    const SeedTable *t = ctx->last_small ? nullptr : ctx->cur_table;
    const DevBuf *meta = ctx->last_small ? &ctx->small_meta : (t ? &t->meta : nullptr);
    if (!meta || !meta->p) return 0;
    FLM_ON_DEVICE(ctx);
    if (t && t->written_valid) FLM_HIP(ctx, hipEventSynchronize(t->written));
    if (const hipEvent_t read = t ? t->readers.event_of(t->w_stream) : nullptr) FLM_HIP(ctx, hipEventSynchronize(read));
    uint32_t parts = 0;
    FLM_HIP(ctx, hipMemcpy(&parts, meta->p, sizeof parts, hipMemcpyDeviceToHost));
    if (2 + 2 * (size_t)parts > meta->cap / sizeof(uint32_t))
        return fail(ctx, FLM_EHIP, "seed table sign counts: %u parts overrun the table", parts);
    std::vector<uint32_t> m(2 + 2 * (size_t)parts);
    FLM_HIP(ctx, hipMemcpy(m.data(), meta->p, m.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t p = 0; p < parts; ++p) *bad_count += (int)m[3 + 2 * p];
    return 0;
}

int flm_last_plan(const flm_ctx *ctx, int *items, int *tile_slots, int *atomics, int *variant) {
    if (!ctx) return FLM_EINVAL;
    if (items) *items = ctx->last_items;
    if (tile_slots) *tile_slots = ctx->last_tile;
    if (atomics) *atomics = ctx->last_atomics;
    if (variant) *variant = ctx->last_variant;
    return 0;
}

// ------------------------------------------------------------------ P-256
static int ec_dims(flm_ctx *ctx, int T, int D) {
    if (T < 0 || D < 0) return fail(ctx, FLM_EINVAL, "negative batch size (T=%d, D=%d)", T, D);
    if ((size_t)T * (size_t)D > flm::rt::kMaxRows) return fail(ctx, FLM_EINVAL, "batch too large (T*D=%zu)", (size_t)T * D);
    return 0;
}

// The other calls' size rules (flm_call_args.h) as refusals: the _dev form's first check, and the host
// form's before it reads an array or returns for an empty batch.
static int shamir_deal_dims(flm_ctx *ctx, int T, int M, int C) {
    const char *why = flm::rt::shamir_deal_dims_error(T, M, C);
    return why ? fail(ctx, FLM_EINVAL, "shamir deal (T=%d, M=%d, C=%d): %s", T, M, C, why) : 0;
}
static int aes_gcm_xor_dims(flm_ctx *ctx, int nonce_len, size_t len, int n) {
    const char *why = flm::rt::aes_gcm_dims_error(nonce_len, len, n);
    return why ? fail(ctx, FLM_EINVAL, "aes gcm xor (nonce_len=%d, len=%zu, n=%d): %s", nonce_len, len, n, why) : 0;
}
static int aes_gcm_auth_dims(flm_ctx *ctx, const char *what, int nonce_len, size_t aad_len, size_t len, int n) {
    const char *why = flm::rt::aes_gcm_auth_dims_error(nonce_len, aad_len, len, n);
    return why ? fail(ctx, FLM_EINVAL, "%s (nonce_len=%d, aad_len=%zu, len=%zu, n=%d): %s", what, nonce_len, aad_len, len, n, why)
               : 0;
}
static int ecdsa_verify_dims(flm_ctx *ctx, int n) {
    const char *why = flm::rt::ecdsa_verify_dims_error(n);
    return why ? fail(ctx, FLM_EINVAL, "ecdsa verify (n=%d): %s", n, why) : 0;
}
static int feldman_verify_dims(flm_ctx *ctx, int T, int M, int x_bits, int n) {
    const char *why = flm::rt::feldman_verify_dims_error(T, M, x_bits, n);
    return why ? fail(ctx, FLM_EINVAL, "feldman verify (T=%d, M=%d, x_bits=%d, n=%d): %s", T, M, x_bits, n, why) : 0;
}

// Cooperative scalar multiplication when the whole batch fits one pass of the device -- the
// latency-bound case: the row-field kernel (four waves per 4 products, ec_mul_row_kernel) up to
// 20 products per CU, e.g. one G = 8 rank's pair chunk (ceil(962/8) x 20 = 2,420: 0.77 against
// 1.20 ms per-lane-field cooperative, tools/probes/ec_kernel_sweep.py, profiles/r04_ec_kernel_sweep.log;
// still 13 % ahead at 4,800, 39 % behind at 9,620), then the per-lane-field cooperative kernel (four
// waves per 64 products, 78 KiB of LDS: two workgroups per CU) up to 128 per CU, e.g. the whole c5
// seed recovery (19,240 products); bigger batches, and launches the caller confines to a few CUs
// (ServerReconstruction's CU-split stream sets 0), keep one lane per product.
int ec_coop(flm_ctx *ctx, size_t n) {
    if (ctx->tune_ec_coop >= 0) return ctx->tune_ec_coop;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess) return 0;
    if (n <= (size_t)cus * 20) return 2;
    return n <= (size_t)cus * 2 * 64 ? 1 : 0;
}

int flm_ec_combine_dev(flm_ctx *ctx, const uint8_t *d_c1, const uint8_t *d_shares, const uint8_t *d_lambdas, int T,
                       int D, int negate, uint8_t *d_points_out, uint8_t *d_seeds_out, uint32_t *d_flags,
                       void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ec_dims(ctx, T, D)) return rc;
    if (D == 0) return 0;
    if ((T > 0 && (!d_shares || !d_lambdas)) || !d_flags) return fail(ctx, FLM_EINVAL, "NULL argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, ctx->ec_jac.reserve((size_t)std::max(T, 1) * D * 96));
    FLM_HIP(ctx, hipMemsetAsync(d_flags, 0, (size_t)D * 4, s));
    const int coop = ec_coop(ctx, (size_t)T * D);
    const int terms = coop ? 1 : ctx->tune_ec_terms;
    FLM_HIP(ctx, flm::launch_ec_mul(d_shares, d_lambdas, 0, T, D, ctx->ec_jac.as<uint32_t>(), d_flags, s,
                                    ctx->tune_ec_threads, ctx->tune_ec_waves, coop, terms,
                                    1024u * (unsigned)ctx->tune_ec_spread));
    FLM_HIP(ctx, flm::launch_ec_finish(d_c1, ctx->ec_jac.as<uint32_t>(), flm::ec_mul_groups(T, terms), D, negate,
                                       d_points_out, d_seeds_out,
                                       d_flags, s));
    return 0;
}

int flm_ec_combine(flm_ctx *ctx, const uint8_t *c1, const uint8_t *shares, const uint8_t *lambdas, int T, int D,
                   int negate, uint8_t *points_out, uint8_t *seeds_out, uint32_t *flags_out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ec_dims(ctx, T, D)) return rc;
    if (D == 0) return 0;
    if (T > 0 && (!shares || !lambdas)) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> fl(D);
    HostCopies hc(ctx, s);
    hc.declare(flm::rt::ec_combine_args(T, D, c1, points_out, seeds_out), {shares, lambdas, c1, fl.data(), points_out, seeds_out});
    // the kernel writes points and digests whether or not the caller takes them back
    if (!points_out) FLM_HIP(ctx, ctx->ec_out.reserve((size_t)D * 64));
    if (!seeds_out) FLM_HIP(ctx, ctx->ec_dig.reserve((size_t)D * 32));
    if (int rc = hc.begin()) return rc;
    if (int rc = flm_ec_combine_dev(ctx, hc.dev<uint8_t>(2), hc.dev<uint8_t>(0), hc.dev<uint8_t>(1), T, D, negate,
                                    ctx->ec_out.as<uint8_t>(), ctx->ec_dig.as<uint8_t>(), hc.dev<uint32_t>(3), s))
        return rc;
    if (int rc = hc.finish()) return rc;
    if (flags_out) std::copy(fl.begin(), fl.end(), flags_out);
    for (int i = 0; i < D; ++i)
        if (fl[i] & 3u)
            return fail(ctx, FLM_EINVAL, "element %d: %s is not a point on P-256", i,
                        (fl[i] & 1u) ? "ciphertext c1" : "a decryption share");
    return 0;
}

int flm_shamir_combine_dev(flm_ctx *ctx, const uint8_t *d_shares, const uint8_t *d_lambdas, int T, int M,
                           uint8_t *d_seeds_out, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ec_dims(ctx, T, M)) return rc;
    if (M == 0) return 0;
    if (!d_seeds_out || (T > 0 && (!d_shares || !d_lambdas))) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FLM_HIP(ctx, flm::launch_shamir_combine(d_shares, d_lambdas, T, M, d_seeds_out, s));
    return 0;
}

int flm_pair_units_dev(flm_ctx *ctx, const uint8_t *d_seeds, const int8_t *d_signs, int K, const uint32_t *d_p0,
                       const uint32_t *d_p1, uint32_t *d_dst, size_t L, uint32_t *d_ws, int final_pass, int groups,
                       void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (K < 0) return fail(ctx, FLM_EINVAL, "negative K");
    if (groups <= 0) return fail(ctx, FLM_EINVAL, "groups must be positive");
    if (!d_dst || !d_ws || (K > 0 && (!d_seeds || !d_signs))) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (final_pass && (!d_p0 || !d_p1)) return fail(ctx, FLM_EINVAL, "the final pass needs both partial rows");
    if (final_pass && (((uintptr_t)d_p0 | (uintptr_t)d_p1 | (uintptr_t)d_dst) & 15))
        return fail(ctx, FLM_EINVAL, "partial rows and dst must be 16-byte aligned");
    if (L > ((uint64_t)1 << 36)) return fail(ctx, FLM_EINVAL, "L=%zu beyond the 2^32-block ChaCha counter", L);
    if (flm::pair_units_count(K, L, nullptr) == 0xFFFFFFFFu) return fail(ctx, FLM_EINVAL, "too many units");
    FLM_ON_DEVICE(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (final_pass) FLM_HIP(ctx, flm::launch_add2(d_p0, d_p1, d_dst, L, s));
    if (L == 0 || K == 0) return 0;
    SeedTable *table = nullptr;
    if (int rc = run_seed_schedule(ctx, d_seeds, d_signs, K, s, &table)) return rc;
    hipError_t e = flm::launch_pair_units(!final_pass, table->recs.as<flm::SeedRec>(), K, d_dst, L, d_ws, groups, s);
    if (e == hipSuccess) e = table_read(table, s);
    if (e != hipSuccess) {
        table_cover(table, s);
        return fail(ctx, FLM_EHIP, "pair units launch: %s", hipGetErrorString(e));
    }
    return 0;
}

int flm_flag_set_dev(flm_ctx *ctx, uint32_t *d_ws, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (!d_ws) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_flag_set(d_ws, static_cast<hipStream_t>(stream)));
    return 0;
}

int flm_shamir_combine(flm_ctx *ctx, const uint8_t *shares, const uint8_t *lambdas, int T, int M,
                       uint8_t *seeds_out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ec_dims(ctx, T, M)) return rc;
    if (M == 0) return 0;
    if (!seeds_out || (T > 0 && (!shares || !lambdas))) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::shamir_combine_args(T, M), {shares, lambdas, seeds_out});
    if (int rc = hc.begin()) return rc;
    // launched here, not through flm_shamir_combine_dev: through it this call measured over its bound
    FLM_HIP(ctx, flm::launch_shamir_combine(hc.dev<uint8_t>(0), hc.dev<uint8_t>(1), T, M, hc.dev<uint8_t>(2), ctx->stream));
    return hc.finish();
}

int flm_shamir_deal_dev(flm_ctx *ctx, const uint8_t *d_coeffs, int T, int M, const uint32_t *d_xs, int C,
                        uint8_t *d_shares_out, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = shamir_deal_dims(ctx, T, M, C)) return rc;
    if (M == 0) return 0;
    if (!d_coeffs || !d_xs || !d_shares_out) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (((uintptr_t)d_coeffs | (uintptr_t)d_shares_out) & 15)
        return fail(ctx, FLM_EINVAL, "coeffs and shares_out must be 16-byte aligned");
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_shamir_deal(d_coeffs, T, M, d_xs, C, d_shares_out, static_cast<hipStream_t>(stream)));
    return 0;
}

int flm_shamir_deal(flm_ctx *ctx, const uint8_t *coeffs, int T, int M, const uint32_t *xs, int C,
                    uint8_t *shares_out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = shamir_deal_dims(ctx, T, M, C)) return rc;
    if (!xs) return fail(ctx, FLM_EINVAL, "NULL argument");
    const int zero = flm::rt::shamir_deal_zero_x(xs, C);
    if (zero >= 0) return fail(ctx, FLM_EINVAL, "xs[%d] is 0: a share at x = 0 would be the secret itself", zero);
    if (M == 0) return 0;
    if (!coeffs || !shares_out) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::shamir_deal_args(T, M, C), {coeffs, xs, shares_out});
    if (int rc = hc.begin()) return rc;
    if (int rc = flm_shamir_deal_dev(ctx, hc.dev<uint8_t>(0), T, M, hc.dev<uint32_t>(1), C, hc.dev<uint8_t>(2), ctx->stream))
        return rc;
    return hc.finish();
}

int flm_aes_gcm_xor_dev(flm_ctx *ctx, const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len,
                        const uint8_t *d_in, uint8_t *d_out, size_t len, int n, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = aes_gcm_xor_dims(ctx, nonce_len, len, n)) return rc;
    if (n == 0) return 0;
    if (!d_keys || !d_nonces || !d_in || !d_out) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_aes_gcm_xor(d_keys, d_nonces, nonce_len, d_in, d_out, (uint32_t)len, n,
                                         static_cast<hipStream_t>(stream)));
    return 0;
}

int flm_aes_gcm_xor(flm_ctx *ctx, const uint8_t *keys, const uint8_t *nonces, int nonce_len, const uint8_t *in,
                    uint8_t *out, size_t len, int n) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = aes_gcm_xor_dims(ctx, nonce_len, len, n)) return rc;
    if (n == 0) return 0;
    if (!keys || !nonces || !in || !out) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    // in and out are read and written in place in the bounce buffer when they fit (flm_chacha20_xor)
    hc.declare(flm::rt::aes_gcm_xor_args(nonce_len, len, n), {keys, nonces, in, out});
    if (int rc = hc.begin()) return rc;
    if (int rc = flm_aes_gcm_xor_dev(ctx, hc.dev<uint8_t>(0), hc.dev<uint8_t>(1), nonce_len, hc.dev<uint8_t>(2),
                                     hc.dev<uint8_t>(3), len, n, ctx->stream))
        return rc;
    return hc.finish();
}

int flm_aes_gcm_seal_dev(flm_ctx *ctx, const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len,
                         const uint8_t *d_aad, size_t aad_len, const uint8_t *d_in, uint8_t *d_out, size_t len,
                         uint8_t *d_tags_out, int n, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = aes_gcm_auth_dims(ctx, "aes gcm seal", nonce_len, aad_len, len, n)) return rc;
    if (n == 0) return 0;
    if (const char *why = flm::rt::aes_gcm_auth_null_error(d_keys, d_nonces, d_aad, aad_len, d_in, d_out, len, d_tags_out, nullptr, false))
        return fail(ctx, FLM_EINVAL, "aes gcm seal: %s", why);
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_aes_gcm_seal(d_keys, d_nonces, nonce_len, d_aad, (uint32_t)aad_len, d_in, d_out,
                                          (uint32_t)len, d_tags_out, n, static_cast<hipStream_t>(stream)));
    return 0;
}

int flm_aes_gcm_open_dev(flm_ctx *ctx, const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len,
                         const uint8_t *d_aad, size_t aad_len, const uint8_t *d_in, const uint8_t *d_tags,
                         uint8_t *d_out, size_t len, uint8_t *d_ok_out, int n, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = aes_gcm_auth_dims(ctx, "aes gcm open", nonce_len, aad_len, len, n)) return rc;
    if (n == 0) return 0;
    if (const char *why = flm::rt::aes_gcm_auth_null_error(d_keys, d_nonces, d_aad, aad_len, d_in, d_out, len, d_tags, d_ok_out, true))
        return fail(ctx, FLM_EINVAL, "aes gcm open: %s", why);
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_aes_gcm_open(d_keys, d_nonces, nonce_len, d_aad, (uint32_t)aad_len, d_in, d_tags, d_out,
                                          (uint32_t)len, d_ok_out, n, static_cast<hipStream_t>(stream)));
    return 0;
}

namespace {
// the host-pointer seal (ok_out NULL: tags written) and open (tags read, ok_out written): one body
int aes_gcm_auth_host(flm_ctx *ctx, const char *what, const uint8_t *keys, const uint8_t *nonces, int nonce_len,
                      const uint8_t *aad, size_t aad_len, const uint8_t *in, uint8_t *out, size_t len, uint8_t *tags,
                      uint8_t *ok_out, bool open, int n) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = aes_gcm_auth_dims(ctx, what, nonce_len, aad_len, len, n)) return rc;
    if (n == 0) return 0;
    if (const char *why = flm::rt::aes_gcm_auth_null_error(keys, nonces, aad, aad_len, in, out, len, tags, ok_out, open))
        return fail(ctx, FLM_EINVAL, "%s: %s", what, why);
    FLM_ON_DEVICE(ctx);
    hipStream_t s = ctx->stream;
    HostCopies hc(ctx, s);
    hc.declare(flm::rt::aes_gcm_auth_args(nonce_len, aad_len, len, n, open), {keys, nonces, aad, in, out, tags, ok_out});
    if (int rc = hc.begin()) return rc;
    const uint8_t *d_keys = hc.dev<uint8_t>(0), *d_nonces = hc.dev<uint8_t>(1), *d_aad = hc.dev<uint8_t>(2);
    const uint8_t *d_in = hc.dev<uint8_t>(3);
    uint8_t *d_out = hc.dev<uint8_t>(4), *d_tags = hc.dev<uint8_t>(5);
    if (int rc = open ? flm_aes_gcm_open_dev(ctx, d_keys, d_nonces, nonce_len, d_aad, aad_len, d_in, d_tags, d_out, len,
                                             hc.dev<uint8_t>(6), n, s)
                      : flm_aes_gcm_seal_dev(ctx, d_keys, d_nonces, nonce_len, d_aad, aad_len, d_in, d_out, len, d_tags, n, s))
        return rc;
    return hc.finish();
}
}  // namespace

int flm_aes_gcm_seal(flm_ctx *ctx, const uint8_t *keys, const uint8_t *nonces, int nonce_len, const uint8_t *aad,
                     size_t aad_len, const uint8_t *in, uint8_t *out, size_t len, uint8_t *tags_out, int n) {
    return aes_gcm_auth_host(ctx, "aes gcm seal", keys, nonces, nonce_len, aad, aad_len, in, out, len, tags_out, nullptr,
                             false, n);
}

int flm_aes_gcm_open(flm_ctx *ctx, const uint8_t *keys, const uint8_t *nonces, int nonce_len, const uint8_t *aad,
                     size_t aad_len, const uint8_t *in, const uint8_t *tags, uint8_t *out, size_t len,
                     uint8_t *ok_out, int n) {
    return aes_gcm_auth_host(ctx, "aes gcm open", keys, nonces, nonce_len, aad, aad_len, in, out, len,
                             const_cast<uint8_t *>(tags), ok_out, true, n);
}

int flm_ecdsa_verify_dev(flm_ctx *ctx, const uint8_t *d_pubkeys, const uint8_t *d_digests, const uint8_t *d_sigs,
                         int n, uint8_t *d_ok_out, uint32_t *d_flags, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ecdsa_verify_dims(ctx, n)) return rc;
    if (n == 0) return 0;
    if (!d_pubkeys || !d_digests || !d_sigs || !d_ok_out) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (!flm::rt::ecdsa_verify_aligned((uintptr_t)d_pubkeys, (uintptr_t)d_digests, (uintptr_t)d_sigs))
        return fail(ctx, FLM_EINVAL, "pubkeys, digests and sigs must be 16-byte aligned");
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_ecdsa_verify(d_pubkeys, d_digests, d_sigs, n, d_ok_out, d_flags,
                                          static_cast<hipStream_t>(stream)));
    return 0;
}

int flm_ecdsa_verify(flm_ctx *ctx, const uint8_t *pubkeys, const uint8_t *digests, const uint8_t *sigs, int n,
                     uint8_t *ok_out, uint32_t *flags_out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ecdsa_verify_dims(ctx, n)) return rc;
    if (n == 0) return 0;
    if (!pubkeys || !digests || !sigs || !ok_out) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::ecdsa_verify_args(n, flags_out), {pubkeys, digests, sigs, ok_out, flags_out});
    if (int rc = hc.begin()) return rc;
    if (int rc = flm_ecdsa_verify_dev(ctx, hc.dev<uint8_t>(0), hc.dev<uint8_t>(1), hc.dev<uint8_t>(2), n, hc.dev<uint8_t>(3),
                                      hc.dev<uint32_t>(4), ctx->stream))
        return rc;
    return hc.finish();
}

int flm_feldman_verify_dev(flm_ctx *ctx, const uint8_t *d_commitments, int T, int M, const uint32_t *d_dealer,
                           const uint32_t *d_xs, int x_bits, const uint8_t *d_shares, int n, uint8_t *d_ok_out,
                           uint8_t *d_points_out, uint32_t *d_flags, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = feldman_verify_dims(ctx, T, M, x_bits, n)) return rc;
    if (n == 0) return 0;
    if (!d_commitments || !d_xs || !d_shares || !d_ok_out) return fail(ctx, FLM_EINVAL, "NULL argument");
    if (!flm::rt::feldman_verify_aligned((uintptr_t)d_commitments, (uintptr_t)d_shares, (uintptr_t)d_points_out))
        return fail(ctx, FLM_EINVAL, "commitments, shares and points_out must be 16-byte aligned");
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_feldman_verify(d_commitments, T, M, d_dealer, d_xs, x_bits, d_shares, n, d_ok_out,
                                            d_points_out, d_flags, static_cast<hipStream_t>(stream)));
    return 0;
}

int flm_feldman_verify(flm_ctx *ctx, const uint8_t *commitments, int T, int M, const uint32_t *dealer,
                       const uint32_t *xs, int x_bits, const uint8_t *shares, int n, uint8_t *ok_out,
                       uint8_t *points_out, uint32_t *flags_out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = feldman_verify_dims(ctx, T, M, x_bits, n)) return rc;
    if (n == 0) return 0;
    if (!commitments || !xs || !shares || !ok_out) return fail(ctx, FLM_EINVAL, "NULL argument");
    const int bad = flm::rt::feldman_bad_dealer(dealer, n, M);
    if (bad >= 0) return fail(ctx, FLM_EINVAL, "dealer[%d] = %u, but there are %d dealers", bad, dealer[bad], M);
    FLM_ON_DEVICE(ctx);
    HostCopies hc(ctx, ctx->stream);
    hc.declare(flm::rt::feldman_verify_args(T, M, n, dealer, points_out, flags_out),
               {commitments, dealer, xs, shares, ok_out, points_out, flags_out});
    if (int rc = hc.begin()) return rc;
    if (int rc = flm_feldman_verify_dev(ctx, hc.dev<uint8_t>(0), T, M, hc.dev<uint32_t>(1), hc.dev<uint32_t>(2), x_bits,
                                        hc.dev<uint8_t>(3), n, hc.dev<uint8_t>(4), hc.dev<uint8_t>(5), hc.dev<uint32_t>(6),
                                        ctx->stream))
        return rc;
    return hc.finish();
}

int flm_ec_mul(flm_ctx *ctx, const uint8_t *points, const uint8_t *scalars, int n, uint8_t *out, uint32_t *flags_out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ec_dims(ctx, 1, n)) return rc;
    if (n == 0) return 0;
    if (!points || !scalars || !out) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, ctx->ec_jac.reserve((size_t)n * 96));
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> fl(n);
    HostCopies hc(ctx, s);
    hc.declare(flm::rt::ec_mul_args(n), {points, scalars, fl.data(), out});
    if (int rc = hc.begin()) return rc;
    uint32_t *d_flags = hc.dev<uint32_t>(2);
    FLM_HIP(ctx, hipMemsetAsync(d_flags, 0, (size_t)n * 4, s));
    FLM_HIP(ctx, flm::launch_ec_mul(hc.dev<uint8_t>(0), hc.dev<uint8_t>(1), 1, 1, n, ctx->ec_jac.as<uint32_t>(), d_flags, s,
                                    ctx->tune_ec_threads, ctx->tune_ec_waves, ec_coop(ctx, (size_t)n)));
    FLM_HIP(ctx, flm::launch_ec_finish(nullptr, ctx->ec_jac.as<uint32_t>(), 1, n, 0, hc.dev<uint8_t>(3), nullptr, d_flags, s));
    if (int rc = hc.finish()) return rc;
    if (flags_out) std::copy(fl.begin(), fl.end(), flags_out);
    for (int i = 0; i < n; ++i)
        if (fl[i] & 2u) return fail(ctx, FLM_EINVAL, "element %d: input is not a point on P-256", i);
    return 0;
}

// one body for the three host forms: uniform (n x 96 bytes, flm_h2c_from_uniform), else msgs + lens, else decimals
static int h2c_run(flm_ctx *ctx, const uint8_t *uniform, const uint8_t *msgs, const uint32_t *lens, uint32_t v0, int n,
                   uint8_t *out, uint32_t *flags_out) {
    FLM_ON_DEVICE(ctx);
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> fl(n);
    HostCopies hc(ctx, s);
    hc.declare(flm::rt::h2c_args(n, uniform, msgs), {uniform ? uniform : msgs, lens, fl.data(), out});
    if (int rc = hc.begin()) return rc;
    if (uniform)
        FLM_HIP(ctx, flm::launch_h2c_from_uniform(hc.dev<uint8_t>(0), n, hc.dev<uint8_t>(3), hc.dev<uint32_t>(2), s));
    else
        FLM_HIP(ctx, flm::launch_hash_to_curve(hc.dev<uint8_t>(0), hc.dev<uint32_t>(1), v0, n, hc.dev<uint8_t>(3),
                                               hc.dev<uint32_t>(2), s));
    if (int rc = hc.finish()) return rc;
    if (flags_out) std::copy(fl.begin(), fl.end(), flags_out);
    for (int i = 0; i < n; ++i)
        if (fl[i] & 8u) return fail(ctx, FLM_EINVAL, "message %d: map_to_curve found no square root", i);
    return 0;
}

int flm_hash_to_curve(flm_ctx *ctx, const uint8_t *msgs, const uint32_t *lens, int n, uint8_t *out,
                      uint32_t *flags_out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ec_dims(ctx, 1, n)) return rc;
    if (n == 0) return 0;
    if (!msgs || !lens || !out) return fail(ctx, FLM_EINVAL, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (lens[i] > 64) return fail(ctx, FLM_EINVAL, "message %d is %u bytes (at most 64)", i, lens[i]);
    return h2c_run(ctx, nullptr, msgs, lens, 0, n, out, flags_out);
}

int flm_hash_to_curve_decimal(flm_ctx *ctx, uint32_t v0, int n, uint8_t *out, uint32_t *flags_out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ec_dims(ctx, 1, n)) return rc;
    if (n == 0) return 0;
    if (!out) return fail(ctx, FLM_EINVAL, "NULL argument");
    if ((uint64_t)v0 + (uint64_t)n > (1ull << 32)) return fail(ctx, FLM_EINVAL, "v0 + n exceeds 2^32");
    return h2c_run(ctx, nullptr, nullptr, nullptr, v0, n, out, flags_out);
}

int flm_hash_to_curve_decimal_dev(flm_ctx *ctx, uint32_t v0, int n, uint8_t *d_out, uint32_t *d_flags, void *stream) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ec_dims(ctx, 1, n)) return rc;
    if (n == 0) return 0;
    if (!d_out || !d_flags) return fail(ctx, FLM_EINVAL, "NULL argument");
    if ((uint64_t)v0 + (uint64_t)n > (1ull << 32)) return fail(ctx, FLM_EINVAL, "v0 + n exceeds 2^32");
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, flm::launch_hash_to_curve(nullptr, nullptr, v0, n, d_out, d_flags, static_cast<hipStream_t>(stream)));
    return 0;
}

int flm_h2c_from_uniform(flm_ctx *ctx, const uint8_t *uniform, int n, uint8_t *out, uint32_t *flags_out) {
    if (!ctx) return fail(nullptr, FLM_EINVAL, "ctx is NULL");
    if (int rc = ec_dims(ctx, 1, n)) return rc;
    if (n == 0) return 0;
    if (!uniform || !out) return fail(ctx, FLM_EINVAL, "NULL argument");
    return h2c_run(ctx, uniform, nullptr, nullptr, 0, n, out, flags_out);
}

void *flm_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void flm_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int flm_cu_count(flm_ctx *ctx, int *n_cus) {
    if (!ctx || !n_cus) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_HIP(ctx, hipDeviceGetAttribute(n_cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    return 0;
}

int flm_stream_create_cu_mask(flm_ctx *ctx, const uint32_t *mask, int n_words, void **stream_out) {
    if (!ctx || !mask || !stream_out || n_words <= 0) return fail(ctx, FLM_EINVAL, "NULL argument or empty mask");
    int n_cus = 0;
    FLM_HIP(ctx, hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    int set = 0;
    for (int w = 0; w < n_words; ++w)
        for (int b = 0; b < 32; ++b)
            if ((mask[w] >> b) & 1u) {
                if (w * 32 + b >= n_cus)
                    return fail(ctx, FLM_EINVAL, "CU mask names CU %d of %d", w * 32 + b, n_cus);
                ++set;
            }
    if (set == 0) return fail(ctx, FLM_EINVAL, "CU mask selects no CU");
    FLM_ON_DEVICE(ctx);
    hipStream_t s = nullptr;
    FLM_HIP(ctx, hipExtStreamCreateWithCUMask(&s, (uint32_t)n_words, mask));
    *stream_out = s;
    return 0;
}

int flm_stream_destroy(flm_ctx *ctx, void *stream) {
    if (!ctx || !stream) return fail(ctx, FLM_EINVAL, "NULL argument");
    FLM_ON_DEVICE(ctx);
    FLM_HIP(ctx, hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"
