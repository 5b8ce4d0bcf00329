// flm_fieldtest.hip -- test-only harness: the 256-bit field layers one operation at a time (gfx950).
//
// Includes the product's flm_fe256.h, flm_jac256.h and flm_fe_row.h unchanged and wraps each device
// function in a kernel of its own, so tests/test_fe_ops_gpu.py can feed a single fe_mul, sc_mul or
// row::mul the operands of tests/fe_cases.py and compare the words with Python integers.
// flamingo_amd.build compiles this into flamingo_amd/lib/libflm_fieldtest.so, beside
// libflamingo_hip.so and never linked into it.  The device functions are inlined here afresh, so this
// tests the source of the layers, not the product's code objects.
//
// One entry, host pointers (it allocates, copies and frees itself):
//   int flm_fieldtest_run(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, int n, int device)
// returns 0 or the HIP error; one launch of 64-thread workgroups, synchronised before it returns.
//   lane ops (0..13): one element per thread; a, b: n x 8 little-endian words (b ignored, may be
//     NULL, for one-operand ops); out: n x 8 words, a predicate is 0 or 1 in word 0, the rest 0.
//   wnaf5 (14): a: n x 8 words holding the 32 big-endian bytes of each scalar; out: n x 65 words
//     holding kNafLen = 258 int8 digits and two zero bytes.
//   row ops (20..26): one 16-lane row per element, four elements per wave: element i is row i % 4 of
//     wave i / 4; word r of the element goes to lane r, lanes 8..15 get 0; out: n x 16 words, every
//     lane's result (row::is_zero: 0 or 1 in each of the 16).  n is padded with zero rows to whole
//     waves, since every lane must be active in the carry loops' wave-wide votes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../flamingo_amd/csrc/flm_fe256.h"
#include "../../flamingo_amd/csrc/flm_jac256.h"
#include "../../flamingo_amd/csrc/flm_fe_row.h"

namespace flm {
namespace {

enum Op : int {
    kFeMul = 0, kFeSqr, kFeAdd, kFeSub, kFeNeg, kToMont, kFromMont, kFeIsZero, kFeEq, kFeLtP,
    kScMul, kScAdd, kScBelowN, kScLtN, kWnaf5,
    kRowMul = 20, kRowSqr, kRowAdd, kRowSub, kRowNeg, kRowCanon, kRowIsZero
};
constexpr int kThreads = 64;
constexpr int kNafWords = (kNafLen + 3) / 4;  // 65

__device__ __forceinline__ Fe flag(bool f) {
    Fe r = {};
    r.v[0] = f ? 1u : 0u;
    return r;
}

template <int OP>
__global__ __launch_bounds__(kThreads) void lane_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                        uint32_t *__restrict__ out, int n) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    Fe x, y, r;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        x.v[k] = a[(size_t)i * 8 + k];
        y.v[k] = b[(size_t)i * 8 + k];
    }
    if constexpr (OP == kFeMul) r = fe_mul(x, y);
    else if constexpr (OP == kFeSqr) r = fe_sqr(x);
    else if constexpr (OP == kFeAdd) r = fe_add(x, y);
    else if constexpr (OP == kFeSub) r = fe_sub(x, y);
    else if constexpr (OP == kFeNeg) r = fe_neg(x);
    else if constexpr (OP == kToMont) r = to_mont(x);
    else if constexpr (OP == kFromMont) r = from_mont(x);
    else if constexpr (OP == kFeIsZero) r = flag(fe_is_zero(x));
    else if constexpr (OP == kFeEq) r = flag(fe_eq(x, y));
    else if constexpr (OP == kFeLtP) r = flag(fe_lt_p(x));
    else if constexpr (OP == kScMul) r = sc_mul(x, y);
    else if constexpr (OP == kScAdd) r = sc_add(x, y);
    else if constexpr (OP == kScBelowN) r = sc_below_n(x);
    else r = flag(sc_lt_n(x));
#pragma unroll
    for (int k = 0; k < 8; ++k) out[(size_t)i * 8 + k] = r.v[k];
}

__global__ __launch_bounds__(kThreads) void wnaf5_kernel(const uint32_t *__restrict__ a, uint32_t *__restrict__ out,
                                                         int n) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    int8_t d[kNafLen];
    wnaf5(reinterpret_cast<const uint8_t *>(a) + (size_t)i * 32, d);
    uint8_t *o = reinterpret_cast<uint8_t *>(out) + (size_t)i * kNafWords * 4;
    for (int k = 0; k < kNafWords * 4; ++k) o[k] = k < kNafLen ? (uint8_t)d[k] : (uint8_t)0;
}

// rows: the padded element count, a multiple of 4; a, b and out hold that many rows, so no lane
// returns early and none reads or writes past its buffers
template <int OP>
__global__ __launch_bounds__(kThreads) void row_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                       uint32_t *__restrict__ out) {
    const row::Ctx K = row::make_ctx();
    const int lane = (int)(threadIdx.x & 63), r = lane & 15;
    const size_t e = (size_t)blockIdx.x * 4 + (size_t)(lane >> 4);
    const uint32_t x = r < 8 ? a[e * 8 + r] : 0u, y = r < 8 ? b[e * 8 + r] : 0u;
    uint32_t w;
    if constexpr (OP == kRowMul) w = row::mul(x, y, K);
    else if constexpr (OP == kRowSqr) w = row::sqr(x, K);
    else if constexpr (OP == kRowAdd) w = row::add(x, y, K);
    else if constexpr (OP == kRowSub) w = row::sub(x, y, K);
    else if constexpr (OP == kRowNeg) w = row::neg(x, K);
    else if constexpr (OP == kRowCanon) w = row::canon(x, K);
    else w = row::is_zero(x, K) ? 1u : 0u;
    out[e * 16 + r] = w;
}

template <int OP>
void launch_lane(const uint32_t *a, const uint32_t *b, uint32_t *out, int n) {
    hipLaunchKernelGGL(lane_kernel<OP>, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, a, b, out,
                       n);
}

template <int OP>
void launch_row(const uint32_t *a, const uint32_t *b, uint32_t *out, int rows) {
    hipLaunchKernelGGL(row_kernel<OP>, dim3((unsigned)(rows / 4)), dim3(kThreads), 0, 0, a, b, out);
}

bool launch(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, int n, int rows) {
    switch (op) {
#define FLM_LANE(o) case o: launch_lane<o>(a, b, out, n); return true;
        FLM_LANE(kFeMul) FLM_LANE(kFeSqr) FLM_LANE(kFeAdd) FLM_LANE(kFeSub) FLM_LANE(kFeNeg) FLM_LANE(kToMont)
        FLM_LANE(kFromMont) FLM_LANE(kFeIsZero) FLM_LANE(kFeEq) FLM_LANE(kFeLtP) FLM_LANE(kScMul) FLM_LANE(kScAdd)
        FLM_LANE(kScBelowN) FLM_LANE(kScLtN)
#undef FLM_LANE
        case kWnaf5:
            hipLaunchKernelGGL(wnaf5_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, a,
                               out, n);
            return true;
#define FLM_ROW(o) case o: launch_row<o>(a, b, out, rows); return true;
        FLM_ROW(kRowMul) FLM_ROW(kRowSqr) FLM_ROW(kRowAdd) FLM_ROW(kRowSub) FLM_ROW(kRowNeg) FLM_ROW(kRowCanon)
        FLM_ROW(kRowIsZero)
#undef FLM_ROW
        default: return false;
    }
}

}  // namespace
}  // namespace flm

extern "C" __attribute__((visibility("default"))) int flm_fieldtest_run(int op, const uint32_t *a, const uint32_t *b,
                                                                       uint32_t *out, int n, int device) {
    using namespace flm;
    const bool is_row = op >= kRowMul && op <= kRowIsZero;
    if (!(is_row || (op >= kFeMul && op <= kWnaf5)) || !a || !out || n < 0 || n > (1 << 24))
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const int rows = is_row ? (n + 3) / 4 * 4 : n;               // device rows, zero-padded to whole waves
    const size_t in_words = (size_t)rows * 8, out_per = is_row ? 16 : op == kWnaf5 ? (size_t)kNafWords : 8;
    uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
    hipError_t rc = hipSetDevice(device);
    if (rc == hipSuccess) rc = hipMalloc(&da, in_words * 4);
    if (rc == hipSuccess) rc = hipMalloc(&db, in_words * 4);
    if (rc == hipSuccess) rc = hipMalloc(&dout, (size_t)rows * out_per * 4);
    if (rc == hipSuccess) rc = hipMemset(da, 0, in_words * 4);
    if (rc == hipSuccess) rc = hipMemset(db, 0, in_words * 4);
    if (rc == hipSuccess) rc = hipMemset(dout, 0, (size_t)rows * out_per * 4);
    if (rc == hipSuccess) rc = hipMemcpy(da, a, (size_t)n * 32, hipMemcpyHostToDevice);
    if (rc == hipSuccess && b) rc = hipMemcpy(db, b, (size_t)n * 32, hipMemcpyHostToDevice);
    if (rc == hipSuccess) {
        launch(op, da, db, dout, n, rows);
        rc = hipGetLastError();
    }
    if (rc == hipSuccess) rc = hipDeviceSynchronize();
    if (rc == hipSuccess) rc = hipMemcpy(out, dout, (size_t)n * out_per * 4, hipMemcpyDeviceToHost);
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dout);
    return (int)rc;
}
