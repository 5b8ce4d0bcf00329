// flm_host_layout.h -- where each array of a host-pointer call goes (HostCopies, flm_runtime.hip),
// and how a large one is cut into staging-buffer pieces.  Plain C++ with no HIP in it, so the rules
// are checked on the CPU (tests/test_host_layout_cpu.py, tools/planner_check.cpp).  Which arrays a call
// declares -- the round path's and the batch crypto calls' alike -- at which width, rows and pitches, and in
// which of the context's buffers, is flm_call_args.h (tools/args_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace flm {
namespace rt __attribute__((visibility("hidden"))) {  // the library exports nothing of this header

// One pinned staging buffer; also the size from which a copy skips the bounce buffer.
constexpr size_t kStageBytes = size_t(32) << 20;

enum HostRoute : int {
    kRouteInPlace = 0,  // the kernel reads or writes the bounce buffer itself, rows at `pitch`
    kRouteBounce = 1,   // packed in the bounce buffer, one DMA to or from device memory
    kRouteRing = 2,     // streamed through the two staging buffers in pieces: no bounce bytes
};

struct HostSpan {
    size_t width, rows;  // bytes per row, rows
    bool may_in_place;
    HostRoute route;       // host_layout's answer: the route, the bytes between rows in the bounce
    size_t pitch, offset;  // buffer, and the offset into it (a multiple of 256)
};

// Routes the spans of one call and packs them into the bounce buffer in the order given; returns
// the bounce bytes the call needs.  One size per span decides its route AND sizes its space: the
// padded rows x round_up(width, 16) in place, else the packed rows x width.  The products are
// plain size_t: the caller bounds width x rows (the entry points do, by the memory they index).
inline size_t host_layout(HostSpan *spans, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        HostSpan &s = spans[i];
        const size_t padded = (s.width + 15) / 16 * 16, packed = s.width * s.rows;
        const bool in_place = s.may_in_place && s.rows * padded < kStageBytes;
        s.route = in_place ? kRouteInPlace : packed < kStageBytes ? kRouteBounce : kRouteRing;
        s.pitch = in_place ? padded : s.width;
        s.offset = total;
        total += (s.route == kRouteRing ? 0 : (s.rows * s.pitch + 255) / 256 * 256);
    }
    return total;
}

// Pieces of at most kStageBytes of a rows x width copy: whole rows, or one row's columns.
struct Piece {
    size_t r, c, w, nr;  // first row, first column, bytes per row, rows
};
inline std::vector<Piece> pieces(size_t width, size_t rows) {
    std::vector<Piece> v;
    if (width > kStageBytes) {
        for (size_t r = 0; r < rows; ++r)
            for (size_t c = 0; c < width; c += kStageBytes) v.push_back({r, c, std::min(kStageBytes, width - c), 1});
    } else {
        const size_t per = kStageBytes / width;
        for (size_t r = 0; r < rows; r += per) v.push_back({r, 0, width, std::min(per, rows - r)});
    }
    return v;
}

}  // namespace rt
}  // namespace flm
