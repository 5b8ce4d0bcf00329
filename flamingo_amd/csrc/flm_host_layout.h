// flm_host_layout.h -- where each array of a host-pointer call goes (HostCopies, flm_runtime.hip).
// Plain C++ with no HIP in it, so the rule is checked on the CPU (tests/test_host_layout_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace flm {
namespace rt {

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

}  // namespace rt
}  // namespace flm
