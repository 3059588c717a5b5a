// cvs_layout.h -- how a set of planes lies in memory: the two questions every one-launch route asks before it hands a kernel "frame 0
// plus z strides" instead of a table of pointers.  Addresses and row steps only: nothing here dereferences a plane, calls the device or
// knows a handle, so tests/cpp/host_logic_san.cpp drives it on made-up addresses.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "cvsteer_hip.h"

namespace cvs {

struct PlaneAt {
    uintptr_t addr;   // byte address, 0 = absent
    size_t step;      // row step in bytes
};
inline PlaneAt plane_at(const cvs_plane& p) { return {reinterpret_cast<uintptr_t>(p.data), p.step}; }

struct PlaneRun {
    bool ok;
    ptrdiff_t stride;   // bytes from frame i to frame i + 1 (0 with one frame, or with no plane present)
};

// n frames of K planes, at(i, k) = plane k of frame i: ok when a plane is present in every frame or in none, every present plane keeps
// frame 0's row step, and frame i's planes lie i * stride behind frame 0's -- ONE stride >= 0 for all K.  Planes of different k may differ
// in step and lie anywhere relative to each other.  Per site (only n > 1 frames have a stride): zero_ok = false refuses a stride of 0
// (every frame the same planes); the stride must be a multiple of `divisor` bytes.
template <class At>
PlaneRun plane_run(int n, int K, At at, bool zero_ok, ptrdiff_t divisor = 1)
{
    ptrdiff_t stride = 0;
    bool have = false;
    for (int k = 0; k < K; ++k) {
        const PlaneAt p0 = at(0, k);
        for (int i = 1; i < n; ++i) {
            const PlaneAt pi = at(i, k);
            if ((pi.addr == 0) != (p0.addr == 0)) return {false, 0};
            if (!p0.addr) continue;
            const ptrdiff_t d = (ptrdiff_t)(pi.addr - p0.addr);
            if (!have) {   // (i == 1: the first present plane's second frame sets the stride)
                stride = d;
                have = true;
            }
            if (d != stride * i || pi.step != p0.step) return {false, 0};
        }
    }
    if (have && (stride < 0 || (stride == 0 && !zero_ok) || stride % divisor != 0)) return {false, 0};
    return {true, stride};
}

// Up to eight planes of one frame (absent ones skipped) as ONE buffer resource: the lowest base, each plane's byte offset from it, and
// the span up to the end of the last plane's last row.  ok = the present planes share one row step and the span is within `limit`.
struct OneResource {
    bool ok;
    uintptr_t base;
    size_t step, span;
    unsigned off[8];   // (saturated: an offset beyond 32 bits is never ok)
    unsigned mask;     // bit k = plane k is present
};
inline OneResource one_resource(const PlaneAt planes[8], int rows, size_t limit)
{
    OneResource r{true, 0, 0, 0, {}, 0};
    for (int k = 0; k < 8; ++k) {
        if (!planes[k].addr) continue;
        if (!r.mask) r.step = planes[k].step;
        if (!r.mask || planes[k].addr < r.base) r.base = planes[k].addr;
        r.ok = r.ok && planes[k].step == r.step;
        r.mask |= 1u << k;
    }
    for (int k = 0; k < 8; ++k) {
        if (!planes[k].addr) continue;
        const size_t off = planes[k].addr - r.base;
        r.off[k] = (unsigned)std::min<size_t>(off, 0xffffffffu);
        r.span = std::max(r.span, off + (size_t)rows * r.step);
    }
    r.ok = r.ok && r.span <= limit;
    return r;
}

}  // namespace cvs
