// cvs_overlap.h -- what the overlapped host paths share (cvs_batch.cpp: frames of a shard, chunk by chunk; cvs_host.cpp: one image, band by
// band): which items a rank owns, how a shard is cut into chunks, which planes leave as one copy, and how the thread that queues launches
// tells the download thread what it may fetch.  Like cvs_layout.h, nothing here calls the device or dereferences a plane -- the copies are
// the callbacks' -- so tests/cpp/host_logic_san.cpp holds every piece to a model under ASan / UBSan.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "cvs_layout.h"

namespace cvs {

// contiguous block [lo, hi) of `rank`: item f belongs to rank floor(f * world / n)
inline void shard_range(int n, int world, int rank, int* lo, int* hi)
{
    *lo = (int)(((long long)rank * n + world - 1) / world);
    *hi = (int)(((long long)(rank + 1) * n + world - 1) / world);
}

// A shard of n frames as chunks [c[k], c[k + 1]): the starts 0 ... n.  `whole` = one chunk (state kept: the handle's frames after the call
// must be the whole shard).  Otherwise chunks GROW: the downloads set the pace (three maps down for one frame up) and run back to back once
// the first chunk's maps exist, so what the chunking costs is the time until then -- upload + launch of the FIRST chunk.  A thirty-second of
// the shard first, every later chunk twice its predecessor (its upload and launch hide behind the predecessor's download), the fifth chunk
// -- or an earlier one, once what is left is within one and a half times its size -- takes the rest: 1 | 2 | 4 | 8 | 17 frames for a shard of
// 32 instead of four chunks of 8: 0.79 -> 0.84 of the link's roof for 8-bit frames in / three 8-bit maps out (profiles/r06_host_chunks.txt).
inline std::vector<int> chunk_starts(int n, bool whole)
{
    std::vector<int> c(1, 0);
    if (whole) c.push_back(n);
    else
        for (int sz = std::max(1, n / 32); c.back() < n; sz *= 2) c.push_back((n - c.back() <= sz + sz / 2 || c.size() >= 5) ? n : c.back() + sz);
    return c;
}

// n planes of plane_bytes = rows * row_bytes each, staged back to back (plane i at i * plane_bytes) and lying on the host wherever
// at(i) -> PlaneAt says.  Dense planes (step == row_bytes) that lie back to back on the host too -- the usual [n][K][rows][cols] block -- make
// ONE run: linear(first, count, addr of the first) per maximal run, in order; a plane with padded rows ends the open run and gets
// pitched(i, addr, step) of its own.  A callback returns false to stop the walk (nothing is called after it); -> false then.
template <class At, class Linear, class Pitched>
bool walk_runs(size_t n, size_t plane_bytes, size_t row_bytes, At at, Linear linear, Pitched pitched)
{
    size_t first = 0, count = 0;
    uintptr_t run = 0;
    auto flush = [&] {
        const bool ok = !count || linear(first, count, run);
        count = 0;
        return ok;
    };
    for (size_t i = 0; i < n; ++i) {
        const PlaneAt p = at(i);
        if (p.step != row_bytes) {
            if (!flush() || !pitched(i, p.addr, p.step)) return false;
        } else if (count && p.addr == run + count * plane_bytes) {
            ++count;
        } else {
            if (!flush()) return false;
            first = i;
            run = p.addr;
            count = 1;
        }
    }
    return flush();
}

// The producer queues items 0, 1, ... and says so; the worker takes item k once it is published.  stop() releases a waiting worker for
// good: a producer that fails MUST call it before it joins the worker, which otherwise waits for an item that never comes.
class Gate {
public:
    void publish(int k)   // items below k are queued
    {
        {
            std::lock_guard<std::mutex> lock(mu_);
            published_ = k;
        }
        cv_.notify_all();
    }
    bool wait(int k)   // -> item k is queued; false = stopped
    {
        std::unique_lock<std::mutex> lock(mu_);
        cv_.wait(lock, [&] { return published_ > k || stopped_; });
        return !stopped_;
    }
    void stop()
    {
        {
            std::lock_guard<std::mutex> lock(mu_);
            stopped_ = true;
        }
        cv_.notify_all();
    }

private:
    std::mutex mu_;
    std::condition_variable cv_;
    int published_ = 0;
    bool stopped_ = false;
};

}  // namespace cvs
