// cvs_contour_host.h -- what the host units of the contour tail share in front of their kernels (cvs_contour.cpp, which defines it,
// cvs_components.cpp, cvs_link.cpp, cvs_chains.cpp, cvs_chains_batch.cpp, cvs_polyline.cpp, cvs_refine.cpp, cvs_segments.cpp, cvs_turns.cpp,
// cvs_joins.cpp, cvs_paths.cpp, cvs_bridges.cpp): the checks every entry point begins with, the handle's scratch as a bump allocator, the routes of mask inputs and mask
// outputs, and the arrays of the chain calls -- their checks (with cvs_chain_table.h, the rules of a HOST chain table) and their staging
// (Staged).  Internal; the overlap rule of the tail is check_disjoint (cvs_context.h).
#pragma once
#include <algorithm>

#include "cvs_chain_table.h"
#include "cvs_components.h"
#include "cvs_context.h"

namespace cvs {

// ---- checks ----
int need_image(cvs_handle h);   // CVS_E_STATE before the first setup: the handle has no image size (each caller's pixel limit is its own)
int check_sized(cvs_handle h, const cvs_plane* p, const char* name, int rows, int cols, bool allow_u8 = false);   // check_plane, then check_same
int capturing(cvs_handle h, bool& yes);               // is the handle's stream being captured?
int refuse_capture(cvs_handle h, const char* what);   // CVS_E_UNSUPPORTED with `what` when it is: after every argument check, before the first launch

// a device f32 plane of the engine's own (a state plane, a plane of the handle's scratch) as a cvs_plane
inline cvs_plane device_plane(float* p, int rows, int cols, size_t pitch_elems)
{
    cvs_plane q{};
    q.data = p;
    q.rows = rows;
    q.cols = cols;
    q.step = pitch_elems * sizeof(float);
    q.mem = CVS_MEM_DEVICE;
    return q;
}

// ---- the handle's scratch as a bump allocator: sizes first (reserve), then one allocation ----
struct Scratch {
    size_t need = 0;
    size_t reserve(size_t bytes)
    {
        const size_t off = need;
        need += round_up(std::max<size_t>(bytes, 1), 256);
        return off;
    }
};
int grow_cc(cvs_handle h, size_t need);   // cvs_context::cc_scr of at least `need` bytes (only a call that allocates sets the device)

// ---- mask inputs: device bytes are read directly, everything else through in_ref (host planes staged, host bytes widened) ----
inline bool direct_u8(const cvs_plane* p) { return is_u8(p) && mem_of(p) == CVS_MEM_DEVICE; }   // (nothing for begin() to reserve)
int mask_ref(Call& c, const cvs_plane* p, MaskRef& m);

// ---- mask outputs: f32 planes through out_ref, device bytes directly, host bytes into `slot` (rows of slot_pitch bytes in the handle's
// scratch) and from there to the caller with fetch_mask, behind the launch that wrote them.  p / pitch: what the kernel's descriptor holds,
// the pitch in elements of the output's own type ----
inline bool staged_bytes(const cvs_plane* o, bool u8) { return u8 && mem_of(o) == CVS_MEM_HOST; }
int mask_out(Call& c, const cvs_plane* o, bool u8, unsigned char* slot, size_t slot_pitch, void*& p, size_t& pitch);
int fetch_mask(Call& c, const cvs_plane* o, bool u8, const void* p, size_t pitch);   // queues the copy; the caller synchronises

// ---- the arrays of a chain call (points, chain tables, xy, strength, record tables: 4-byte words in HOST or DEVICE memory) ----
inline bool misaligned(const void* p, size_t to = alignof(int32_t)) { return reinterpret_cast<uintptr_t>(p) % to != 0; }
// an array of `n` records of `words` 4-byte words as a plane, for the overlap rule of the contour tail (check_disjoint)
cvs_plane array_plane(const void* p, long long n, int words, int mem);

// Where the kernels of one chain call find its arrays.  The call binds every pointer its launches take, in the order the copies are to be
// queued: device-only scratch (always in cvs_context::ch_scr), inputs and outputs (the caller's own pointer for a DEVICE call, for which
// nothing is reserved; a slice of ch_scr for a HOST call; nullptr for an array the caller left out).  Then commit() -- one grow_scratch, which
// points every bound field into the block --, upload(), the launches, and fetch().  So "stage, launch, fetch" is one order for every call.
// commit() refuses (CVS_E_UNSUPPORTED) to grow the block while the stream is captured.  Of the calls in front of it only cvs_chain_joins, cvs_chain_paths
// and cvs_chain_bridges can meet that: the others reserve nothing for a DEVICE call, and have refused a captured HOST call before they stage.
// Whether and where a call sets the device stays its own business (only a call that allocates has to).
class Staged {
public:
    Staged(cvs_handle h, const char* call, bool host) : h_(h), call_(call), host_(host) {}
    template <class T>
    void scratch(T*& dev, size_t bytes) { bind(&dev, nullptr, bytes, kNone); }
    template <class T>
    void in(const T*& dev, const void* src, size_t bytes) { dev = static_cast<const T*>(src); stage(&dev, const_cast<void*>(src), bytes, kUp); }
    template <class T>
    void out(T*& dev, void* dst, size_t bytes) { dev = static_cast<T*>(dst); stage(&dev, dst, bytes, kDown); }
    int commit();
    int upload(hipStream_t s);     // every input of a HOST call that holds a byte, in the order bound
    int download(hipStream_t s);   // every output of a HOST call that holds a byte, in the order bound; queued only
    int fetch(hipStream_t s);      // download(), and a HOST call waits for it

private:
    enum Dir { kNone, kUp, kDown };
    struct Item {
        void* field;   // the bound pointer: commit() stores base + off there
        void* host;
        size_t off, bytes;
        Dir dir;
    };
    void stage(void* field, void* host, size_t bytes, Dir dir) { if (host_ && host) bind(field, host, bytes, dir); }
    void bind(void* field, void* host, size_t bytes, Dir dir) { items_[n_++] = Item{field, host, sc_.reserve(bytes), bytes, dir}; }
    int copy(hipStream_t s, Dir dir);
    static constexpr int kMaxItems = 12;   // (cvs_chain_paths binds the most: scratch, four inputs, seven outputs)
    cvs_handle h_;
    const char* call_;
    bool host_;
    Scratch sc_;
    Item items_[kMaxItems];
    int n_ = 0;
};

}  // namespace cvs
