// facade.cpp -- fa::SteerableFilters / SteerableFiltersG2 / SteerableFiltersG4 on top of the C ABI
// (include/cvsteer_hip.h).  Builds libcvsteer.so: the library name the reference installs
// (cvsteer/CMakeLists.txt: target `cvsteer`), so an existing `-lcvsteer` link line picks up the
// MI355X engine.  No arithmetic on image data happens here: every method marshals fa::Mat1f
// views into cvs_plane structs and calls the HIP library.  Errors become std::runtime_error
// (the reference surfaces errors as cv::Exception thrown from inside OpenCV).
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include <cstddef>
#include <limits>
#include <mutex>
#include <stdexcept>
#include <string>
#include <typeinfo>
#include <vector>

#include "cvsteer_hip.h"

namespace fa {

namespace {

cvs_plane view(const Mat1f& m)
{
    cvs_plane p;
    p.data = const_cast<float*>(reinterpret_cast<const float*>(m.data));
    p.rows = m.rows;
    p.cols = m.cols;
    p.step = (size_t)m.step;
    if (m.rows == 1 || p.step == 0) p.step = (size_t)m.cols * sizeof(float);
    p.mem = CVS_MEM_HOST;
    return p;
}

// (re)allocate an output the way cv::Mat::create does: no-op when the size already matches
cvs_plane out_view(Mat1f& m, int rows, int cols)
{
    m.create(rows, cols);
    return view(m);
}

void throw_status(cvs_handle h, int status, const char* where)
{
    std::string msg = std::string("cvsteer: ") + where + ": " + cvs_status_string(status);
    if (h) {
        const char* d = cvs_last_error(h);
        if (d && *d) msg += std::string(" (") + d + ")";
    }
    throw std::runtime_error(msg);
}

// handle for the static, object-less entry points (phaseWeights, wrap)
std::mutex g_static_mutex;
cvs_handle static_handle()
{
    static cvs_handle h = 0;
    if (!h) {
        int rc = cvs_create(CVS_KIND_G2, 4, 0.67f, 0, &h);
        if (rc != CVS_OK) throw_status(0, rc, "cvs_create (static helper handle; no HIP device?)");
    }
    return h;
}

Mat1f taps_of(cvs_handle h, int idx, int width)
{
    Mat1f k(1, 2 * width + 1);
    cvs_taps(h, idx, reinterpret_cast<float*>(k.data));
    return k;
}

// contour components (extension), shared by the G2 and G4 classes: status, or the number of components through *n
int prune_contours(cvs_handle h, const Mat1f& mask, const Mat1f& weight, int minArea, float minPeak, Mat1f& out, int* n)
{
    cvs_plane pm = view(mask), pw = view(weight), po = out_view(out, mask.rows, mask.cols);
    return cvs_contour_prune(h, 1, &pm, weight.empty() ? 0 : &pw, minArea, minPeak, &po, n);
}

int count_components(cvs_handle h, const Mat1f& mask, int* n)
{
    std::vector<int32_t> labels((size_t)mask.rows * (size_t)mask.cols);
    cvs_plane pm = view(mask), pl;
    pl.data = reinterpret_cast<float*>(labels.data());
    pl.rows = mask.rows;
    pl.cols = mask.cols;
    pl.step = (size_t)mask.cols * sizeof(int32_t);
    pl.mem = CVS_MEM_HOST | CVS_DEPTH_S32;
    return cvs_label(h, &pm, &pl, n);
}

// sized by a first call, then filled; the host loop here only re-packs the finished lists into vectors
int trace_contours(cvs_handle h, const Mat1f& mask, std::vector<std::vector<Point> >& out, std::vector<int>* flags, int* n)
{
    cvs_plane pm = view(mask);
    int np = 0, nc = 0;
    int rc = cvs_contour_chains(h, &pm, 0, 0, 0, 0, CVS_MEM_HOST, &np, &nc);
    if (rc != CVS_OK && rc != CVS_E_SIZE) return rc;
    std::vector<int32_t> pts((size_t)np * 2);
    std::vector<cvs_chain> tab((size_t)nc);
    if (np > 0 && (rc = cvs_contour_chains(h, &pm, pts.data(), np, tab.data(), nc, CVS_MEM_HOST, &np, &nc)) != CVS_OK) return rc;
    out.assign((size_t)nc, std::vector<Point>());
    if (flags) flags->assign((size_t)nc, 0);
    for (int c = 0; c < nc; ++c) {
        const cvs_chain& t = tab[(size_t)c];
        out[(size_t)c].reserve((size_t)t.length);
        for (int k = 0; k < t.length; ++k) out[(size_t)c].push_back(Point(pts[2 * (size_t)(t.start + k)], pts[2 * (size_t)(t.start + k) + 1]));
        if (flags) (*flags)[(size_t)c] = t.flags;
    }
    *n = nc;
    return CVS_OK;
}

// the chains packed into one point list and a table, one call, the polylines unpacked again: no arithmetic on the host
int approx_contours(cvs_handle h, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, float eps,
                    std::vector<std::vector<Point> >& out, int* n)
{
    if (flags && flags->size() != chains.size()) return CVS_E_BADARG;
    size_t np = 0;
    for (size_t c = 0; c < chains.size(); ++c) np += chains[c].size();
    if (np > (size_t)1 << 30) return CVS_E_SIZE;
    std::vector<int32_t> pts(np * 2), vtx(np * 2);
    std::vector<cvs_chain> tab(chains.size()), pol(chains.size());
    size_t at = 0;
    for (size_t c = 0; c < chains.size(); ++c) {
        tab[c].start = (int32_t)at;
        tab[c].length = (int32_t)chains[c].size();
        tab[c].flags = flags ? (*flags)[c] : 0;
        tab[c].reserved = 0;
        for (size_t k = 0; k < chains[c].size(); ++k, ++at) {
            pts[2 * at] = chains[c][k].x;
            pts[2 * at + 1] = chains[c][k].y;
        }
    }
    int nv = 0;
    const int rc = cvs_chain_polylines(h, pts.data(), (int)np, tab.data(), (int)chains.size(), eps, vtx.data(), (int)np, 0, pol.data(),
                                       CVS_MEM_HOST, &nv);
    if (rc != CVS_OK) return rc;
    out.assign(chains.size(), std::vector<Point>());
    for (size_t c = 0; c < chains.size(); ++c) {
        const cvs_chain& t = pol[c];
        out[c].reserve((size_t)t.length);
        for (int k = 0; k < t.length; ++k) out[c].push_back(Point(vtx[2 * (size_t)(t.start + k)], vtx[2 * (size_t)(t.start + k) + 1]));
    }
    *n = nv;
    return CVS_OK;
}

// the chains packed into one point list, one call on the handle's own theta, the pairs unpacked again: no arithmetic on the host
int refine_contours(cvs_handle h, const Mat1f& response, const std::vector<std::vector<Point> >& chains, std::vector<std::vector<float> >& xs,
                    std::vector<std::vector<float> >& ys, std::vector<std::vector<float> >* strength, int* n)
{
    size_t np = 0;
    for (size_t c = 0; c < chains.size(); ++c) np += chains[c].size();
    if (np > (size_t)1 << 30) return CVS_E_SIZE;
    std::vector<int32_t> pts(np * 2);
    std::vector<float> xy(np * 2), str(strength ? np : 0);
    size_t at = 0;
    for (size_t c = 0; c < chains.size(); ++c)
        for (size_t k = 0; k < chains[c].size(); ++k, ++at) {
            pts[2 * at] = chains[c][k].x;
            pts[2 * at + 1] = chains[c][k].y;
        }
    cvs_plane pr = view(response);
    const int rc = cvs_chain_refine(h, &pr, 0, pts.data(), (int)np, xy.data(), strength ? str.data() : 0, CVS_MEM_HOST);
    if (rc != CVS_OK) return rc;
    xs.assign(chains.size(), std::vector<float>());
    ys.assign(chains.size(), std::vector<float>());
    if (strength) strength->assign(chains.size(), std::vector<float>());
    at = 0;
    for (size_t c = 0; c < chains.size(); ++c) {
        const size_t len = chains[c].size();
        xs[c].resize(len);
        ys[c].resize(len);
        for (size_t k = 0; k < len; ++k) {
            xs[c][k] = xy[2 * (at + k)];
            ys[c][k] = xy[2 * (at + k) + 1];
        }
        if (strength) (*strength)[c].assign(str.begin() + (std::ptrdiff_t)at, str.begin() + (std::ptrdiff_t)(at + len));
        at += len;
    }
    *n = (int)np;
    return CVS_OK;
}

// approx_contours (with the index), refine_contours on the handle's own theta and cvs_polyline_segments on their results, one packing for
// the three calls; the host loop only evaluates the end points of the finished records and narrows them to float
int fit_segments(cvs_handle h, const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, float eps,
                 std::vector<std::vector<float> >& lines, std::vector<std::vector<float> >* rms, int* n)
{
    if (flags && flags->size() != chains.size()) return CVS_E_BADARG;
    size_t np = 0;
    for (size_t c = 0; c < chains.size(); ++c) np += chains[c].size();
    if (np > (size_t)1 << 30) return CVS_E_SIZE;
    std::vector<int32_t> pts(np * 2), vtx(np * 2), idx(np);
    std::vector<float> xy(np * 2);
    std::vector<cvs_chain> tab(chains.size()), pol(chains.size());
    size_t at = 0;
    for (size_t c = 0; c < chains.size(); ++c) {
        tab[c].start = (int32_t)at;
        tab[c].length = (int32_t)chains[c].size();
        tab[c].flags = flags ? (*flags)[c] : 0;
        tab[c].reserved = 0;
        for (size_t k = 0; k < chains[c].size(); ++k, ++at) {
            pts[2 * at] = chains[c][k].x;
            pts[2 * at + 1] = chains[c][k].y;
        }
    }
    int nv = 0;
    int rc = cvs_chain_polylines(h, pts.data(), (int)np, tab.data(), (int)chains.size(), eps, vtx.data(), (int)np, idx.data(), pol.data(),
                                 CVS_MEM_HOST, &nv);
    if (rc != CVS_OK) return rc;
    cvs_plane pr = view(response);
    if ((rc = cvs_chain_refine(h, &pr, 0, pts.data(), (int)np, xy.data(), 0, CVS_MEM_HOST)) != CVS_OK) return rc;
    std::vector<cvs_segment> seg((size_t)nv);
    rc = cvs_polyline_segments(h, pts.data(), (int)np, tab.data(), pol.data(), (int)chains.size(), idx.data(), nv, xy.data(), 0, seg.data(),
                               CVS_MEM_HOST);
    if (rc != CVS_OK) return rc;
    lines.assign(chains.size(), std::vector<float>());
    if (rms) rms->assign(chains.size(), std::vector<float>());
    int count = 0;
    for (int k = 0; k < nv; ++k) {
        const cvs_segment& s = seg[(size_t)k];
        if (s.count < 2 || (s.flags & CVS_SEG_DEGENERATE)) continue;
        std::vector<float>& out = lines[(size_t)s.chain];
        out.push_back((float)(s.cx + s.t0 * s.ux));
        out.push_back((float)(s.cy + s.t0 * s.uy));
        out.push_back((float)(s.cx + s.t1 * s.ux));
        out.push_back((float)(s.cy + s.t1 * s.uy));
        if (rms) (*rms)[(size_t)s.chain].push_back((float)s.rms);
        ++count;
    }
    *n = count;
    return CVS_OK;
}

// refine_contours on the handle's own theta and cvs_chain_turns on its result, one packing for the two calls; the host loop only sorts the
// corner records into their chains
int corner_contours(cvs_handle h, const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, int radius,
                    float maxCosine, std::vector<std::vector<int> >& corners, std::vector<std::vector<float> >* cosines, int* n)
{
    if (flags && flags->size() != chains.size()) return CVS_E_BADARG;
    size_t np = 0;
    for (size_t c = 0; c < chains.size(); ++c) np += chains[c].size();
    if (np > (size_t)1 << 30) return CVS_E_SIZE;
    std::vector<int32_t> pts(np * 2);
    std::vector<float> xy(np * 2);
    std::vector<cvs_chain> tab(chains.size());
    size_t at = 0;
    for (size_t c = 0; c < chains.size(); ++c) {
        tab[c].start = (int32_t)at;
        tab[c].length = (int32_t)chains[c].size();
        tab[c].flags = flags ? (*flags)[c] : 0;
        tab[c].reserved = 0;
        for (size_t k = 0; k < chains[c].size(); ++k, ++at) {
            pts[2 * at] = chains[c][k].x;
            pts[2 * at + 1] = chains[c][k].y;
        }
    }
    cvs_plane pr = view(response);
    int rc = cvs_chain_refine(h, &pr, 0, pts.data(), (int)np, xy.data(), 0, CVS_MEM_HOST);
    if (rc != CVS_OK) return rc;
    cvs_turn_cfg cfg;
    cfg.radius = cfg.min_arm = cfg.nms = radius;
    cfg.max_cos = maxCosine;
    std::vector<cvs_chain_turn> turns(np);
    if ((rc = cvs_chain_turns(h, pts.data(), (int)np, tab.data(), (int)chains.size(), xy.data(), &cfg, turns.data(), 0, CVS_MEM_HOST)) != CVS_OK)
        return rc;
    corners.assign(chains.size(), std::vector<int>());
    if (cosines) cosines->assign(chains.size(), std::vector<float>());
    int count = 0;
    for (size_t i = 0; i < np; ++i) {
        const cvs_chain_turn& t = turns[i];
        if (!(t.flags & CVS_TURN_CORNER)) continue;
        corners[(size_t)t.chain].push_back((int)(i - (size_t)tab[(size_t)t.chain].start));
        if (cosines) (*cosines)[(size_t)t.chain].push_back(t.cos);
        ++count;
    }
    *n = count;
    return CVS_OK;
}

// refine_contours on the handle's own theta and cvs_chain_joins on its result, one packing for the two calls; the host loop only copies the
// partners of the mutual joins out of the records
int join_contours(cvs_handle h, const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, int radius,
                  float minCosine, std::vector<int>& partners, std::vector<float>* cosines, int* n)
{
    if (flags && flags->size() != chains.size()) return CVS_E_BADARG;
    size_t np = 0;
    for (size_t c = 0; c < chains.size(); ++c) np += chains[c].size();
    if (np > (size_t)1 << 30 || chains.size() > (size_t)1 << 26) return CVS_E_SIZE;
    std::vector<int32_t> pts(np * 2);
    std::vector<float> xy(np * 2);
    std::vector<cvs_chain> tab(chains.size());
    size_t at = 0;
    for (size_t c = 0; c < chains.size(); ++c) {
        tab[c].start = (int32_t)at;
        tab[c].length = (int32_t)chains[c].size();
        tab[c].flags = flags ? (*flags)[c] : 0;
        tab[c].reserved = 0;
        for (size_t k = 0; k < chains[c].size(); ++k, ++at) {
            pts[2 * at] = chains[c][k].x;
            pts[2 * at + 1] = chains[c][k].y;
        }
    }
    cvs_plane pr = view(response);
    int rc = cvs_chain_refine(h, &pr, 0, pts.data(), (int)np, xy.data(), 0, CVS_MEM_HOST);
    if (rc != CVS_OK) return rc;
    cvs_join_cfg cfg;
    cfg.radius = radius;
    cfg.min_arm = radius < 3 ? radius : 3;
    cfg.min_cos = minCosine;
    cfg.reserved = 0;
    std::vector<cvs_chain_join> joins(2 * chains.size());
    if ((rc = cvs_chain_joins(h, pts.data(), (int)np, tab.data(), (int)chains.size(), xy.data(), &cfg, joins.data(), CVS_MEM_HOST)) != CVS_OK)
        return rc;
    partners.assign(joins.size(), -1);
    if (cosines) cosines->assign(joins.size(), std::numeric_limits<float>::quiet_NaN());
    int count = 0;
    for (size_t e = 0; e < joins.size(); ++e) {
        const cvs_chain_join& j = joins[e];
        if (!(j.flags & CVS_JOIN_MUTUAL)) continue;
        partners[e] = j.partner;
        if (cosines) (*cosines)[e] = j.cos;
        if ((size_t)j.partner > e) ++count;   // each pair once
    }
    *n = count;
    return CVS_OK;
}

// cvs_chain_paths on host arrays: the chains packed as for the joins, a join table that holds nothing but the partners of the mutual joins
// (what joinContours returned), and the paths, their flags and their member lists unpacked from the records
int stitch_contours(cvs_handle h, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, const std::vector<int>& partners,
                    std::vector<std::vector<Point> >& paths, std::vector<int>* pathFlags, std::vector<std::vector<int> >* members, int* n)
{
    if ((flags && flags->size() != chains.size()) || partners.size() != 2 * chains.size()) return CVS_E_BADARG;
    size_t np = 0;
    for (size_t c = 0; c < chains.size(); ++c) np += chains[c].size();
    if (np > (size_t)1 << 30 || chains.size() > (size_t)1 << 26) return CVS_E_SIZE;
    std::vector<int32_t> pts(np * 2), out(np * 2);
    std::vector<cvs_chain> tab(chains.size()), ptab(chains.size());
    std::vector<cvs_chain_join> joins(2 * chains.size());
    std::vector<cvs_path_info> info(chains.size());
    std::vector<cvs_path_member> mem(chains.size());
    size_t at = 0;
    for (size_t c = 0; c < chains.size(); ++c) {
        tab[c].start = (int32_t)at;
        tab[c].length = (int32_t)chains[c].size();
        tab[c].flags = flags ? (*flags)[c] : 0;
        tab[c].reserved = 0;
        for (size_t k = 0; k < chains[c].size(); ++k, ++at) {
            pts[2 * at] = chains[c][k].x;
            pts[2 * at + 1] = chains[c][k].y;
        }
    }
    for (size_t e = 0; e < joins.size(); ++e) {
        cvs_chain_join j = cvs_chain_join();
        j.node = j.next = -1;
        j.partner = partners[e];
        j.flags = partners[e] >= 0 ? CVS_JOIN_MUTUAL : CVS_JOIN_NONE;
        j.cos = j.sin = std::numeric_limits<float>::quiet_NaN();
        joins[e] = j;
    }
    int32_t counts[2] = {0, 0};
    const int rc = cvs_chain_paths(h, pts.data(), (int)np, tab.data(), (int)chains.size(), joins.data(), 0, out.data(), ptab.data(), info.data(),
                                   mem.data(), 0, 0, counts, CVS_MEM_HOST);
    if (rc != CVS_OK) return rc;
    paths.assign((size_t)counts[0], std::vector<Point>());
    if (pathFlags) pathFlags->assign((size_t)counts[0], 0);
    if (members) members->assign((size_t)counts[0], std::vector<int>());
    for (size_t p = 0; p < (size_t)counts[0]; ++p) {
        paths[p].reserve((size_t)ptab[p].length);
        for (int32_t k = ptab[p].start; k < ptab[p].start + ptab[p].length; ++k) paths[p].push_back(Point(out[2 * (size_t)k], out[2 * (size_t)k + 1]));
        if (pathFlags) (*pathFlags)[p] = ptab[p].flags;
        if (members)
            for (int32_t m = info[p].first_member; m < info[p].first_member + info[p].n_members; ++m)
                (*members)[p].push_back(2 * mem[(size_t)m].chain + ((mem[(size_t)m].flags & CVS_MEMBER_REVERSED) ? 1 : 0));
    }
    *n = counts[0];
    return CVS_OK;
}

// cvs_chain_bridges on host arrays, on the integer points: the chains packed as for the joins, one call with room for every bridge there can
// be (one per chain, max_gap + 1 points each), and the bridged table unpacked -- the chains, then the bridges, and for stitch_contours the
// partners the bridges make: the smaller end of a pair continues into the bridge's head, the bridge's tail into the larger end
int bridge_contours(cvs_handle h, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, int radius, int maxGap,
                    float minCosine, std::vector<std::vector<Point> >& bridged, std::vector<int>& bridgedFlags, std::vector<int>* partners, int* n)
{
    if (flags && flags->size() != chains.size()) return CVS_E_BADARG;
    if (maxGap < 2 || maxGap > CVS_BRIDGE_MAX_GAP) return CVS_E_BADARG;
    size_t np = 0;
    for (size_t c = 0; c < chains.size(); ++c) np += chains[c].size();
    const size_t capPoints = np + chains.size() * ((size_t)maxGap + 1), capChains = 2 * chains.size();
    if (np > (size_t)1 << 30 || chains.size() > (size_t)1 << 26 || capPoints > (size_t)0x7fffffff) return CVS_E_SIZE;
    std::vector<int32_t> pts(np * 2), out(capPoints * 2);
    std::vector<cvs_chain> tab(chains.size()), otab(capChains);
    std::vector<cvs_chain_bridge> rec(2 * chains.size());
    size_t at = 0;
    for (size_t c = 0; c < chains.size(); ++c) {
        tab[c].start = (int32_t)at;
        tab[c].length = (int32_t)chains[c].size();
        tab[c].flags = flags ? (*flags)[c] : 0;
        tab[c].reserved = 0;
        for (size_t k = 0; k < chains[c].size(); ++k, ++at) {
            pts[2 * at] = chains[c][k].x;
            pts[2 * at + 1] = chains[c][k].y;
        }
    }
    cvs_bridge_cfg cfg;
    cfg.radius = radius;
    cfg.min_arm = radius < 3 ? radius : 3;
    cfg.max_gap = maxGap;
    cfg.min_cos = minCosine;
    int32_t counts[3] = {0, 0, 0};
    const int rc = cvs_chain_bridges(h, pts.data(), (int)np, tab.data(), (int)chains.size(), 0, &cfg, rec.data(), chains.empty() ? 0 : out.data(),
                                     chains.empty() ? 0 : (int)capPoints, chains.empty() ? 0 : otab.data(), chains.empty() ? 0 : (int)capChains, 0,
                                     counts, CVS_MEM_HOST);
    if (rc != CVS_OK) return rc;
    const size_t total = (size_t)counts[1];
    if (total > capChains || (size_t)counts[2] > capPoints) return CVS_E_HIP;   // (never: the capacities hold every bridge there can be)
    bridged.assign(total, std::vector<Point>());
    bridgedFlags.assign(total, 0);
    for (size_t c = 0; c < total; ++c) {
        bridged[c].reserve((size_t)otab[c].length);
        for (int32_t k = otab[c].start; k < otab[c].start + otab[c].length; ++k) bridged[c].push_back(Point(out[2 * (size_t)k], out[2 * (size_t)k + 1]));
        bridgedFlags[c] = otab[c].flags;
    }
    if (partners) {
        partners->assign(2 * total, -1);
        for (size_t e = 0; e < rec.size(); ++e) {
            const cvs_chain_bridge& b = rec[e];
            if (!(b.flags & CVS_BRIDGE_MUTUAL) || b.bridge < 0) continue;
            const int end = 2 * ((int)chains.size() + b.bridge) + ((size_t)b.partner > e ? 0 : 1);   // the smaller end meets the bridge's head
            (*partners)[e] = end;
            (*partners)[(size_t)end] = (int)e;
        }
    }
    *n = counts[0];
    return CVS_OK;
}

}  // namespace

// --------------------------------------------------------------------------- base
SteerableFilters::SteerableFilters(int kind, int width, float spacing, int device) : m_memberSync(true), m_handle(0), m_device(device)
{
    int rc = cvs_create(kind, width, spacing, device, &m_handle);
    if (rc != CVS_OK) throw_status(0, rc, "cvs_create (is a HIP device present? there is no CPU fallback)");
}

SteerableFilters::~SteerableFilters()
{
    if (m_handle) cvs_destroy(m_handle);
}

void SteerableFilters::check(int status, const char* where) const
{
    if (status != CVS_OK) throw_status(m_handle, status, where);
}

// Only a subclass can read the protected plane members, so only objects whose dynamic type is NOT the facade class
// itself get them filled after setup().  (Inside a base-class constructor typeid(*this) is the base class: a subclass
// constructor that wants them calls syncMembers() itself.)
bool SteerableFilters::memberSyncWanted(const void* exact_type_info) const
{
    return m_memberSync && typeid(*this) != *static_cast<const std::type_info*>(exact_type_info);
}

void SteerableFilters::synchronize() { check(cvs_sync(m_handle), "cvs_sync"); }

void SteerableFilters::setExactAtan(bool on) { check(cvs_set_option(m_handle, CVS_OPT_ATAN_MODE, on ? 1 : 0), "cvs_set_option"); }

void SteerableFilters::fetch(int which, Mat1f& dst) const
{
    int rows = 0, cols = 0;
    check(cvs_shape(m_handle, &rows, &cols), "cvs_shape");
    if (rows == 0 || cols == 0) throw_status(m_handle, CVS_E_STATE, "fetch");
    cvs_plane p = out_view(dst, rows, cols);
    check(cvs_read_state(m_handle, which, &p), "cvs_read_state");
}

Mat1f SteerableFilters::create(int width, float spacing, KernelType f)
{
    Mat1f kernel(1, width * 2 + 1);
    float* k = reinterpret_cast<float*>(kernel.data);
    for (int i = -width; i <= width; i++) k[i + width] = f(float(i) * spacing);
    return kernel;
}

void SteerableFilters::wrap(const Mat1f& angle, Mat1f& output)
{
    std::lock_guard<std::mutex> lock(g_static_mutex);
    cvs_handle h = static_handle();
    Mat1f src = (angle.data == output.data) ? angle.clone() : angle;  // the reference is called aliased
    cvs_plane a = view(src), o = out_view(output, src.rows, src.cols);
    int rc = cvs_wrap(h, &a, &o);
    if (rc != CVS_OK) throw_status(h, rc, "cvs_wrap");
}

// --------------------------------------------------------------------------- G2
SteerableFiltersG2::SteerableFiltersG2(const Mat1f& image, int width, float spacing)
    : SteerableFilters(CVS_KIND_G2, width, spacing, 0), m_thetaValid(false), m_strengthValid(false)
{
    init(image);
}

SteerableFiltersG2::SteerableFiltersG2(const Mat1f& image, int width, float spacing, int device)
    : SteerableFilters(CVS_KIND_G2, width, spacing, device), m_thetaValid(false), m_strengthValid(false)
{
    init(image);
}

void SteerableFiltersG2::init(const Mat1f& image)
{
    int kind = 0, width = 0;
    cvs_kind(m_handle, &kind, &width, 0);
    Mat1f* taps[7] = {&m_g1, &m_g2, &m_g3, &m_h1, &m_h2, &m_h3, &m_h4};
    for (int i = 0; i < 7; ++i) *taps[i] = taps_of(m_handle, i, width);
    if (!image.empty()) setup(image);
}

void SteerableFiltersG2::setup(const Mat1f& image)
{
    m_thetaValid = m_strengthValid = false;
    cvs_plane p = view(image);
    check(cvs_setup(m_handle, &p, CVS_SETUP_FULL), "cvs_setup");
    if (memberSyncWanted(&typeid(SteerableFiltersG2))) syncMembers();
}

// SteerableFiltersG2.h:64-66 of the reference: m_g2a..m_h2d, m_c1..m_c3, m_theta, m_orientationStrength
void SteerableFiltersG2::syncMembers()
{
    Mat1f* basis[7] = {&m_g2a, &m_g2b, &m_g2c, &m_h2a, &m_h2b, &m_h2c, &m_h2d};
    for (int i = 0; i < 7; ++i) fetch(CVS_PLANE_BASIS0 + i, *basis[i]);
    fetch(CVS_PLANE_C1, m_c1);
    fetch(CVS_PLANE_C2, m_c2);
    fetch(CVS_PLANE_C3, m_c3);
    (void)getDominantOrientationAngle();
    (void)getDominantOrientationStrength();
}

const Mat1f& SteerableFiltersG2::getDominantOrientationAngle() const
{
    if (!m_thetaValid) {
        fetch(CVS_PLANE_THETA, m_theta);
        m_thetaValid = true;
    }
    return m_theta;
}

const Mat1f& SteerableFiltersG2::getDominantOrientationStrength() const
{
    if (!m_strengthValid) {
        fetch(CVS_PLANE_STRENGTH, m_orientationStrength);
        m_strengthValid = true;
    }
    return m_orientationStrength;
}

void SteerableFiltersG2::getBasis(int index, Mat1f& dst) const { fetch(CVS_PLANE_BASIS0 + index, dst); }

void SteerableFiltersG2::getCoefficients(Mat1f& c1, Mat1f& c2, Mat1f& c3) const
{
    fetch(CVS_PLANE_C1, c1);
    fetch(CVS_PLANE_C2, c2);
    fetch(CVS_PLANE_C3, c3);
}

void SteerableFiltersG2::steer(const Point& p, float theta, float& g2, float& h2)
{
    float out[5];
    check(cvs_steer_point(m_handle, p.x, p.y, theta, out), "cvs_steer_point");
    g2 = out[0];
    h2 = out[1];
}

void SteerableFiltersG2::steer(const Point& p, float theta, float& g2, float& h2, float& e, float& magnitude, float& phase)
{
    float out[5];
    check(cvs_steer_point(m_handle, p.x, p.y, theta, out), "cvs_steer_point");
    g2 = out[0];
    h2 = out[1];
    e = out[2];
    magnitude = out[3];
    phase = out[4];
}

// the callers pass getDominantOrientationAngle() straight back in (test/test.cpp:86): then the
// device-resident theta plane is used and nothing is uploaded
bool SteerableFiltersG2::isOwnTheta(const Mat1f& theta) const { return m_thetaValid && theta.data == m_theta.data; }

void SteerableFiltersG2::steer(float theta, Mat1f& g2, Mat1f& h2)
{
    int rows = 0, cols = 0;
    check(cvs_shape(m_handle, &rows, &cols), "cvs_shape");
    cvs_plane g = out_view(g2, rows, cols), h = out_view(h2, rows, cols);
    check(cvs_steer_scalar(m_handle, theta, &g, &h, 0, 0, 0), "cvs_steer_scalar");
}

void SteerableFiltersG2::steer(const Mat1f& theta, Mat1f& g2, Mat1f& h2)
{
    cvs_plane t = view(theta);
    cvs_plane g = out_view(g2, theta.rows, theta.cols), h = out_view(h2, theta.rows, theta.cols);
    check(cvs_steer_map(m_handle, isOwnTheta(theta) ? 0 : &t, &g, &h, 0, 0, 0), "cvs_steer_map");
}

void SteerableFiltersG2::steer(float theta, Mat1f& g2, Mat1f& h2, Mat1f& e, Mat1f& magnitude, Mat1f& phase)
{
    int rows = 0, cols = 0;
    check(cvs_shape(m_handle, &rows, &cols), "cvs_shape");
    cvs_plane g = out_view(g2, rows, cols), h = out_view(h2, rows, cols), pe = out_view(e, rows, cols);
    cvs_plane pm = out_view(magnitude, rows, cols), pp = out_view(phase, rows, cols);
    check(cvs_steer_scalar(m_handle, theta, &g, &h, &pe, &pm, &pp), "cvs_steer_scalar");
}

void SteerableFiltersG2::steer(const Mat1f& theta, Mat1f& g2, Mat1f& h2, Mat1f& e, Mat1f& magnitude, Mat1f& phase)
{
    cvs_plane t = view(theta);
    const int rows = theta.rows, cols = theta.cols;
    cvs_plane g = out_view(g2, rows, cols), h = out_view(h2, rows, cols), pe = out_view(e, rows, cols);
    cvs_plane pm = out_view(magnitude, rows, cols), pp = out_view(phase, rows, cols);
    check(cvs_steer_map(m_handle, isOwnTheta(theta) ? 0 : &t, &g, &h, &pe, &pm, &pp), "cvs_steer_map");
}

void SteerableFiltersG2::computeMagnitudeAndPhase(const Mat1f& g2, const Mat1f& h2, Mat1f& magnitude, Mat1f& phase)
{
    cvs_plane g = view(g2), h = view(h2);
    cvs_plane pm = out_view(magnitude, g2.rows, g2.cols), pp = out_view(phase, g2.rows, g2.cols);
    check(cvs_mag_phase(m_handle, &g, &h, &pm, &pp), "cvs_mag_phase");
}

void SteerableFiltersG2::findEdges(const Mat1f& e, const Mat1f& phase, Mat1f& output, float)
{
    cvs_plane pe = view(e), pp = view(phase), po = out_view(output, e.rows, e.cols);
    check(cvs_find(m_handle, &pe, &pp, &po, 0, 0), "cvs_find");
}

void SteerableFiltersG2::findDarkLines(const Mat1f& e, const Mat1f& phase, Mat1f& output, float)
{
    cvs_plane pe = view(e), pp = view(phase), po = out_view(output, e.rows, e.cols);
    check(cvs_find(m_handle, &pe, &pp, 0, &po, 0), "cvs_find");
}

void SteerableFiltersG2::findBrightLines(const Mat1f& e, const Mat1f& phase, Mat1f& output, float)
{
    cvs_plane pe = view(e), pp = view(phase), po = out_view(output, e.rows, e.cols);
    check(cvs_find(m_handle, &pe, &pp, 0, 0, &po), "cvs_find");
}

// extension: thin `response` to its local maxima across the object's dominant orientation -- m_theta, read where it lives on the
// device (cvs_nonmax with theta = NULL), so the lazy host copy is not needed
void SteerableFiltersG2::nonMaxSuppression(const Mat1f& response, Mat1f& output)
{
    cvs_plane pr = view(response), po = out_view(output, response.rows, response.cols);
    check(cvs_nonmax(m_handle, 0, 1, &pr, &po), "cvs_nonmax");
}

// extension: 8-connected hysteresis; 0 / 255 floats, so that the callers' convertTo(CV_8UC1) applies unchanged
void SteerableFiltersG2::hysteresis(const Mat1f& response, float low, float high, Mat1f& output)
{
    cvs_plane pr = view(response), po = out_view(output, response.rows, response.cols);
    check(cvs_hysteresis(m_handle, 1, &pr, low, high, &po, 0), "cvs_hysteresis");
}

int SteerableFiltersG2::pruneContours(const Mat1f& mask, const Mat1f& weight, int minArea, float minPeak, Mat1f& out)
{
    int n = 0;
    check(prune_contours(m_handle, mask, weight, minArea, minPeak, out, &n), "cvs_contour_prune");
    return n;
}

// extension: hysteresis and prune in one labelling; 0 / 255 floats like both
void SteerableFiltersG2::linkContours(const Mat1f& response, float low, float high, int minArea, float minPeak, Mat1f& output)
{
    cvs_plane pr = view(response), po = out_view(output, response.rows, response.cols);
    check(cvs_link(m_handle, 1, &pr, low, high, minArea, minPeak, &po, 0), "cvs_link");
}

int SteerableFiltersG2::countComponents(const Mat1f& mask)
{
    int n = 0;
    check(count_components(m_handle, mask, &n), "cvs_label");
    return n;
}

int SteerableFiltersG2::traceContours(const Mat1f& mask, std::vector<std::vector<Point> >& chains, std::vector<int>* flags)
{
    int n = 0;
    check(trace_contours(m_handle, mask, chains, flags, &n), "cvs_contour_chains");
    return n;
}

int SteerableFiltersG2::approxContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, float epsilon,
                                       std::vector<std::vector<Point> >& polylines)
{
    int n = 0;
    check(approx_contours(m_handle, chains, flags, epsilon, polylines, &n), "cvs_chain_polylines");
    return n;
}

int SteerableFiltersG2::refineContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, std::vector<std::vector<float> >& xs,
                                       std::vector<std::vector<float> >& ys, std::vector<std::vector<float> >* strength)
{
    int n = 0;
    check(refine_contours(m_handle, response, chains, xs, ys, strength, &n), "cvs_chain_refine");
    return n;
}

int SteerableFiltersG2::fitSegments(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags,
                                    float epsilon, std::vector<std::vector<float> >& lines, std::vector<std::vector<float> >* rms)
{
    int n = 0;
    check(fit_segments(m_handle, response, chains, flags, epsilon, lines, rms, &n), "cvs_polyline_segments");
    return n;
}

int SteerableFiltersG2::cornerContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags,
                                       int radius, float maxCosine, std::vector<std::vector<int> >& corners,
                                       std::vector<std::vector<float> >* cosines)
{
    int n = 0;
    check(corner_contours(m_handle, response, chains, flags, radius, maxCosine, corners, cosines, &n), "cvs_chain_turns");
    return n;
}

int SteerableFiltersG2::joinContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags,
                                     int radius, float minCosine, std::vector<int>& partners, std::vector<float>* cosines)
{
    int n = 0;
    check(join_contours(m_handle, response, chains, flags, radius, minCosine, partners, cosines, &n), "cvs_chain_joins");
    return n;
}

int SteerableFiltersG2::stitchContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, const std::vector<int>& partners,
                                       std::vector<std::vector<Point> >& paths, std::vector<int>* pathFlags, std::vector<std::vector<int> >* members)
{
    int n = 0;
    check(stitch_contours(m_handle, chains, flags, partners, paths, pathFlags, members, &n), "cvs_chain_paths");
    return n;
}

int SteerableFiltersG2::bridgeContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, int radius, int maxGap, float minCosine,
                                       std::vector<std::vector<Point> >& bridged, std::vector<int>& bridgedFlags, std::vector<int>* partners)
{
    int n = 0;
    check(bridge_contours(m_handle, chains, flags, radius, maxGap, minCosine, bridged, bridgedFlags, partners, &n), "cvs_chain_bridges");
    return n;
}

void SteerableFiltersG2::phaseWeights(const Mat1f& phase, Mat1f& lambda, float phi, bool signum, float k)
{
    std::lock_guard<std::mutex> lock(g_static_mutex);
    cvs_handle h = static_handle();
    cvs_plane pp = view(phase), pl = out_view(lambda, phase.rows, phase.cols);
    int rc = cvs_phase_weights(h, &pp, &pl, phi, signum ? 1 : 0, k);
    if (rc != CVS_OK) throw_status(h, rc, "cvs_phase_weights");
}

void SteerableFiltersG2::pipeline(const Mat1f& image, Mat1f& g2, Mat1f& h2, Mat1f& e, Mat1f& magnitude, Mat1f& phase,
                                  Mat1f& edges, Mat1f& linesDark, Mat1f& linesBright)
{
    m_thetaValid = m_strengthValid = false;
    cvs_plane pi = view(image);
    Mat1f* outs[8] = {&g2, &h2, &e, &magnitude, &phase, &edges, &linesDark, &linesBright};
    cvs_plane planes[8];
    const cvs_plane* ptrs[8];
    for (int i = 0; i < 8; ++i) {
        planes[i] = out_view(*outs[i], image.rows, image.cols);
        ptrs[i] = &planes[i];
    }
    check(cvs_pipeline(m_handle, &pi, ptrs), "cvs_pipeline");
}

// steer(thetas[k], ...) for every angle in one cvs_steer_bank call: outs[o] (g, h, e, magnitude, phase; NULL = not wanted) resized
// to one host plane per angle, allocated as the Mat1f& overloads allocate theirs
namespace {
int steer_bank_views(cvs_handle h, const std::vector<float>& thetas, std::vector<Mat1f>* const outs[5])
{
    int rows = 0, cols = 0;
    int rc = cvs_shape(h, &rows, &cols);
    if (rc != CVS_OK) return rc;
    const size_t n = thetas.size();
    std::vector<cvs_plane> planes(5 * n);
    for (int o = 0; o < 5; ++o) {
        if (!outs[o]) continue;
        outs[o]->resize(n);
        for (size_t k = 0; k < n; ++k) planes[5 * k + o] = out_view((*outs[o])[k], rows, cols);
    }
    return cvs_steer_bank(h, thetas.empty() ? 0 : thetas.data(), (int)n, planes.empty() ? 0 : planes.data());
}
}  // namespace

void SteerableFiltersG2::steer(const std::vector<float>& thetas, std::vector<Mat1f>& g2, std::vector<Mat1f>& h2)
{
    std::vector<Mat1f>* const outs[5] = {&g2, &h2, 0, 0, 0};
    check(steer_bank_views(m_handle, thetas, outs), "cvs_steer_bank");
}

void SteerableFiltersG2::steer(const std::vector<float>& thetas, std::vector<Mat1f>& g2, std::vector<Mat1f>& h2, std::vector<Mat1f>& e,
                               std::vector<Mat1f>& magnitude, std::vector<Mat1f>& phase)
{
    std::vector<Mat1f>* const outs[5] = {&g2, &h2, &e, &magnitude, &phase};
    check(steer_bank_views(m_handle, thetas, outs), "cvs_steer_bank");
}

// cvs_orientation_peaks into host planes allocated as the Mat1f& overloads allocate theirs; the count plane stays here and only its
// largest byte is returned.  Status, or that number through *n
namespace {
int orientation_peaks(cvs_handle h, std::vector<Mat1f>& angles, std::vector<Mat1f>& energies, int nAngles, int maxPeaks, float minEnergy,
                      float minRatio, float minContrast, int* n)
{
    int rows = 0, cols = 0;
    int rc = cvs_shape(h, &rows, &cols);
    if (rc != CVS_OK) return rc;
    cvs_peaks_cfg cfg;
    cfg.struct_size = (unsigned)sizeof(cfg);
    cfg.n_angles = nAngles;
    cfg.max_peaks = maxPeaks;
    cfg.min_energy = minEnergy;
    cfg.min_ratio = minRatio;
    cfg.min_contrast = minContrast;
    const size_t m = maxPeaks >= 1 && maxPeaks <= CVS_PEAKS_MAX && rows > 0 ? (size_t)maxPeaks : 0;   // (the library refuses the rest)
    std::vector<cvs_plane> pa(m), pe(m);
    angles.resize(m);
    energies.resize(m);
    for (size_t s = 0; s < m; ++s) {
        pa[s] = out_view(angles[s], rows, cols);
        pe[s] = out_view(energies[s], rows, cols);
    }
    std::vector<unsigned char> count((size_t)rows * (size_t)cols);
    cvs_plane pc;
    pc.data = reinterpret_cast<float*>(count.data());
    pc.rows = rows;
    pc.cols = cols;
    pc.step = (size_t)cols;
    pc.mem = CVS_MEM_HOST | CVS_DEPTH_U8;
    rc = cvs_orientation_peaks(h, &cfg, m ? pa.data() : 0, m ? pe.data() : 0, &pc);
    if (rc != CVS_OK) return rc;
    unsigned char most = 0;
    for (size_t i = 0; i < count.size(); ++i) most = count[i] > most ? count[i] : most;
    *n = (int)most;
    return CVS_OK;
}
}  // namespace

int SteerableFiltersG2::orientationPeaks(std::vector<Mat1f>& angles, std::vector<Mat1f>& energies, int nAngles, int maxPeaks, float minEnergy,
                                         float minRatio, float minContrast)
{
    int n = 0;
    check(orientation_peaks(m_handle, angles, energies, nAngles, maxPeaks, minEnergy, minRatio, minContrast, &n), "cvs_orientation_peaks");
    return n;
}

// --------------------------------------------------------------------------- G4
SteerableFiltersG4::SteerableFiltersG4(const Mat1f& image, int width, float spacing)
    : SteerableFilters(CVS_KIND_G4, width, spacing, 0)
{
    init(image);
}

SteerableFiltersG4::SteerableFiltersG4(const Mat1f& image, int width, float spacing, int device)
    : SteerableFilters(CVS_KIND_G4, width, spacing, device)
{
    init(image);
}

int SteerableFiltersG4::pruneContours(const Mat1f& mask, const Mat1f& weight, int minArea, float minPeak, Mat1f& out)
{
    int n = 0;
    check(prune_contours(m_handle, mask, weight, minArea, minPeak, out, &n), "cvs_contour_prune");
    return n;
}

// extension: hysteresis and prune in one labelling; 0 / 255 floats like both
void SteerableFiltersG4::linkContours(const Mat1f& response, float low, float high, int minArea, float minPeak, Mat1f& output)
{
    cvs_plane pr = view(response), po = out_view(output, response.rows, response.cols);
    check(cvs_link(m_handle, 1, &pr, low, high, minArea, minPeak, &po, 0), "cvs_link");
}

int SteerableFiltersG4::countComponents(const Mat1f& mask)
{
    int n = 0;
    check(count_components(m_handle, mask, &n), "cvs_label");
    return n;
}

int SteerableFiltersG4::traceContours(const Mat1f& mask, std::vector<std::vector<Point> >& chains, std::vector<int>* flags)
{
    int n = 0;
    check(trace_contours(m_handle, mask, chains, flags, &n), "cvs_contour_chains");
    return n;
}

int SteerableFiltersG4::approxContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, float epsilon,
                                       std::vector<std::vector<Point> >& polylines)
{
    int n = 0;
    check(approx_contours(m_handle, chains, flags, epsilon, polylines, &n), "cvs_chain_polylines");
    return n;
}

int SteerableFiltersG4::refineContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, std::vector<std::vector<float> >& xs,
                                       std::vector<std::vector<float> >& ys, std::vector<std::vector<float> >* strength)
{
    int n = 0;
    check(refine_contours(m_handle, response, chains, xs, ys, strength, &n), "cvs_chain_refine");
    return n;
}

int SteerableFiltersG4::fitSegments(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags,
                                    float epsilon, std::vector<std::vector<float> >& lines, std::vector<std::vector<float> >* rms)
{
    int n = 0;
    check(fit_segments(m_handle, response, chains, flags, epsilon, lines, rms, &n), "cvs_polyline_segments");
    return n;
}

int SteerableFiltersG4::cornerContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags,
                                       int radius, float maxCosine, std::vector<std::vector<int> >& corners,
                                       std::vector<std::vector<float> >* cosines)
{
    int n = 0;
    check(corner_contours(m_handle, response, chains, flags, radius, maxCosine, corners, cosines, &n), "cvs_chain_turns");
    return n;
}

int SteerableFiltersG4::joinContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags,
                                     int radius, float minCosine, std::vector<int>& partners, std::vector<float>* cosines)
{
    int n = 0;
    check(join_contours(m_handle, response, chains, flags, radius, minCosine, partners, cosines, &n), "cvs_chain_joins");
    return n;
}

int SteerableFiltersG4::stitchContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, const std::vector<int>& partners,
                                       std::vector<std::vector<Point> >& paths, std::vector<int>* pathFlags, std::vector<std::vector<int> >* members)
{
    int n = 0;
    check(stitch_contours(m_handle, chains, flags, partners, paths, pathFlags, members, &n), "cvs_chain_paths");
    return n;
}

int SteerableFiltersG4::bridgeContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, int radius, int maxGap, float minCosine,
                                       std::vector<std::vector<Point> >& bridged, std::vector<int>& bridgedFlags, std::vector<int>* partners)
{
    int n = 0;
    check(bridge_contours(m_handle, chains, flags, radius, maxGap, minCosine, bridged, bridgedFlags, partners, &n), "cvs_chain_bridges");
    return n;
}

void SteerableFiltersG4::init(const Mat1f& image)
{
    int kind = 0, width = 0;
    cvs_kind(m_handle, &kind, &width, 0);
    Mat1f* taps[11] = {&m_g1, &m_g2, &m_g3, &m_g4, &m_g5, &m_h1, &m_h2, &m_h3, &m_h4, &m_h5, &m_h6};
    for (int i = 0; i < 11; ++i) *taps[i] = taps_of(m_handle, i, width);
    if (!image.empty()) setup(image);
}

void SteerableFiltersG4::setup(const Mat1f& image)
{
    cvs_plane p = view(image);
    check(cvs_setup(m_handle, &p, CVS_SETUP_BASIS), "cvs_setup");
    if (memberSyncWanted(&typeid(SteerableFiltersG4))) syncMembers();
}

// SteerableFiltersG4.h:53-54 of the reference: m_g4a..m_g4e, m_h4a..m_h4f
void SteerableFiltersG4::syncMembers()
{
    Mat1f* basis[11] = {&m_g4a, &m_g4b, &m_g4c, &m_g4d, &m_g4e, &m_h4a, &m_h4b, &m_h4c, &m_h4d, &m_h4e, &m_h4f};
    for (int i = 0; i < 11; ++i) fetch(CVS_PLANE_BASIS0 + i, *basis[i]);
}

void SteerableFiltersG4::steer(const Mat1f& theta, Mat1f& g4, Mat1f& h4)
{
    cvs_plane t = view(theta);
    cvs_plane g = out_view(g4, theta.rows, theta.cols), h = out_view(h4, theta.rows, theta.cols);
    check(cvs_steer_map(m_handle, &t, &g, &h, 0, 0, 0), "cvs_steer_map");
}

void SteerableFiltersG4::steer(float theta, Mat1f& g4, Mat1f& h4)
{
    int rows = 0, cols = 0;
    check(cvs_shape(m_handle, &rows, &cols), "cvs_shape");
    cvs_plane g = out_view(g4, rows, cols), h = out_view(h4, rows, cols);
    check(cvs_steer_scalar(m_handle, theta, &g, &h, 0, 0, 0), "cvs_steer_scalar");
}

// G4.cpp:88-90: empty body in the reference; outputs are left untouched
void SteerableFiltersG4::steer(const std::vector<float>& thetas, std::vector<Mat1f>& g4, std::vector<Mat1f>& h4)
{
    std::vector<Mat1f>* const outs[5] = {&g4, &h4, 0, 0, 0};
    check(steer_bank_views(m_handle, thetas, outs), "cvs_steer_bank");
}

int SteerableFiltersG4::orientationPeaks(std::vector<Mat1f>& angles, std::vector<Mat1f>& energies, int nAngles, int maxPeaks, float minEnergy,
                                         float minRatio, float minContrast)
{
    int n = 0;
    check(orientation_peaks(m_handle, angles, energies, nAngles, maxPeaks, minEnergy, minRatio, minContrast, &n), "cvs_orientation_peaks");
    return n;
}

void SteerableFiltersG4::computeMagnitudeAndPhase(const Mat1f&, const Mat1f&, Mat1f&, Mat1f&) {}

void SteerableFiltersG4::getBasis(int index, Mat1f& dst) const { fetch(CVS_PLANE_BASIS0 + index, dst); }

}  // namespace fa
