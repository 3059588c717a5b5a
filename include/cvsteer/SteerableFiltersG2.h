// cvsteer/SteerableFiltersG2.h -- G2/H2 quadrature pair, facade over libcvsteer_hip.so.
// Public surface = reference cvsteer/SteerableFiltersG2.h:38-60, same names, same default
// arguments (width = 4, spacing = 0.67, k = 2.0), same overload set.  Each method states the
// reference lines it replaces; the arithmetic runs in HIP kernels on the MI355X.
#ifndef CVSTEER_AMD_STEERABLEFILTERSG2_H
#define CVSTEER_AMD_STEERABLEFILTERSG2_H

#include <cvsteer/SteerableFilters.h>

#include <vector>

namespace fa {

class SteerableFiltersG2 : public SteerableFilters {
public:
    // G2.cpp:44-58: build the 7 tap vectors, then setup(image)
    SteerableFiltersG2(const Mat1f& image, int width = 4, float spacing = 0.67f);
    // addition: choose the HIP device; image may be empty (call setup later)
    SteerableFiltersG2(const Mat1f& image, int width, float spacing, int device);

    // G2.h:40-41.  References stay valid until the next setup(); filled on first use.
    const Mat1f& getDominantOrientationAngle() const;
    const Mat1f& getDominantOrientationStrength() const;

    void setup(const Mat1f& image);  // G2.cpp:60-100

    // Steer filters at single point (G2.cpp:115-134); p.x = column, p.y = row
    void steer(const Point& p, float theta, float& g2, float& h2);
    void steer(const Point& p, float theta, float& g2, float& h2, float& e, float& magnitude, float& phase);
    void steer(const Mat1f& theta, Mat1f& g2, Mat1f& h2);  // G2.cpp:147-155

    // Processing on entire images
    void steer(float theta, Mat1f& g2, Mat1f& h2);  // G2.cpp:137-145
    void steer(float theta, Mat1f& g2, Mat1f& h2, Mat1f& e, Mat1f& magnitude, Mat1f& phase);          // G2.cpp:157-165
    void steer(const Mat1f& theta, Mat1f& g2, Mat1f& h2, Mat1f& e, Mat1f& magnitude, Mat1f& phase);   // G2.cpp:167-177
    void computeMagnitudeAndPhase(const Mat1f& g2, const Mat1f& h2, Mat1f& magnitude, Mat1f& phase);  // G2.cpp:107-112

    void findEdges(const Mat1f& e, const Mat1f& phase, Mat1f& output, float k = 2.0f);        // G2.cpp:201-204
    void findDarkLines(const Mat1f& e, const Mat1f& phase, Mat1f& output, float k = 2.0f);    // G2.cpp:205-208
    void findBrightLines(const Mat1f& e, const Mat1f& phase, Mat1f& output, float k = 2.0f);  // G2.cpp:209-212

    static void phaseWeights(const Mat1f& phase, Mat1f& lambda, float phi, bool signum, float k);  // G2.cpp:179-186

    // -- additions of this build --
    // the reference's protected basis planes m_g2a..m_h2d (index 0..6) and m_c1..m_c3
    void getBasis(int index, Mat1f& dst) const;
    void getCoefficients(Mat1f& c1, Mat1f& c2, Mat1f& c3) const;
    // the callers' whole sequence (test/test.cpp:85-90) in two kernel launches
    void pipeline(const Mat1f& image, Mat1f& g2, Mat1f& h2, Mat1f& e, Mat1f& magnitude, Mat1f& phase,
                  Mat1f& edges, Mat1f& linesDark, Mat1f& linesBright);
    // steer(thetas[k], g2[k], h2[k][, e[k], magnitude[k], phase[k]]) for every angle from one read of the basis planes
    // (cvs_steer_bank): the vectors are resized to thetas.size(), each plane allocated like the Mat1f& overloads'
    void steer(const std::vector<float>& thetas, std::vector<Mat1f>& g2, std::vector<Mat1f>& h2);
    void steer(const std::vector<float>& thetas, std::vector<Mat1f>& g2, std::vector<Mat1f>& h2, std::vector<Mat1f>& e,
               std::vector<Mat1f>& magnitude, std::vector<Mat1f>& phase);
    // orientation peaks (extension, cvs_orientation_peaks): every local orientation of each pixel from one read of the basis planes --
    // the oriented energy at nAngles angles, its circular local maxima refined, the maxPeaks strongest kept.  angles / energies are
    // resized to maxPeaks planes, slot 0 the strongest; slots a pixel does not fill hold angle -1 and energy 0.  A ridge of direction
    // phi peaks at phi + pi/2 (mod pi).  Returns the largest number of peaks any pixel has.
    int orientationPeaks(std::vector<Mat1f>& angles, std::vector<Mat1f>& energies, int nAngles = 16, int maxPeaks = 2, float minEnergy = 0.f,
                         float minRatio = 0.25f, float minContrast = 1e-3f);
    // contour thinning (extension): non-maximum suppression of `response` across the dominant orientation m_theta (cvs_nonmax), and
    // 8-connected hysteresis with output 0 / 255 as floats (cvs_hysteresis) -- the callers' convertTo(CV_8UC1) applies unchanged
    void nonMaxSuppression(const Mat1f& response, Mat1f& output);
    void hysteresis(const Mat1f& response, float low, float high, Mat1f& output);
    // contour components (extension): keep the 8-connected components of `mask` (foreground: > 0) with at least minArea pixels and -- unless
    // `weight` is empty -- a largest weight >= minPeak, as 0 / 255 floats (cvs_contour_prune); returns the number kept.  countComponents:
    // the number of 8-connected components (cvs_label)
    int pruneContours(const Mat1f& mask, const Mat1f& weight, int minArea, float minPeak, Mat1f& out);
    // the two in one labelling (extension, cvs_link): hysteresis(response, low, high) followed by pruneContours(that, response, minArea,
    // minPeak), bit for bit, as 0 / 255 floats; minPeak = -INFINITY: no peak test
    void linkContours(const Mat1f& response, float low, float high, int minArea, float minPeak, Mat1f& output);
    int countComponents(const Mat1f& mask);
    // contour chains (extension, cvs_contour_chains): the linked contours of `mask` as ordered chains of pixels (x = column, y = row), cut
    // at junctions and free ends, in the canonical order of include/cvsteer_hip.h; flags (optional): CVS_CHAIN_* per chain.  Returns the
    // number of chains
    int traceContours(const Mat1f& mask, std::vector<std::vector<Point> >& chains, std::vector<int>* flags = 0);
    // contour polylines (extension, cvs_chain_polylines): Ramer-Douglas-Peucker simplification of all chains at once with tolerance
    // `epsilon` (pixels), by the split rule of include/cvsteer_hip.h; flags: what traceContours returned (a chain with CVS_CHAIN_CLOSED is
    // treated as a cycle), 0 = all chains open.  polylines[c] = the kept points of chains[c] in order.  Returns the number of vertices
    int approxContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, float epsilon,
                       std::vector<std::vector<Point> >& polylines);
    // contour edgels (extension, cvs_chain_refine): the sub-pixel position (xs[c][k], ys[c][k]) of point k of chains[c], and optionally its
    // strength there, from `response` -- the UN-THINNED map the contours were found in (what nonMaxSuppression was given, not what it
    // returned) -- across the dominant orientation m_theta, by the contract of include/cvsteer_hip.h.  A point outside the image throws.
    // Returns the number of points
    int refineContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, std::vector<std::vector<float> >& xs,
                       std::vector<std::vector<float> >& ys, std::vector<std::vector<float> >* strength = 0);
    // contour segments (extension, cvs_polyline_segments): the straight segments of the chains to sub-pixel accuracy -- approxContours
    // with tolerance `epsilon`, refineContours on `response`, and the total-least-squares line through the refined points of every polyline
    // span, by the contract of include/cvsteer_hip.h.  lines[c] = four floats x0 y0 x1 y1 per span of chains[c] that is not degenerate, in
    // span order (narrowed from double); rms (optional): rms[c] = one float per such span, its RMS distance from the line.  flags as in
    // approxContours.  Returns the number of segments
    int fitSegments(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, float epsilon,
                    std::vector<std::vector<float> >& lines, std::vector<std::vector<float> >* rms = 0);
    // contour turns (extension, cvs_chain_turns): the corners of the chains -- refineContours on `response`, then the turn of the contour
    // at every point between the centroids of the `radius` points before and after it, by the contract of include/cvsteer_hip.h with
    // min_arm = nms = radius and max_cos = maxCosine.  corners[c] = the offsets into chains[c] of its corners, ascending; cosines
    // (optional): cosines[c] = the cosine of the turn at each of them.  flags as in approxContours.  Returns the number of corners
    int cornerContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, int radius,
                       float maxCosine, std::vector<std::vector<int> >& corners, std::vector<std::vector<float> >* cosines = 0);
    // contour joins (extension, cvs_chain_joins): which chains continue each other through a junction -- refineContours on `response`,
    // then the joins of the chain ends by the contract of include/cvsteer_hip.h with min_arm = min(3, radius) and min_cos = minCosine.
    // partners[2c] / partners[2c + 1] = the chain end (2 * chain + side, side 0 the head, 1 the tail) that the head / the tail of chains[c]
    // continues into where the join is MUTUAL, else -1; cosines (optional): the cosine of the turn there, NaN where partners is -1.
    // flags as in approxContours.  Returns the number of mutual joins, each pair of ends counted once
    int joinContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, int radius,
                     float minCosine, std::vector<int>& partners, std::vector<float>* cosines = 0);
    // contour paths (extension, cvs_chain_paths): the chains stitched into whole contours over the mutual joins -- chains, flags and
    // `partners` as joinContours took and returned them (2 entries per chain; -1: no mutual join).  paths[p] = the points of path p: its
    // chains in walk order, a chain entered through its tail listed backwards, the junction pixel between two chains listed once, and a
    // path that closes on itself without its first pixel repeated; pathFlags (optional): CVS_CHAIN_CLOSED for such a cycle or a closed
    // chain, else the junction bits of the path's two ends; members (optional): members[p] = 2 * chain + reversed for every chain of path
    // p, in walk order.  Paths are ordered by the contract of include/cvsteer_hip.h.  Returns the number of paths
    int stitchContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, const std::vector<int>& partners,
                       std::vector<std::vector<Point> >& paths, std::vector<int>* pathFlags = 0, std::vector<std::vector<int> >* members = 0);
    // contour bridges (extension, cvs_chain_bridges): the gaps between free chain ends that face each other, closed -- chains and flags as
    // traceContours or stitchContours gave them, on their integer points, by the contract of include/cvsteer_hip.h with min_arm =
    // min(3, radius): two free ends whose pixels are 2 .. maxGap apart, each pointing at the other within minCosine and each the other's
    // nearest such end, get a bridge, a digital line from the one end pixel to the other.  bridged = the chains followed by the bridges,
    // bridgedFlags their flags (a bridged end reads as a junction); partners (optional): 2 entries per bridged chain as joinContours
    // returns them, naming for every bridged end the bridge end that continues it and the reverse, -1 elsewhere -- so
    // stitchContours(bridged, &bridgedFlags, partners, paths) puts the dashes of a line together.  Returns the number of bridges
    int bridgeContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, int radius, int maxGap, float minCosine,
                       std::vector<std::vector<Point> >& bridged, std::vector<int>& bridgedFlags, std::vector<int>* partners = 0);

protected:
    // the reference's protected members, same names (SteerableFiltersG2.h:62-66).  m_g1..m_h4 are the 7 tap vectors; the
    // planes m_g2a..m_h2d, m_c1..m_c3 are host copies of the GPU state, filled for subclasses (see SteerableFilters.h:
    // after setup() on a subclass object, or by syncMembers()); m_dx / m_dy are declared and never used, as in the reference
    Mat1f m_dx, m_dy;
    Mat1f m_g1, m_g2, m_g3, m_h1, m_h2, m_h3, m_h4;
    Mat1f m_g2a, m_g2b, m_g2c, m_h2a, m_h2b, m_h2c, m_h2d;
    Mat1f m_c1, m_c2, m_c3;
    mutable Mat1f m_theta, m_orientationStrength;    // host copies, fetched lazily by the getters
    mutable bool m_thetaValid, m_strengthValid;
    void syncMembers();  // download m_g2a..m_h2d, m_c1..m_c3, m_theta, m_orientationStrength now

private:
    void init(const Mat1f& image);
    bool isOwnTheta(const Mat1f& theta) const;
};

}  // namespace fa

#endif
