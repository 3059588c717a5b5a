// cvsteer/SteerableFiltersG4.h -- G4/H4 quadrature pair, facade over libcvsteer_hip.so.
// Public surface = reference cvsteer/SteerableFiltersG4.h:38-48 (defaults width = 6,
// spacing = 0.5).  Like the reference: setup() builds the 11 basis planes only, steer() has the
// scalar and the per-pixel overloads, computeMagnitudeAndPhase() is an empty body
// (G4.cpp:88-90) and the two getters return Mats that are never filled (G4.h:40-41,55).
#ifndef CVSTEER_AMD_STEERABLEFILTERSG4_H
#define CVSTEER_AMD_STEERABLEFILTERSG4_H

#include <cvsteer/SteerableFilters.h>

#include <vector>

namespace fa {

class SteerableFiltersG4 : public SteerableFilters {
public:
    SteerableFiltersG4(const Mat1f& image, int width = 6, float spacing = 0.5f);  // G4.cpp:47-65
    SteerableFiltersG4(const Mat1f& image, int width, float spacing, int device);

    const Mat1f& getDominantOrientationAngle() const { return m_theta; }
    const Mat1f& getDominantOrientationStrength() const { return m_orientationStrength; }

    void setup(const Mat1f& image);  // G4.cpp:67-81

    void steer(const Mat1f& theta, Mat1f& g4, Mat1f& h4);  // G4.cpp:92-112
    void steer(float theta, Mat1f& g4, Mat1f& h4);         // G4.cpp:114-122
    void computeMagnitudeAndPhase(const Mat1f& g4, const Mat1f& h4, Mat1f& magnitude, Mat1f& phase);  // G4.cpp:88-90: no-op

    // addition: the reference's protected basis planes m_g4a..m_h4f (index 0..10)
    void getBasis(int index, Mat1f& dst) const;
    // addition: steer(thetas[k], g4[k], h4[k]) for every angle from one read of the basis planes (cvs_steer_bank)
    void steer(const std::vector<float>& thetas, std::vector<Mat1f>& g4, std::vector<Mat1f>& h4);
    // addition: orientation peaks, as in SteerableFiltersG2 (cvs_orientation_peaks): the G4 / H4 pair separates arms the G2 / H2 pair blurs
    int orientationPeaks(std::vector<Mat1f>& angles, std::vector<Mat1f>& energies, int nAngles = 16, int maxPeaks = 2, float minEnergy = 0.f,
                         float minRatio = 0.25f, float minContrast = 1e-3f);
    // addition: contour components, as in SteerableFiltersG2 (cvs_contour_prune / cvs_label; they read the planes passed, not the object's state)
    int pruneContours(const Mat1f& mask, const Mat1f& weight, int minArea, float minPeak, Mat1f& out);
    // addition: hysteresis and pruneContours(that, response, ...) in one labelling, as in SteerableFiltersG2 (cvs_link)
    void linkContours(const Mat1f& response, float low, float high, int minArea, float minPeak, Mat1f& output);
    int countComponents(const Mat1f& mask);
    // addition: ordered contour chains, as in SteerableFiltersG2 (cvs_contour_chains)
    int traceContours(const Mat1f& mask, std::vector<std::vector<Point> >& chains, std::vector<int>* flags = 0);
    // addition: polylines of the chains, as in SteerableFiltersG2 (cvs_chain_polylines)
    int approxContours(const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, float epsilon,
                       std::vector<std::vector<Point> >& polylines);
    // addition: sub-pixel chain points, as in SteerableFiltersG2 (cvs_chain_refine on the object's own theta: it throws where the object has
    // no orientation state)
    int refineContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, std::vector<std::vector<float> >& xs,
                       std::vector<std::vector<float> >& ys, std::vector<std::vector<float> >* strength = 0);
    // addition: sub-pixel line fits of the polyline spans, as in SteerableFiltersG2 (cvs_polyline_segments; it refines on the object's own
    // theta and throws where the object has no orientation state)
    int fitSegments(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, float epsilon,
                    std::vector<std::vector<float> >& lines, std::vector<std::vector<float> >* rms = 0);
    // addition: the corners of the chains, as in SteerableFiltersG2 (cvs_chain_turns; it refines on the object's own theta and throws where
    // the object has no orientation state)
    int cornerContours(const Mat1f& response, const std::vector<std::vector<Point> >& chains, const std::vector<int>* flags, int radius,
                       float maxCosine, std::vector<std::vector<int> >& corners, std::vector<std::vector<float> >* cosines = 0);
    // addition: the joins of the chain ends, as in SteerableFiltersG2 (cvs_chain_joins; it refines on the object's own theta and throws
    // where the object has no orientation state)
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
    // the reference's protected members, same names (SteerableFiltersG4.h:50-56): 11 tap vectors; the planes m_g4a..m_h4f
    // are host copies of the GPU state, filled for subclasses (see SteerableFilters.h); m_c1..m_c3, m_theta and
    // m_orientationStrength are declared and never assigned, as in the reference
    Mat1f m_g1, m_g2, m_g3, m_g4, m_g5;
    Mat1f m_h1, m_h2, m_h3, m_h4, m_h5, m_h6;
    Mat1f m_g4a, m_g4b, m_g4c, m_g4d, m_g4e;
    Mat1f m_h4a, m_h4b, m_h4c, m_h4d, m_h4e, m_h4f;
    Mat1f m_c1, m_c2, m_c3, m_theta, m_orientationStrength;
    void syncMembers();  // download m_g4a..m_h4f now

private:
    void init(const Mat1f& image);
};

}  // namespace fa

#endif
