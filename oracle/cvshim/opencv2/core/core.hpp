// oracle/cvshim/opencv2/core/core.hpp -- a stand-in for the slice of OpenCV that the reference's three source files use
// (TEST INFRASTRUCTURE ONLY; this is NOT OpenCV and holds no OpenCV text).
//
// oracle/ref_run.mk puts this directory on the include path so that the reference's SteerableFilters.cpp,
// SteerableFiltersG2.cpp and SteerableFiltersG4.cpp compile unchanged, where they lie, and run: what their author wrote --
// tap tables, the pairing of taps with basis planes, every sign and coefficient, the gates, the call order -- then executes
// as written, and the planes it writes are committed as data (tests/golden/ref_run/).
//
// RECALLED, not pinned (see DESIGN.md "Oracle and parity"): the semantics given to the cv:: names here are our reading of
// OpenCV 3.4 for CV_32F, the same reading cvsteer_oracle.h records:
//   * every matrix operator is EAGER: one operator = one float32 plane, each element rounded once (OpenCV's MatExpr folds
//     some of these into one call, e.g. alpha * (a + b) into addWeighted; the eager form adds in another order and lands
//     within one ulp of it);
//   * a double scalar is narrowed to float before use, in arithmetic and in Mat > scalar;
//   * sepFilter2D, cartToPolar and polarToCart (imgproc.hpp) are the oracle's own C primitives;
//   * Mat assignment and copy share storage, clone() copies.
#ifndef CVSTEER_CVSHIM_CORE_HPP
#define CVSTEER_CVSHIM_CORE_HPP

#include <cmath>
#include <cstddef>
#include <memory>
#include <vector>

#define CV_32FC1 5

namespace cv {

struct Point {
    int x, y;
    Point() : x(0), y(0) {}
    Point(int x_, int y_) : x(x_), y(y_) {}
};

// cv::Mat() -- only ever passed as the empty magnitude of polarToCart
struct Mat {};

typedef std::vector<unsigned char> Mask;

class Mat1f {
public:
    int rows, cols;
    Mat1f() : rows(0), cols(0) {}
    Mat1f(int r, int c) : rows(r), cols(c), d_(new float[(size_t)r * c](), std::default_delete<float[]>()) {}

    bool empty() const { return !d_ || rows == 0 || cols == 0; }
    size_t total() const { return (size_t)rows * cols; }
    float* ptr() { return d_.get(); }
    const float* ptr() const { return d_.get(); }
    float& operator()(int i) { return d_.get()[i]; }
    const float& operator()(int i) const { return d_.get()[i]; }
    float& operator()(int r, int c) { return d_.get()[(size_t)r * cols + c]; }
    const float& operator()(int r, int c) const { return d_.get()[(size_t)r * cols + c]; }
    float& operator()(const Point& p) { return (*this)(p.y, p.x); }
    const float& operator()(const Point& p) const { return (*this)(p.y, p.x); }

    Mat1f clone() const
    {
        Mat1f m(rows, cols);
        for (size_t i = 0; i < total(); ++i) m(int(i)) = (*this)(int(i));
        return m;
    }
    Mat1f t() const
    {
        Mat1f m(cols, rows);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) m(c, r) = (*this)(r, c);
        return m;
    }
    Mat1f mul(const Mat1f& o) const
    {
        Mat1f m(rows, cols);
        for (size_t i = 0; i < total(); ++i) m(int(i)) = (*this)(int(i)) * o(int(i));
        return m;
    }
    void copyTo(Mat1f& dst, const Mask& mask) const
    {
        for (size_t i = 0; i < total(); ++i)
            if (mask[i]) dst(int(i)) = (*this)(int(i));
    }
    void setTo(double v, const Mask& mask)
    {
        for (size_t i = 0; i < total(); ++i)
            if (mask[i]) (*this)(int(i)) = float(v);
    }
    Mat1f& operator*=(double s)
    {
        const float f = float(s);
        for (size_t i = 0; i < total(); ++i) (*this)(int(i)) = (*this)(int(i)) * f;
        return *this;
    }

private:
    std::shared_ptr<float> d_;
};

namespace shim {
template <class F>
inline Mat1f map1(const Mat1f& a, F f)
{
    Mat1f m(a.rows, a.cols);
    for (size_t i = 0; i < a.total(); ++i) m(int(i)) = f(a(int(i)));
    return m;
}
template <class F>
inline Mat1f map2(const Mat1f& a, const Mat1f& b, F f)
{
    Mat1f m(a.rows, a.cols);
    for (size_t i = 0; i < a.total(); ++i) m(int(i)) = f(a(int(i)), b(int(i)));
    return m;
}
}  // namespace shim

inline Mat1f operator+(const Mat1f& a, const Mat1f& b) { return shim::map2(a, b, [](float x, float y) { return x + y; }); }
inline Mat1f operator-(const Mat1f& a, const Mat1f& b) { return shim::map2(a, b, [](float x, float y) { return x - y; }); }
inline Mat1f operator-(const Mat1f& a) { return shim::map1(a, [](float x) { return -x; }); }
inline Mat1f operator*(double s, const Mat1f& a) { const float f = float(s); return shim::map1(a, [f](float x) { return f * x; }); }
inline Mat1f operator*(const Mat1f& a, double s) { const float f = float(s); return shim::map1(a, [f](float x) { return x * f; }); }
inline Mat1f operator-(double s, const Mat1f& a) { const float f = float(s); return shim::map1(a, [f](float x) { return f - x; }); }
inline Mat1f operator-(const Mat1f& a, double s) { const float f = float(s); return shim::map1(a, [f](float x) { return x - f; }); }
inline Mask operator>(const Mat1f& a, double s)
{
    const float f = float(s);
    Mask m(a.total());
    for (size_t i = 0; i < a.total(); ++i) m[i] = a(int(i)) > f ? 255 : 0;
    return m;
}

inline Mat1f abs(const Mat1f& a) { return shim::map1(a, [](float x) { return std::fabs(x); }); }
// cv::min on floats: a < b ? a : b (the second operand where either is NaN)
inline Mat1f min(const Mat1f& a, const Mat1f& b) { return shim::map2(a, b, [](float x, float y) { return x < y ? x : y; }); }
inline void patchNaNs(Mat1f& a, double v = 0)
{
    for (size_t i = 0; i < a.total(); ++i)
        if (a(int(i)) != a(int(i))) a(int(i)) = float(v);
}

}  // namespace cv

// the facade's own headers name these types fa::Mat1f / fa::Point (include/cvsteer/Mat.h does the same over real OpenCV), so one
// driver source (tests/cpp/ref_sequence.cpp) builds against either
namespace fa {
typedef cv::Mat1f Mat1f;
typedef cv::Point Point;
}

#endif
