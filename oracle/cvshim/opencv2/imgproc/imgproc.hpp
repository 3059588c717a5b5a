// oracle/cvshim/opencv2/imgproc/imgproc.hpp -- stand-in (TEST INFRASTRUCTURE ONLY, not OpenCV; see core/core.hpp).
// The three primitives the reference calls are the oracle's own C restatements (cvsteer_oracle.h), so they stay RECALLED:
//   sepFilter2D  -> ora_sepfilter2d_f32  (correlation, centre anchor, BORDER_REFLECT_101, f32 row buffer)
//   cartToPolar  -> ora_cart_to_polar    (radians, the compatible arctangent polynomial)
//   polarToCart  -> ora_polar_to_cart    (empty magnitude: c = cos(a), s = sin(a))
#ifndef CVSTEER_CVSHIM_IMGPROC_HPP
#define CVSTEER_CVSHIM_IMGPROC_HPP

#include <opencv2/core/core.hpp>

#include "cvsteer_oracle.h"

namespace cv {

// kx is 1 x n, ky is n x 1 (the reference passes a transposed row); both hold 2 * width + 1 taps
inline void sepFilter2D(const Mat1f& src, Mat1f& dst, int /*ddepth*/, const Mat1f& kx, const Mat1f& ky)
{
    Mat1f out(src.rows, src.cols);
    ora_sepfilter2d_f32(src.ptr(), src.rows, src.cols, (size_t)src.cols, kx.ptr(), ky.ptr(), int(kx.total() - 1) / 2, out.ptr());
    dst = out;
}

inline void cartToPolar(const Mat1f& x, const Mat1f& y, Mat1f& magnitude, Mat1f& angle)
{
    Mat1f m(x.rows, x.cols), a(x.rows, x.cols);
    ora_cart_to_polar(x.ptr(), y.ptr(), x.total(), m.ptr(), a.ptr(), ORA_ATAN_CV);
    magnitude = m;
    angle = a;
}

inline void polarToCart(const Mat&, const Mat1f& angle, Mat1f& x, Mat1f& y)
{
    Mat1f c(angle.rows, angle.cols), s(angle.rows, angle.cols);
    ora_polar_to_cart(angle.ptr(), angle.total(), c.ptr(), s.ptr());
    x = c;
    y = s;
}

}  // namespace cv

#endif
