// Pillow's 8-bit resampling tables (ImagingResample: precompute_coeffs + normalize_coeffs_8bpc), host only.
// Plain C++ (no HIP): the expression order below is Pillow's, and the file is built without fast-math and without
// contraction (build.py PER_FILE) so that libm's sin and every division round as they do there.  With these
// tables the resize itself is integer arithmetic (csrc/resample.hip, tests/resample_ref.py).
#include <cmath>
#include <exception>
#include <string>
#include <vector>

#include "../../include/irx.h"

namespace irx {
void set_error(const std::string& msg);   // capi.cpp
}

namespace {

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return std::sin(x) / x;
}

double lanczos_filter(double x) {
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

const int PRECISION_BITS = 32 - 8 - 2;

int fail(const std::string& msg) {
  irx::set_error("irx_resample_coeffs: " + msg);
  return -1;
}

}  // namespace

extern "C" int irx_resample_coeffs(int in_size, int out_size, int filter, int* bounds, int* coeffs, int cap,
                                   int* ksize_out) {
  try {
    if (!ksize_out) return fail("null ksize pointer");
    if (in_size < 1 || out_size < 1) return fail("sizes must be >= 1");
    if (filter != IRX_RESAMPLE_LANCZOS && filter != IRX_RESAMPLE_BICUBIC)
      return fail("unknown filter " + std::to_string(filter));
    if ((bounds == nullptr) != (coeffs == nullptr)) return fail("bounds and coeffs: both tables or neither");
    double (*const f)(double) = filter == IRX_RESAMPLE_LANCZOS ? lanczos_filter : bicubic_filter;
    const double base_support = filter == IRX_RESAMPLE_LANCZOS ? 3.0 : 2.0;

    double filterscale, scale;
    filterscale = scale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = base_support * filterscale;
    const long ksize_l = (long)std::ceil(support) * 2 + 1;
    if (ksize_l > 0x7fffffffL / 4) return fail("kernel size overflows");
    const int ksize = (int)ksize_l;
    *ksize_out = ksize;
    if (!coeffs) return 0;                      // sizes only
    if ((long)cap < (long)out_size * ksize) return fail("coefficient table capacity too small");

    std::vector<double> row((size_t)ksize);     // one output index's weights before the fixed-point step
    double* k = row.data();
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
      const double center = (xx + 0.5) * scale;
      double ww = 0.0;
      int xmin = (int)(center - support + 0.5);
      if (xmin < 0) xmin = 0;
      int xmax = (int)(center + support + 0.5);
      if (xmax > in_size) xmax = in_size;
      xmax -= xmin;
      int x;
      for (x = 0; x < xmax; ++x) {
        const double w = f((x + xmin - center + 0.5) * ss);
        k[x] = w;
        ww += w;
      }
      for (x = 0; x < xmax; ++x)
        if (ww != 0.0) k[x] /= ww;
      for (; x < ksize; ++x) k[x] = 0;
      bounds[xx * 2 + 0] = xmin;
      bounds[xx * 2 + 1] = xmax;
      int* kk = coeffs + (size_t)xx * ksize;
      for (x = 0; x < ksize; ++x)
        kk[x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << PRECISION_BITS));
    }
    return 0;
  } catch (const std::exception& e) {
    return fail(e.what());
  }
}
