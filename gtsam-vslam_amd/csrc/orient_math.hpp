// Float math of k_orient_desc (extract_kernels.hip) in a header that needs no HIP: the fastAtan2 polynomial of the
// keypoint angle and the cos / sin of the rotated BRIEF pattern.  The kernel includes it for the device; a host compiler
// can include it as well (tests/native/orient_census.cpp walks every float angle through it).  Both sides must be built
// with -ffp-contract=off: float expressions round exactly as written.  On the host fma() and rint() of libm are
// correctly rounded, so a host evaluation equals the device's bit for bit.
#pragma once
#include <cmath>
#include <cfloat>

#if defined(__HIPCC__)
#define VS_OM_HD __host__ __device__ __forceinline__
#else
#define VS_OM_HD inline
#endif

namespace vslam {

VS_OM_HD float fast_atan2_deg(float y, float x) {
    const float scale = (float)(180 / 3.1415926535897932384626433832795);
    const float p1 = 0.9997878412794807f * scale;
    const float p3 = -0.3258083974640975f * scale;
    const float p5 = 0.1555786518463281f * scale;
    const float p7 = -0.04432655554792128f * scale;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// float(cos(double(x))), float(sin(double(x))) for x in [0, ~2 pi]: Cody-Waite reduction by pi/2 (k <= 4, so k * pio2_1
// is exact and the difference is exact) and the fdlibm kernel polynomials (< 1 ulp in double).  Replaces the library
// cos() + sin() calls (two separate range reductions, ~4x the instructions); wave-uniform work.
VS_OM_HD void sincos_deg_range(float xf, float& s_out, float& c_out) {
    const double x = (double)xf;
    const double kd = rint(x * 6.36619772367581382433e-01);
    const int k = (int)kd;
    double r = fma(-kd, 1.57079632673412561417e+00, x);
    r = fma(-kd, 6.07710050650619224932e-11, r);
    const double z = r * r;
    double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = fma(z, ps, 2.75573137070700676789e-06);
    ps = fma(z, ps, -1.98412698298579493134e-04);
    ps = fma(z, ps, 8.33333333332248946124e-03);
    const double sn = fma(z * r, fma(z, ps, -1.66666666666666324348e-01), r);
    double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = fma(z, pc, -2.75573143513906633035e-07);
    pc = fma(z, pc, 2.48015872894767294178e-05);
    pc = fma(z, pc, -1.38888888888741095749e-03);
    pc = fma(z, pc, 4.16666666666666019037e-02);
    const double cs = 1.0 - fma(0.5, z, -(z * (z * pc)));
    const double sq = (k & 1) ? cs : sn, cq = (k & 1) ? sn : cs;
    s_out = (float)((k & 2) ? -sq : sq);
    c_out = (float)(((k + 1) & 2) ? -cq : cq);
}

}  // namespace vslam
