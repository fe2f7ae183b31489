// CataCamera::liftProjective with the 8-step recursive distortion model + (b.x/b.z, b.y/b.z) -> Point2f
// (CataCamera.cc:556-626, 766-783; feature_tracker.cpp:306-309; pose_graph/src/keyframe.cpp:65-72).  All in double.
// One device function for every translation unit that lifts pixels (lvi_tracker.hip, lvi_kf.hip): the same code, the
// same bits.
#pragma once
#include "lvi_dev.hpp"

#ifdef __HIPCC__
namespace lvi {

__device__ __forceinline__ void mei_distortion(const lvi_mei_params& c, double pux, double puy, double& dux, double& duy)
{
    const double mx2_u = pux * pux, my2_u = puy * puy, mxy_u = pux * puy;
    const double rho2_u = mx2_u + my2_u;
    const double rad_dist_u = c.k1 * rho2_u + c.k2 * rho2_u * rho2_u;
    dux = pux * rad_dist_u + 2.0 * c.p1 * mxy_u + c.p2 * (rho2_u + 2.0 * mx2_u);
    duy = puy * rad_dist_u + 2.0 * c.p2 * mxy_u + c.p1 * (rho2_u + 2.0 * my2_u);
}

// pixel (x, y) -> (X / Z, Y / Z) of the lifted ray, stored as float
__device__ __forceinline__ void mei_lift_normalized(const lvi_mei_params& c, float x, float y, float& out_x, float& out_y)
{
    const double inv_K11 = 1.0 / c.gamma1, inv_K13 = -c.u0 / c.gamma1, inv_K22 = 1.0 / c.gamma2, inv_K23 = -c.v0 / c.gamma2;
    const bool noDistortion = c.k1 == 0.0 && c.k2 == 0.0 && c.p1 == 0.0 && c.p2 == 0.0;
    const double mx_d = inv_K11 * (double)x + inv_K13, my_d = inv_K22 * (double)y + inv_K23;
    double mx_u = mx_d, my_u = my_d;
    if (!noDistortion) {
        double dux, duy;
        mei_distortion(c, mx_d, my_d, dux, duy);
        mx_u = mx_d - dux; my_u = my_d - duy;
        for (int it = 1; it < 8; ++it) { mei_distortion(c, mx_u, my_u, dux, duy); mx_u = mx_d - dux; my_u = my_d - duy; }
    }
    double bz;
    if (c.xi == 1.0) bz = (1.0 - mx_u * mx_u - my_u * my_u) / 2.0;
    else { const double rho2_d = mx_u * mx_u + my_u * my_u; bz = 1.0 - c.xi * (rho2_d + 1.0) / (c.xi + sqrt(1.0 + (1.0 - c.xi * c.xi) * rho2_d)); }
    out_x = (float)(mx_u / bz); out_y = (float)(my_u / bz);
}

}  // namespace lvi
#endif  // __HIPCC__
