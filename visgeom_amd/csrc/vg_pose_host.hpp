// vg_pose_host.hpp -- the pose arithmetic of vg_transf_host.hpp on the plain double[6] the C ABI and the handles hold, and the
// rotation matrices the image pipelines upload with a pose, each in one arithmetic order: rot_trig(.., true, false), then
// rotation_matrix (the library is built with -ffp-contract=off, so the bits follow the statements).  Host only; kept apart
// from vg_transf_host.hpp, which the calibration units include.
#pragma once

#include <cstring>

#include "vg_transf_host.hpp"

namespace vgth {

inline Array6d load6(const double *p)
{
    Array6d a;
    std::memcpy(a.data(), p, sizeof(double) * 6);
    return a;
}

inline void store6(const Array6d &a, double *p) { std::memcpy(p, a.data(), sizeof(double) * 6); }

inline void compose(const double *a6, const double *b6, double *out6) { store6(compose(load6(a6), load6(b6)), out6); }
inline void inverse_compose(const double *a6, const double *b6, double *out6) { store6(inverse_compose(load6(a6), load6(b6)), out6); }
inline void inverse(const double *a6, double *out6) { store6(inverse(load6(a6)), out6); }

// rotMat of the pose xi = [t, rotvec], row-major
inline void rotation(const double *xi, double *R)
{
    const vg::RotTrig rt = vg::rot_trig(xi + 3, true, false);
    vg::rotation_matrix(xi + 3, 1., rt, R);
}

// rotMatInv | trans of the pose xi: what a kernel needs to bring a point into the pose's frame; R: rotMat as well, from the
// same rot_trig (a caller with hundreds of poses per call)
inline void inverse_frame(const double *xi, double *Rinv, double *t, double *R = nullptr)
{
    const vg::RotTrig rt = vg::rot_trig(xi + 3, true, false);
    if (R) vg::rotation_matrix(xi + 3, 1., rt, R);
    vg::rotation_matrix(xi + 3, -1., rt, Rinv);
    for (int i = 0; i < 3; i++) t[i] = xi[i];
}

}  // namespace vgth
