// obstacle_reach.h -- which capsules can reach ANY cuboid of an obstacle set: decided once per cppf_set_obstacles, on the host.
// Plain C++ (no HIP): part of cppflow_hip.hip, and compiled on its own by tests/test_collision_prune.py.
//
// The mask-only collision stage of the robot-specialised kernels (collide_tests_static, kernels_collision.h) asks, per row and per
// capsule, whether some lane of the wavefront is within broad-phase reach of each cuboid.  For some capsules the answer is "no" for
// every row of every launch, and known as soon as the cuboids are:
//   * a capsule of the base (cap_link < 0) does not move: its centre is the table's constant, and the device's own bounding-sphere
//     test  point_box_dist2(centre) > cap_cull  has one answer.  It is evaluated here in fp32 in the device's operation order, so
//     the bit is exactly what every lane would compute, whatever the row holds          -> bits `any` and `lim`;
//   * a capsule of link l stays inside the ball of radius rho about the origin o of joint 0's frame (a point of the world):
//     rho = sum_{1 <= j <= l} |t_j| + max(|p0|, |p1|) + the largest |q_j| of every prismatic joint j <= l, since a rotation keeps
//     norms and each fixed transform adds at most its translation.  If dist(o, box) > rho + r + 1 cm no point of the capsule's
//     axis comes within r + 1 cm of the cuboid, and with 1 cm of slack the exact fp32 test could only have said "no hit" (the
//     argument of cull_far).  This needs q inside the joint limits (the prismatic terms; and a rotation matrix that is one, which
//     the sine / cosine give inside their domain only)                                    -> bit `lim` only.
// Bit c set = capsule c is LIVE.  Everything rounds towards "live".
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/cppflow_hip.h"

namespace cppf {

struct CapsuleReach {
    uint32_t any;  // valid for any row
    uint32_t lim;  // valid for rows inside the joint limits (a subset of `any`)
};

// point_box_dist2 of kernels_collision.h, value for value (clampf is a median of three: for lo <= hi and a non-NaN x, the clamp)
inline float host_point_box_dist2(const float m[3], const float lo[3], const float hi[3]) {
    float e[3];
    for (int k = 0; k < 3; ++k) {
        const float cl = m[k] < lo[k] ? lo[k] : (m[k] > hi[k] ? hi[k] : m[k]);
        e[k] = m[k] - cl;
    }
    return fmaf(e[2], e[2], fmaf(e[1], e[1], e[0] * e[0]));
}

// cap_c / cap_cull: the centres and broad-phase thresholds of CollK; obs_lo / obs_hi: the world-frame corners of CollK
inline CapsuleReach capsule_reach(const cppf_robot_desc& d, const float (*cap_c)[3], const float* cap_cull, int nobs,
                                  const float (*obs_lo)[3], const float (*obs_hi)[3]) {
    CapsuleReach r{0u, 0u};
    const double o[3] = {d.F[0][9], d.F[0][10], d.F[0][11]};
    // travel[l]: bound on the distance from o of the origin of link l's frame
    double travel[CPPF_MAX_DOF];
    double acc = 0.0;
    for (int j = 0; j < d.ndof; ++j) {
        if (j > 0) acc += sqrt((double)d.F[j][9] * d.F[j][9] + (double)d.F[j][10] * d.F[j][10] + (double)d.F[j][11] * d.F[j][11]);
        if (d.jtype[j] == CPPF_JOINT_PRISMATIC) acc += fmax(fabs((double)d.lo[j]), fabs((double)d.hi[j]));
        travel[j] = acc;
    }
    for (int c = 0; c < d.n_capsules; ++c) {
        const int l = d.cap_link[c];
        bool live_any = true, live_lim = false;
        // A capsule of link 0 whose axis lies ON a revolute joint 0's axis (end points with x = y = 0 in the link's frame) does not
        // move either, and its centre on the device is the same for every row: frame 0 is F_0 exactly (the identity times F_0), the
        // joint's rotation changes the first two columns of R only, and xform_point of (0, 0, cz) reads the third: t + R_z cz, one fma.
        const bool on_axis0 = l == 0 && d.jtype[0] == CPPF_JOINT_REVOLUTE && d.cap_p0[c][0] == 0.f && d.cap_p0[c][1] == 0.f &&
                              d.cap_p1[c][0] == 0.f && d.cap_p1[c][1] == 0.f;
        if (l < 0 || on_axis0) {
            float m[3] = {cap_c[c][0], cap_c[c][1], cap_c[c][2]};
            if (on_axis0)
                for (int k = 0; k < 3; ++k) m[k] = fmaf(d.F[0][3 * k + 2], cap_c[c][2], d.F[0][9 + k]);
            live_any = false;
            for (int ob = 0; ob < nobs; ++ob) live_any |= !(host_point_box_dist2(m, obs_lo[ob], obs_hi[ob]) > cap_cull[c]);
            live_lim = live_any;
        } else {
            double n0 = 0.0, n1 = 0.0;
            for (int k = 0; k < 3; ++k) n0 += (double)d.cap_p0[c][k] * d.cap_p0[c][k], n1 += (double)d.cap_p1[c][k] * d.cap_p1[c][k];
            const double reach = (travel[l] + sqrt(fmax(n0, n1)) + (double)d.cap_r[c] + 0.01) * (1.0 + 1e-6);
            for (int ob = 0; ob < nobs; ++ob) {
                double d2 = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double lo = obs_lo[ob][k], hi = obs_hi[ob][k];
                    const double e = o[k] < lo ? lo - o[k] : (o[k] > hi ? o[k] - hi : 0.0);
                    d2 += e * e;
                }
                live_lim |= !(d2 > reach * reach);
            }
        }
        if (live_any) r.any |= 1u << c;
        if (live_lim) r.lim |= 1u << c;
    }
    return r;
}

}  // namespace cppf
