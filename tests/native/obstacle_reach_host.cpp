// obstacle_reach_host.cpp -- host-only test entry around csrc/obstacle_reach.h (the capsule reach bits of cppf_set_obstacles).
// Built by tests/test_collision_prune.py with the host compiler: g++ -O2 -ffp-contract=off -shared -fPIC.
#include "../../cppflow_amd/csrc/obstacle_reach.h"

extern "C" void cppf_test_capsule_reach(const cppf_robot_desc* desc, const float* cap_c, const float* cap_cull, int nobs,
                                        const float* obs_lo, const float* obs_hi, uint32_t* live_any, uint32_t* live_lim) {
    const cppf::CapsuleReach r = cppf::capsule_reach(*desc, reinterpret_cast<const float (*)[3]>(cap_c), cap_cull, nobs,
                                                     reinterpret_cast<const float (*)[3]>(obs_lo),
                                                     reinterpret_cast<const float (*)[3]>(obs_hi));
    *live_any = r.any;
    *live_lim = r.lim;
}
