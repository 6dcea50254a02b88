// kernels_optloop.h -- the alternating LM optimiser loop decided on the device (cppf_lm_optimize_enqueue).
//
// run_lm_alternating_loss (cppflow_amd/optimization.py; the reference: cppflow/optimization.py:147-373) takes, per iteration, one
// decision from the [S,16] plan metrics of the iteration's result: which step comes next, whether a valid trajectory is in hand,
// whether the TL measure has converged, whether the loop is over.  Here that decision is `optloop_decide` -- plain C++ without a HIP
// intrinsic, so that the host compiler builds the very same function for the CPU tests (tests/test_optloop_decide.py) -- and the
// kernels around it: the decision kernel (one wavefront per loop-control record; it also takes the snapshot of a valid x), and the
// gated entry points of the clamp and of the plan metrics.  The steps and the capsule masks are the existing kernels, which take the
// gate (StepGateK, lmik_device.h) as their last argument.  Ordering comes from the stream alone: nothing here waits or polls.
//
// Part of the translation unit cppflow_hip.hip (included inside its anonymous namespace); the part above the HIP section also
// compiles on its own with a host compiler.
#pragma once

#include "../../include/cppflow_hip.h"

#if defined(__HIPCC__)
#define CPPF_HD __host__ __device__
#else
#define CPPF_HD
#endif

// One iteration's decision for one record (G = the trajectories it speaks for: 1, or all S), in the order of
// cppflow_amd/optimization.py:183-213.  `metrics` = the G rows of plan metrics of the iteration's (clamped) result; `rec` holds the
// mode the iteration took and is updated to the next one; `tr` receives the trace row.  Returns 1 when x is valid, i.e. when the
// caller has to take the snapshot (last_valid := x).
CPPF_HD inline int optloop_decide(const cppf_optloop_params& P, cppf_optloop_record& rec, const float* metrics, int G,
                                  cppf_optloop_trace& tr) {
    const int i = rec.n_steps;
    const bool took_differencing = rec.mode == CPPF_OPT_MODE_DIFF;
    rec.n_steps = i + 1;
    // TL: the summed revolute path length of every trajectory of the record (column 6), fp32, in index order
    float tl = 0.f;
    for (int g = 0; g < G; ++g) tl += metrics[g * 16 + 6];
    tr.mode = rec.mode;
    tr.tl = tl;
    tr.flags = -1;
    tr.valid = -1;
    if (took_differencing) {  // :186-195
        bool stop_now = false;
        if (!rec.converged && rec.has_tl) {
            double diff = (double)tl - (double)rec.last_tl;
            diff = diff < 0.0 ? -diff : diff;
            if (diff < P.convergence_threshold) {
                rec.converged = 1;
                stop_now = rec.last_valid_idx == i - 1;
            }
        }
        rec.last_tl = tl;
        rec.has_tl = 1;
        if (stop_now) {
            rec.mode = CPPF_OPT_MODE_DONE;
            rec.i_final = i;
            return 0;
        }
    }
    // x_is_valid (optimization_utils.py:387-404): the first trajectory, in order, below the four thresholds (strict <, fp32 against
    // fp32) and free of the collisions that are not ignored; the flags are those of the last trajectory examined, the collision
    // flags those of the last one that got that far
    const float thr[4] = {P.constraints.max_allowed_position_error_cm, P.constraints.max_allowed_rotation_error_deg,
                          P.constraints.max_allowed_mjac_deg, P.constraints.max_allowed_mjac_cm};
    int f[4] = {0, 0, 0, 0}, self_c = 0, env_c = 0, found = -1;
    for (int g = 0; g < G && found < 0; ++g) {
        const float* m = metrics + g * 16;
        f[0] = m[0] < thr[0], f[1] = m[2] < thr[1], f[2] = m[4] < thr[2], f[3] = m[5] < thr[3];
        if (!(f[0] && f[1] && f[2] && f[3])) continue;
        if (!P.constraints.self_collisions_ignored) {
            self_c = m[9] > 0.f ? 2 : 1;
            if (self_c == 2) continue;
        }
        if (!P.constraints.env_collisions_ignored) {
            env_c = m[10] > 0.f ? 2 : 1;
            if (env_c == 2) continue;
        }
        found = g;
    }
    rec.pose_pos_valid = f[0];
    rec.pose_rot_valid = f[1];
    tr.flags = f[0] | (f[1] << 1) | (f[2] << 2) | (f[3] << 3) | (self_c << 4) | (env_c << 6);
    tr.valid = found >= 0;
    bool done = false;
    if (found >= 0) {  // :202-207
        rec.last_valid_idx = i;
        rec.is_valid = 1;
        rec.valid_seed_idx = found;
        done = rec.converged != 0;
    }
    // :212-213, then the end of `for i in range(max_n_steps)`
    if (!done && rec.is_valid && P.return_if_valid_after_n_steps >= 0 && i > P.return_if_valid_after_n_steps) done = true;
    if (!done && i + 1 >= P.max_n_steps) done = true;
    rec.i_final = i;
    if (!done && f[0] && f[1] && P.on_pose_valid == CPPF_OPT_ON_POSE_VALID_STOP) {  // :166-168: the break at the top of iteration i + 1
        done = true;
        rec.i_final = i + 1;
    }
    rec.mode = done ? CPPF_OPT_MODE_DONE
                    : ((f[0] && f[1] && P.on_pose_valid == CPPF_OPT_ON_POSE_VALID_DIFFERENCING) ? CPPF_OPT_MODE_DIFF : CPPF_OPT_MODE_POSE);
    return found >= 0 ? 1 : 0;
}

// records [C] then trace rows [C][trace_capacity]
CPPF_HD inline size_t optloop_control_words(int S, const cppf_optloop_params& P) {
    const size_t C = P.per_trajectory ? (size_t)S : 1;
    return C * (sizeof(cppf_optloop_record) / 4) + C * (size_t)P.trace_capacity * (sizeof(cppf_optloop_trace) / 4);
}

#if defined(__HIPCC__)

static_assert(sizeof(cppf_optloop_record) == 64 && sizeof(cppf_optloop_trace) == 16, "layout documented in cppflow_hip.h");

// One wavefront per record.  Every lane reads the record and the metrics (uniform addresses) and takes the same decision; lane 0
// stores it; all 64 lanes copy the snapshot (G * W * d floats, coalesced).  The stores follow the loads they depend on, and no other
// wavefront touches this record or these rows of x / snapshot in this launch.
__global__ __launch_bounds__(64) void optloop_decide_kernel(const cppf_optloop_params P, int S, int W, int d,
                                                            const float* __restrict__ metrics, const float* __restrict__ x,
                                                            float* __restrict__ snapshot, int32_t* __restrict__ control) {
    const int C = P.per_trajectory ? S : 1, G = P.per_trajectory ? 1 : S;
    const int c = blockIdx.x;
    if (c >= C) return;
    cppf_optloop_record* recs = reinterpret_cast<cppf_optloop_record*>(control);
    cppf_optloop_trace* trace = reinterpret_cast<cppf_optloop_trace*>(recs + C);
    cppf_optloop_record rec = recs[c];
    if (rec.mode == CPPF_OPT_MODE_DONE) return;  // wavefront-uniform
    const int i = rec.n_steps;
    cppf_optloop_trace tr;
    const int snap = optloop_decide(P, rec, metrics + (size_t)c * G * 16, G, tr);
    if (threadIdx.x == 0) {
        recs[c] = rec;
        if (i < P.trace_capacity) trace[(size_t)c * P.trace_capacity + i] = tr;
    }
    if (snap) {
        const size_t count = (size_t)G * W * d, base = (size_t)c * count;
        for (size_t k = threadIdx.x; k < count; k += 64) snapshot[base + k] = x[base + k];
    }
}

// x := clamp(x_new) for the trajectories the gate opens (the host loop's `opt_state.x = clamp_to_joint_limits(robot, x_new)`).
// This launch is the loop's only writer of x, so a pinned end waypoint (CPPF_PIN_FIRST / CPPF_PIN_LAST) is held by skipping its
// elements here, whichever step wrote x_new.
__global__ __launch_bounds__(kBlock) void optloop_clamp_kernel(const ChainK ch, size_t total, int W, int pin,
                                                               const float* __restrict__ x_new, float* __restrict__ x,
                                                               const StepGateK gate) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / (size_t)ch.ndof;
    const size_t s = row / (size_t)W, t = row - s * (size_t)W;
    if (((pin & CPPF_PIN_FIRST) && t == 0) || ((pin & CPPF_PIN_LAST) && t + 1 == (size_t)W)) return;
    if (!step_open(gate, (int)s)) return;
    x[i] = clamp_joint(ch, (int)(i - row * (size_t)ch.ndof), x_new[i]);
}

// plan_metrics_kernel behind the gate: one wavefront per trajectory, all of it or none (wavefront-uniform)
template <int D>
__global__ __launch_bounds__(64) void optloop_metrics_kernel(const ChainK ch, const CollK co, int S, int W, const float* __restrict__ x,
                                                             const float* __restrict__ target,
                                                             const uint8_t* __restrict__ self_mask,
                                                             const uint8_t* __restrict__ env_mask, float* __restrict__ out,
                                                             const StepGateK gate) {
    const int s = blockIdx.x;
    if (s >= S || !step_open(gate, s)) return;
    plan_metrics_seed<D>(ch, co, s, W, x, target, self_mask, env_mask, nullptr, out);
}

#endif  // __HIPCC__
