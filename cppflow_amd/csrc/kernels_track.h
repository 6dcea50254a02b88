// kernels_track.h -- tracking IK in one launch: k candidate joint-space paths along one target path (cppf_track_paths).
// Included inside the anonymous namespace of cppflow_hip.hip (and handed to hipRTC) after kernels_fused.h; gfx950 only.
//
// One lane = one (candidate i, segment s) pair.  The path [0, T) is cut into S contiguous segments; lane (i, s) walks the waypoints of
// its segment in order and keeps q in registers, so the whole candidate set is ONE launch instead of one launch per waypoint.  At every
// waypoint the lane runs a block of LM iterations with exactly the semantics of a fused launch of that many steps (lm_row_iterate of
// kernels_fused.h: without tolerances the first iteration lean with the any-angle polynomials, the middle ones lean, the last canonical;
// with tolerances every iteration general and early-out).  So with S = 1, no recovery and the same start a candidate is the chain of
// fused launches a per-waypoint loop issues (planners.LmIkSeedProvider), in one launch.
//
//   first waypoint of a segment   start from q0[i * S + s] (caller) or a uniform draw in lo + (hi - lo) [0.1, 0.9]; n_restart iterations
//   every later waypoint          warm start from the previous waypoint's q; n_track iterations
//   recovery ladder               a row that is not converged (tolerances set) or whose joint change from the previous row exceeds
//                                 max_jump (set) tries (1) the warm start continued up to n_restart iterations in total, then (2) up to
//                                 R fresh random restarts of n_restart iterations each, stopping at the first attempt that is both
//                                 converged and within max_jump; the attempt kept is the first such one, else the one with the lowest
//                                 scaled pose error  a_pos^2 |e_pos|^2 + a_rot^2 |e_rot|^2
//
// Randomness is counter-based: a 32-bit integer hash of (seed, call_index, candidate, segment, waypoint, attempt, joint).  The same
// arguments give bit-identical output; nothing is kept between launches.
//
// Non-finite inputs as in lm_fused_kernel: a lane whose q0 row is not finite runs like any other and has every row it writes poisoned
// (q, pos_err, rot_err NaN, status 0); a waypoint whose target is not finite is written NaN / 0 by every lane, which then carries its q
// on unchanged to the next waypoint.
#pragma once

// status bits (include/cppflow_hip.h: CPPF_TRACK_*)
constexpr uint8_t kTrackConverged = 1, kTrackRestarted = 2, kTrackJump = 4, kTrackRecovered = 8;

// Kernel arguments besides the chain and the LM parameters (prm.n_steps unused: the blocks have their own lengths).
struct TrackK {
    const float* target;  // [T, 7]
    const float* q0;      // [k * S, d] or NULL
    float* q_out;         // [k, T, d]
    float* pos_err;       // [k, T]
    float* rot_err;       // [k, T]
    uint8_t* status;      // [k, T]
    int32_t T, k, S;
    int32_t n_restart, n_track, n_random;
    float max_jump_rad, max_jump_m;  // 0 = off
    uint32_t seed, call_index;
};

__device__ __forceinline__ uint32_t track_mix(uint32_t h) {  // a 32-bit finaliser (good avalanche, integer VALU only)
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

// A uniform draw inside the joint box lo + (hi - lo) [0.1, 0.9] for (candidate, segment, waypoint, attempt).
template <class RB>
__device__ __forceinline__ void track_draw(const RB& rb, const TrackK& tk, uint32_t i, uint32_t s, uint32_t t, uint32_t attempt,
                                           float (&q)[RB::D]) {
    uint32_t h = track_mix(tk.seed ^ 0x5bd1e995u);
    h = track_mix(h ^ tk.call_index);
    h = track_mix(h ^ i);
    h = track_mix(h ^ s);
    h = track_mix(h ^ t);
    h = track_mix(h ^ attempt);
#pragma unroll
    for (int j = 0; j < RB::D; ++j) {
        const uint32_t hj = track_mix(h ^ (uint32_t)(j + 1) * 0x9e3779b9u);
        const float u = (float)(hj >> 8) * 0x1p-24f;  // [0, 1)
        q[j] = rb.lo(j) + (rb.hi(j) - rb.lo(j)) * (0.1f + 0.8f * u);
    }
}

// n LM iterations of one row toward (Rt, tt), exactly as a fused launch of n steps runs them (lm_fused_kernel's loop).
template <class RB>
__device__ __forceinline__ void track_block(const RB& rb, const LmK& prm, const float (&Rt)[9], const float (&tt)[3],
                                            float* __restrict__ gate_lds, int n, float (&q)[RB::D]) {
    cppf_lm_outputs none = {};
    int it = 0;
    if (!(prm.tol_pos2 > 0.f)) {  // wave-uniform
        if (n >= 2) {
            (void)lm_row_iterate<RB, CPPF_FIRST_LEAN != 0, true>(rb, prm, none, 0, false, Rt, tt, gate_lds, q);
            it = 1;
        }
        for (; it < n - 1; ++it) (void)lm_row_iterate<RB, true>(rb, prm, none, 0, false, Rt, tt, gate_lds, q);
    }
    for (; it < n; ++it) {
        const bool conv = lm_row_iterate<RB, false>(rb, prm, none, 0, false, Rt, tt, gate_lds, q);
        if (prm.tol_pos2 > 0.f && __builtin_amdgcn_ballot_w64(!conv) == 0ull) break;
    }
}

constexpr int kTrackBlock = 64;  // one wavefront per workgroup: k * S lanes are few, spread them over the compute units

template <class RB>
__global__ __launch_bounds__(kTrackBlock) __attribute__((amdgpu_waves_per_eu(1, 2))) void track_kernel(const ChainK ch, const CollK co,
                                                                                                        const LmK prm, const TrackK tk) {
    constexpr int D = RB::D;
    __shared__ float s_gate[GateLds<D>::kFloats];  // the conditioning gate's slots of this (single) wavefront
    const RB rb{ch, co};
    const uint32_t lane_id = blockIdx.x * (unsigned)kTrackBlock + threadIdx.x;
    if (lane_id >= (uint32_t)(tk.k * tk.S)) return;
    const uint32_t i = lane_id / (uint32_t)tk.S, s = lane_id % (uint32_t)tk.S;
    const int t_begin = (int)(((long long)s * tk.T) / tk.S), t_end = (int)(((long long)(s + 1) * tk.T) / tk.S);
    const bool check_jump = tk.max_jump_rad > 0.f || tk.max_jump_m > 0.f;
    const bool have_tol = prm.tol_pos2 > 0.f;

    float q[D];
    bool lane_bad = false;
    if (tk.q0) {
        load_x<D>(tk.q0, lane_id, q);
        float chk = 0.f;
#pragma unroll
        for (int j = 0; j < D; ++j) chk += q[j];
        lane_bad = !(fabsf(chk) < INFINITY);
    } else {
        track_draw<RB>(rb, tk, i, s, (uint32_t)t_begin, 0u, q);
    }

    for (int t = t_begin; t < t_end; ++t) {
        float Rt[9], tt[3];
        load_target(tk.target, t, Rt, tt);
        float chk = tt[0] + tt[1] + tt[2];
#pragma unroll
        for (int k = 0; k < 9; ++k) chk += Rt[k];
        const size_t row = (size_t)i * (size_t)tk.T + (size_t)t;
        if (!(fabsf(chk) < INFINITY)) {  // nothing to track here
            float qn[D];
#pragma unroll
            for (int j = 0; j < D; ++j) qn[j] = __builtin_nanf("");
            store_x<D>(tk.q_out, row, qn);
            tk.pos_err[row] = __builtin_nanf("");
            tk.rot_err[row] = __builtin_nanf("");
            tk.status[row] = 0;
            continue;
        }
        const bool first = t == t_begin;
        // attempt 0: the segment's start (q as set above) or the warm start; kind 0 = that, 1 = warm continuation, 2 = random restart
        float qa[D], best[D];
#pragma unroll
        for (int j = 0; j < D; ++j) qa[j] = best[j] = q[j];
        int n_it = first ? tk.n_restart : tk.n_track, kind = 0, best_kind = 0, restarts = 0;
        bool more = true, best_ok = false, best_conv = false, best_jump = false;
        float best_score = INFINITY, best_pe = __builtin_nanf(""), best_re = __builtin_nanf("");
        while (__builtin_amdgcn_ballot_w64(more) != 0ull) {  // lanes of one wavefront climb the ladder together, each as far as it needs
            if (more) {
                track_block<RB>(rb, prm, Rt, tt, s_gate, n_it, qa);
                float R[9], p[3], e[6], pe, re;
                fk_ee<RB>(rb, qa, R, p);
                pose_error(Rt, tt, R, p, e);
                pose_metrics(Rt, tt, R, p, pe, re);
                const float ep2 = dot3(e[3], e[4], e[5], e[3], e[4], e[5]), er2 = dot3(e[0], e[1], e[2], e[0], e[1], e[2]);
                const bool conv = have_tol && ep2 < prm.tol_pos2 && er2 < prm.tol_rot2;
                bool jump = false;
                if (check_jump && !first) {
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        const float dq = fabsf(qa[j] - q[j]), bar = rb.pris(j) ? tk.max_jump_m : tk.max_jump_rad;
                        jump |= bar > 0.f && !(dq <= bar);
                    }
                }
                const bool ok = (conv || !have_tol) && !jump;
                const float score = prm.a_pos * prm.a_pos * ep2 + prm.a_rot * prm.a_rot * er2;
                if ((ok && !best_ok) || (ok == best_ok && score < best_score) || kind == 0) {  // (attempt 0 always fills `best`)
#pragma unroll
                    for (int j = 0; j < D; ++j) best[j] = qa[j];
                    best_ok = ok, best_conv = conv, best_jump = jump, best_score = score, best_pe = pe, best_re = re, best_kind = kind;
                }
                // the next rung
                if (ok) {
                    more = false;
                } else if (kind == 0 && !first && !conv && tk.n_restart > tk.n_track) {
                    kind = 1, n_it = tk.n_restart - tk.n_track;  // continue from qa
                } else if (restarts < tk.n_random) {
                    ++restarts;
                    kind = 2, n_it = tk.n_restart;
                    track_draw<RB>(rb, tk, i, s, (uint32_t)t, (uint32_t)restarts, qa);
                } else {
                    more = false;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < D; ++j) q[j] = best[j];
        uint8_t st = (best_conv ? kTrackConverged : 0) | ((first || best_kind == 2) ? kTrackRestarted : 0) |
                     (best_jump ? kTrackJump : 0) | (best_kind == 1 ? kTrackRecovered : 0);
        if (lane_bad) {
#pragma unroll
            for (int j = 0; j < D; ++j) best[j] = __builtin_nanf("");
            best_pe = best_re = __builtin_nanf("");
            st = 0;
        }
        store_x<D>(tk.q_out, row, best);
        tk.pos_err[row] = best_pe;
        tk.rot_err[row] = best_re;
        tk.status[row] = st;
    }
}
