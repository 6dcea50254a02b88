// kernels_motion_resolve.h -- the motion test of kernels_motion.h made ADAPTIVE (cppf_motion_resolve): only the intervals whose test
// fails are bisected, until they pass, a node penetrates, or the depth floor is reached.  Included inside the anonymous namespace of
// cppflow_hip.hip behind kernels_motion.h, whose interval test, travel bound and self-pair walk it shares; gfx950 only.
//
// Definition: include/cppflow_hip.h (cppf_motion_resolve), steps 0 .. 7.  Node (L, i) is a for i = 0, b for i = 2^L, else
// fmaf(i 2^-L, b - a, a); interval (L, i) passes when every self pair and every (capsule, cuboid) has
// (clear_i + clear_{i+1}) - lambda 2^-L > 1e-6 in fp32 -- the very expressions of motion_kernel, so that start_level == max_depth
// reproduces cppf_motion_clearance bit for bit.
//
// Shape.  ONE wavefront per transition, and it walks ALL of the scene's cuboids (no grid.y cut: the children of an interval cannot
// be formed before every body has been tested).  The frontier F of level L is a list of interval indices in ascending order; a
// pass takes 32 of them: lanes 2k and 2k+1 hold the two end nodes of the interval in slot k, the decision is one __shfl_down per
// compared value (motion_interval_fails) and is read on the even lane.  Lanes past the end of the frontier work on a copy of its
// last interval and report nothing.  The 64 nodes of a pass lie on one short joint-space segment, so the wavefront's box is tight
// and the tile test of scene_kernel culls most of a scene.
// Frontier.  Two buffers of max_frontier indices per transition in the workspace.  The failing intervals of a pass are compacted
// with a ballot and a popcount of the lower lanes; each writes its two children 2i, 2i+1 behind those of the passes before, which
// keeps the list ascending and independent of anything but the decisions themselves.  Level start_level needs no list (slot k is
// interval k).  The list is written by some lanes and read by others of the SAME wavefront one level later: a wavefront-scope
// fence orders the two; nothing crosses wavefronts, so there is no barrier, no atomic and no waiting anywhere.  Writes past
// max_frontier are dropped (the count goes on, and the next level reports the overflow).
// Cost.  Trip counts are bounded by max_depth - start_level + 1 levels of at most ceil(max_frontier / 32) passes.  A transition
// that is skipped costs one byte read; one that ends at its start level costs that level's passes.  The wavefronts of a block run
// different trip counts and share nothing: the generic form's capsules are in LDS slots private to each lane.
// Outputs are reduced over the lanes once per level (integer minima on scene_key and on the node index) and written by lane 0 when
// the transition ends: one launch, no float atomics, two runs are bit-identical.
#pragma once

struct ResolveK {
    const float* box_lo;  // DEVICE [n_obs, 3] world-frame corners
    const float* box_hi;
    const float* rho;        // DEVICE [CPPF_MAX_DOF][CPPF_MAX_CAPSULES] (the handle's table)
    const uint8_t* decided;  // [S (W-1)] or NULL; may alias status
    uint8_t* status;         // [S (W-1)]
    int32_t* depth;          // [S (W-1)] or NULL
    int32_t* hit_num;        // [S (W-1)] or NULL
    float* min_clear;        // [S (W-1)] or NULL
    int32_t* n_tested;       // [S (W-1)] or NULL
    uint32_t* frontier;      // workspace [S (W-1)][2][max_frontier]
    int32_t S, W, start_level, max_depth, max_frontier, n_obs;
    float reach;
    float tile_cull2;  // as SceneK
    float cull2[CPPF_MAX_CAPSULES];
};

constexpr uint8_t kMotionOverflow = 4;  // CPPF_MOTION_OVERFLOW

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, s, 64);
        v = o < v ? o : v;
    }
    return v;
}

template <class RB>
__global__ __launch_bounds__(kBlock, CPPF_WAVES_COLL) void motion_resolve_kernel(const ChainK ch, const CollK co, const ResolveK rk,
                                                                                  const float* __restrict__ q) {
    extern __shared__ float lds[];
    constexpr int D_ = RB::D;
    const RB rb{ch, co};
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t tr = (size_t)blockIdx.x * (kBlock / 64) + (size_t)(tid >> 6);
    if (tr >= (size_t)rk.S * (size_t)(rk.W - 1)) return;       // (wave-uniform)
    if (rk.decided != nullptr && rk.decided[tr] != 0) return;  // step 0 (wave-uniform: one byte for the whole wavefront)
    const size_t s = tr / (size_t)(rk.W - 1);
    const size_t row = s * (size_t)rk.W + (tr - s * (size_t)(rk.W - 1));  // waypoint a; b is the next row
    const uint32_t row32 = (uint32_t)row;  // (S W <= 2 S (W-1) < 2^32: the host refuses more than 2^31-1 transitions)

    float dq[D_];
    int outside = 0;
    {
        float a[D_], b[D_];
        load_x<D_>(q, row, a);
        load_x<D_>(q, row + 1, b);
#pragma unroll
        for (int j = 0; j < D_; ++j) {
            dq[j] = fabsf(b[j] - a[j]);
            outside |= !(a[j] >= rb.lo(j) && a[j] <= rb.hi(j)) | !(b[j] >= rb.lo(j) && b[j] <= rb.hi(j));
        }
    }
    outside = __builtin_amdgcn_ballot_w64(outside != 0) != 0ull;

    constexpr int LS = SceneCaps<RB>::L;
    float slam[LS];  // (the specialised form keeps lambda_c; the generic one forms it again per survivor)
    if constexpr (RB::kStatic) {
        using T = typename RB::Table;
#pragma unroll
        for (int c = 0; c < T::L; ++c) slam[c] = motion_lambda<D_>(rk.rho, dq, -1, T::cap_link[c], c);
    }

    uint32_t* cur = rk.frontier + tr * 2 * (size_t)rk.max_frontier;
    uint32_t* nxt = cur + rk.max_frontier;
    int L = rk.start_level, n = 1 << rk.start_level, tested = 0;
    uint32_t key_min = scene_key(INFINITY);  // per lane until the end of a level, then the wavefront's
    int hit_min = 0x7fffffff;
    uint8_t status = 0;
    for (;;) {  // one level per trip: at most max_depth - start_level + 1
        if (n > rk.max_frontier) {
            status = kMotionOverflow;
            break;
        }
        tested += n;
        const int M = 1 << L;
        const float inv_m = __int_as_float((127 - L) << 23);  // 2^-L
        const bool last = L == rk.max_depth;
        // every cuboid the culling skips (kernels_motion.h, "Culling"): reach at both ends of the interval
        int far_fail = 0;
        if (rk.n_obs > 0) {
            if constexpr (RB::kStatic) {
#pragma unroll
                for (int c = 0; c < RB::Table::L; ++c) far_fail |= !((rk.reach + rk.reach) - slam[c] * inv_m > kMotionSlack);
            } else {
                for (int c = 0; c < co.ncaps; ++c)
                    far_fail |= !((rk.reach + rk.reach) - motion_lambda<D_>(rk.rho, dq, -1, co.cap_link[c], c) * inv_m > kMotionSlack);
            }
        }
        int n_next = 0;
        for (int base = 0; base < n; base += 32) {  // one pass per 32 intervals: at most ceil(max_frontier / 32)
            const int slot = base + (lane >> 1);
            const bool have = slot < n;
            const int k = have ? slot : n - 1;  // (a lane past the end: a copy of the last interval)
            const uint32_t iv = L == rk.start_level ? (uint32_t)k : cur[k];
            const int i = (int)iv + (lane & 1);  // this lane's node

            // Nothing of a pass may be carried into it from outside the loop: what depends on |b - a| alone (a pair's lambda, 55 of
            // them on Chain12) or on the waypoints would otherwise be hoisted and held in registers across the whole pass.  The
            // empty asm statements make dq and the row opaque, so the waypoints are loaded and the lambdas formed where they are used.
            uint32_t row_here = row32;
            asm volatile("" : "+v"(row_here));
#pragma unroll
            for (int j = 0; j < D_; ++j) asm volatile("" : "+v"(dq[j]));
            float x[D_], R[9], p[3];
            {
                float a[D_], b[D_];
                load_x<D_>(q, (size_t)row_here, a);
                load_x<D_>(q, (size_t)row_here + 1, b);
                const float f = (float)i * inv_m;
#pragma unroll
                for (int j = 0; j < D_; ++j) x[j] = i == 0 ? a[j] : (i == M ? b[j] : CPPF_FMA(f, b[j] - a[j], a[j]));
            }
            float swc[LS][3], swh[LS][3];
            float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
            if constexpr (RB::kStatic) {
                capsule_fk_static<RB>(rb, x, R, p, swc, swh);
#pragma unroll
                for (int c = 0; c < RB::Table::L; ++c) box_add_segment(swc[c], swh[c], blo, bhi);
            } else {
                fk_capsules_to_lds<RB>(rb, co, x, lds, tid, R, p);
                for (int c = 0; c < co.ncaps; ++c) {
                    float wc[3], wh[3];
                    lds_capsule(lds, tid, c, wc, wh);
                    box_add_segment(wc, wh, blo, bhi);
                }
            }

            int fail = far_fail;
            float m = INFINITY;  // the node's smallest clearance, untruncated
            // ---- the self pairs --------------------------------------------------------------------------------------------------------
            if constexpr (RB::kStatic) {
                motion_self_static<RB, 0, RB::Table::P>(swc, swh, rk.rho, dq, inv_m, m, fail);
            } else {
                for (int pi = 0; pi < co.npairs; ++pi) {
                    const int a = co.pair_a[pi], b = co.pair_b[pi];
                    float ca[3], ha[3], cb[3], hb[3];
                    lds_capsule(lds, tid, a, ca, ha);
                    lds_capsule(lds, tid, b, cb, hb);
                    const float d2 = seg_seg_dist2(ca, ha, cb, hb, co.cap_a[a], co.cap_ia[a], co.cap_a[b], co.cap_ia[b]);
                    const float v = __builtin_sqrtf(d2) - (co.cap_r[a] + co.cap_r[b]);
                    m = v < m ? v : m;
                    const int la = co.cap_link[a], lb = co.cap_link[b];
                    const float lam = la <= lb ? motion_lambda<D_>(rk.rho, dq, la, lb, b) : motion_lambda<D_>(rk.rho, dq, lb, la, a);
                    fail |= motion_interval_fails(v, lam, inv_m);
                }
            }
            // ---- the cuboids, all of them ----------------------------------------------------------------------------------------------
            if (rk.n_obs > 0) {
#pragma unroll
                for (int kk = 0; kk < 3; ++kk) {
                    blo[kk] = wave_min(blo[kk]);
                    bhi[kk] = wave_max(bhi[kk]);
                }
                float best = INFINITY;
                for (int ob = 0; ob < rk.n_obs; ob += 64) {
                    const int ol = ob + lane;
                    const bool have_o = ol < rk.n_obs;
                    float llo[3], lhi[3];
#pragma unroll
                    for (int kk = 0; kk < 3; ++kk) {
                        llo[kk] = have_o ? rk.box_lo[(size_t)ol * 3 + kk] : 0.f;
                        lhi[kk] = have_o ? rk.box_hi[(size_t)ol * 3 + kk] : 0.f;
                    }
                    float g2 = 0.f;
#pragma unroll
                    for (int kk = 0; kk < 3; ++kk) {
                        const float gg = fmaxf(fmaxf(llo[kk] - bhi[kk], blo[kk] - lhi[kk]), 0.f);
                        g2 = CPPF_FMA(gg, gg, g2);
                    }
                    unsigned long long live = __builtin_amdgcn_ballot_w64(have_o && !(g2 > rk.tile_cull2));
                    while (live != 0ull) {
                        const int jj = __builtin_ctzll(live);
                        live &= live - 1ull;
                        const float lo[3] = {readlane_f(llo[0], jj), readlane_f(llo[1], jj), readlane_f(llo[2], jj)};
                        const float hi[3] = {readlane_f(lhi[0], jj), readlane_f(lhi[1], jj), readlane_f(lhi[2], jj)};
                        if constexpr (RB::kStatic) {
                            using T = typename RB::Table;
#pragma unroll
                            for (int c = 0; c < T::L; ++c) {
                                if (cull_far(point_box_dist2(swc[c], lo, hi), rk.cull2[c])) continue;
                                const float v = __builtin_sqrtf(seg_box_dist2(swc[c], swh[c], lo, hi)) - T::cap_r[c];
                                best = v < best ? v : best;
                                fail |= motion_interval_fails(v < rk.reach ? v : rk.reach, slam[c], inv_m);
                            }
                        } else {
                            for (int c = 0; c < co.ncaps; ++c) {
                                float wc[3], wh[3];
                                lds_capsule(lds, tid, c, wc, wh);
                                if (cull_far(point_box_dist2(wc, lo, hi), rk.cull2[c])) continue;
                                const float v = __builtin_sqrtf(seg_box_dist2(wc, wh, lo, hi)) - co.cap_r[c];
                                best = v < best ? v : best;
                                const float lam = motion_lambda<D_>(rk.rho, dq, -1, co.cap_link[c], c);
                                fail |= motion_interval_fails(v < rk.reach ? v : rk.reach, lam, inv_m);
                            }
                        }
                    }
                }
                if (best < rk.reach) m = best < m ? best : m;  // (min_env as the scene kernel reports it: nothing beyond reach)
            }

            // ---- this pass's part of the level: the minima, and the children of what failed ----------------------------------------------
            // (a lane past the end holds a copy of a real node: what it adds to a minimum that node adds as well)
            const uint32_t key = scene_key(m);
            key_min = key < key_min ? key : key_min;
            if (m < 0.f) hit_min = i < hit_min ? i : hit_min;
            const bool split = have && (lane & 1) == 0 && fail != 0;  // (the interval's verdict is the even lane's)
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(split);
            if (split && !last) {
                const int pos = n_next + 2 * __builtin_popcountll(mask & ((1ull << lane) - 1ull));
                if (pos < rk.max_frontier) nxt[pos] = 2u * iv;
                if (pos + 1 < rk.max_frontier) nxt[pos + 1] = 2u * iv + 1u;
            }
            n_next += 2 * __builtin_popcountll(mask);
        }
        key_min = wave_min_u32(key_min);
        hit_min = (int)wave_min_u32((uint32_t)hit_min);  // (node indices are not negative)
        if (hit_min != 0x7fffffff) {
            status = 2;  // CPPF_MOTION_HIT
            break;
        }
        if (outside) break;  // undecided: outside the limits the prismatic term of rho is no bound
        if (n_next == 0) {
            status = 1;  // CPPF_MOTION_CERTIFIED
            break;
        }
        if (last) break;  // undecided at the floor
        // the children were written by some lanes and are read by others of this wavefront
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        uint32_t* const t = cur;
        cur = nxt;
        nxt = t;
        n = n_next;
        ++L;
    }
    if (lane == 0) {
        rk.status[tr] = status;
        if (rk.depth) rk.depth[tr] = L;
        if (rk.hit_num) rk.hit_num[tr] = status == 2 ? hit_min : -1;
        if (rk.min_clear) rk.min_clear[tr] = scene_unkey(key_min);
        if (rk.n_tested) rk.n_tested[tr] = tested;
    }
}
