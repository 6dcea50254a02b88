// kernels_motion_resolve.h -- the motion test of kernels_motion.h made ADAPTIVE (cppf_motion_resolve): only the intervals whose test
// fails are bisected, until they pass, a node penetrates, or the depth floor is reached.  Included inside the anonymous namespace of
// cppflow_hip.hip behind kernels_motion.h, whose node test (motion_node_test, motion_far_fails) it calls; gfx950 only.
//
// Definition: include/cppflow_hip.h (cppf_motion_resolve), steps 0 .. 7.  Node (L, i) is a for i = 0, b for i = 2^L, else
// fmaf(i 2^-L, b - a, a); interval (L, i) passes when every self pair and every (capsule, cuboid) has
// (clear_i + clear_{i+1}) - lambda 2^-L > 1e-6 in fp32 -- motion_kernel's own node test, called not copied, so that
// start_level == max_depth reproduces cppf_motion_clearance bit for bit.
//
// Shape.  ONE wavefront per transition, and it walks ALL of the scene's cuboids (no grid.y cut: the children of an interval cannot
// be formed before every body has been tested).  The frontier F of level L is a list of interval indices in ascending order; a
// pass takes 32 of them: lanes 2k and 2k+1 hold the two end nodes of the interval in slot k, the decision is one __shfl_down per
// compared value (motion_interval_fails) and is read on the even lane.  Lanes past the end of the frontier work on a copy of its
// last interval and report nothing.  The 64 nodes of a pass lie on one short joint-space segment, so the wavefront's box is tight
// and the tile test of scene_walk culls most of a scene.
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
    SceneCullK cull;         // the scene and its culling thresholds (kernels_scene.h)
    const float* rho;        // DEVICE [CPPF_MAX_DOF][CPPF_MAX_CAPSULES] (the handle's table)
    const uint8_t* decided;  // [S (W-1)] or NULL; may alias status
    uint8_t* status;         // [S (W-1)]
    int32_t* depth;          // [S (W-1)] or NULL
    int32_t* hit_num;        // [S (W-1)] or NULL
    float* min_clear;        // [S (W-1)] or NULL
    int32_t* n_tested;       // [S (W-1)] or NULL
    uint32_t* frontier;      // workspace [S (W-1)][2][max_frontier]
    int32_t S, W, start_level, max_depth, max_frontier;
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

    float slam[LaneCaps<RB>::L];
    motion_cuboid_lambdas<RB>(rk.rho, dq, slam);
    LaneCaps<RB> caps(co, tid);

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
        // every cuboid the culling skips (kernels_motion.h, "Culling"): once per level
        const int far_fail = rk.cull.n_obs > 0 ? motion_far_fails<RB>(caps, rk.rho, dq, slam, rk.cull.reach, inv_m) : 0;
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
            float x[D_];
            {
                float a[D_], b[D_];
                load_x<D_>(q, (size_t)row_here, a);
                load_x<D_>(q, (size_t)row_here + 1, b);
                const float f = (float)i * inv_m;
#pragma unroll
                for (int j = 0; j < D_; ++j) x[j] = i == 0 ? a[j] : (i == M ? b[j] : CPPF_FMA(f, b[j] - a[j], a[j]));
            }
            float R[9], p[3], blo[3], bhi[3];
            wave_capsule_box<RB>(rb, co, x, caps, R, p, blo, bhi);
            // the self pairs and the cuboids, all of them: the node test of motion_kernel itself
            int fail = far_fail;
            float m = INFINITY;  // the node's smallest clearance, untruncated
            motion_node_test<RB>(caps, rk.cull, rk.rho, dq, slam, inv_m, true, 0, rk.cull.n_obs, lane, blo, bhi, m, fail);

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
