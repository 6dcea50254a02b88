// kernels_motion.h -- certifying the MOTION between the waypoints of q [S, W, d] collision-free (cppf_motion_clearance): the
// adaptive-clearance test of Schwarzer, Saha and Latombe on 2^level equal intervals per transition, against the robot's self pairs
// and a scene of up to CPPF_MAX_SCENE_OBSTACLES axis-aligned cuboids in DEVICE memory.  Included inside the anonymous namespace of
// cppflow_hip.hip behind kernels_scene.h, whose keys, capsule iterator, wavefront box and scene_walk it shares; gfx950 only.
// motion_self, motion_far_fails and motion_node_test below are the ONE definition of a node's test, for motion_resolve_kernel too.
//
// Definition.
//   Nodes.  Transition t of path s goes from a = q[s,t] to b = q[s,t+1] on the straight line in the STORED joint values (no wrapping:
//   a caller with continuous joints unwraps first).  With M = 2^level: node 0 is a itself, node M is b itself, node i in between is
//   fmaf(i / M, b - a, a) per joint (the subtraction in fp32; i / M is exact).  `nodes` [S, W-1, M+1, d] returns them.
//   Clearances at a node, by the canonical functions only: for a self pair p the value cppf_self_collision_distances gives,
//   sqrt_rn(seg_seg_dist2) - (r_a + r_b); for (capsule c, cuboid o)  min(sqrt_rn(seg_box_dist2) - cap_r[c], reach)  -- truncated at
//   reach, which keeps the scene kernel's culling legal and can only make a certificate harder.
//   Travel bound.  rho[j][c] (host, fp64, rounded UP to fp32: motion_rho_table in cppflow_hip.hip) bounds how far any point of
//   capsule c is from the axis of revolute joint j <= cap_link[c]; 1 for a prismatic joint j <= cap_link[c]; 0 for j > cap_link[c].
//   Against a cuboid  lambda_c = sum_j |b_j - a_j| rho[j][c];  for a self pair (c1, c2) with cap_link l1 <= l2 only the joints in
//   between move one capsule relative to the other:  lambda_p = sum_{l1 < j <= l2} |b_j - a_j| rho[j][c2]  (0 for a pair on one
//   link).  Both are accumulated in fp32, joints ascending, one fmaf each, from 0.  One interval's bound is lambda / M.
//   Verdict per transition.
//     CERTIFIED  every interval (i, i+1), every self pair and every (capsule, cuboid) has  (clear_i + clear_{i+1}) - lambda / M > 1e-6
//                (fp32, in that order), both waypoints lie inside the joint limits (outside them the prismatic term of rho is not a
//                bound) and no node is HIT;
//     HIT        some node has a clearance < 0;   UNDECIDED  neither.
//   status u8: bit 0 CERTIFIED, bit 1 HIT (never both).  min_clear: the minimum over the transition's M + 1 nodes of
//   min(min_self, min_env) as cppf_collision_masks / cppf_scene_env_collisions (the latter at the same reach: +inf beyond it) give
//   them for the node.  hit_node: the lowest node index with a negative clearance, else -1.
//
// Shape.  One node per lane, the nodes of a path in sequence: path s has N = (W-1) M + 1 of them (a waypoint inside the path is node
// M of one transition and node 0 of the next: the same bits), so an interval's partner is the neighbouring lane -- one __shfl_down
// per compared value.  Consecutive wavefronts overlap by one node: wavefront k of a path holds nodes 63 k .. 63 k + 63 and decides
// the 63 intervals between them, so a wavefront needs nobody else (no LDS exchange, no barrier).  Lanes past the last node work on a
// copy of it and store nothing.  The cuboids are cut into chunks over grid.y and walked by scene_walk (kernels_scene.h, "Shape");
// its callback does cull_far, the exact test and the interval comparison, per (capsule, survivor).  Chunk 0 also does the self
// pairs and the joint limits.
// Culling.  A culled cuboid has a clearance >= reach at every node of the wavefront, i.e. the truncated value reach itself: its
// intervals stand or fall by  (reach + reach) - lambda_c / M > 1e-6  alone.  Rounding is monotone, so where that fails every cuboid
// fails for capsule c, culled or not, and where it holds a culled cuboid passes: the test is made ONCE per capsule ahead of the
// tiles (whenever the scene holds a cuboid at all), which makes the verdict independent of what the culling skips.
// Combining.  A transition's intervals and nodes spread over lanes, wavefronts and chunks; they meet in the workspace through
// integer atomics -- OR on the "an interval failed" word, MIN on the order-preserving key of the clearance (scene_key) and on the
// node index of a hit.  The minimum is reduced over the lanes of a transition first (a segmented shuffle reduction).  No float
// atomics, nothing depends on arrival order: two runs are bit-identical.  motion_init_kernel sets the words ahead of the launch,
// motion_finish_kernel decodes them behind it; ordering is the stream's, no kernel waits on another.
#pragma once

struct MotionK {
    SceneCullK cull;      // the scene and its culling thresholds (kernels_scene.h)
    const float* rho;     // DEVICE [CPPF_MAX_DOF][CPPF_MAX_CAPSULES] (the handle's table)
    uint32_t* fail;       // workspace [S (W-1)]: non-zero = some interval of the transition is not certified
    uint32_t* clear_key;  // workspace [S (W-1)]: scene_key of the smallest node clearance
    int32_t* hit;         // workspace [S (W-1)]: the lowest node with a negative clearance (INT32_MAX: none)
    float* nodes;         // [S, W-1, M+1, d] or NULL
    int32_t S, W, level, n_nodes, waves_per_path;  // n_nodes = (W-1) 2^level + 1 per path; ceil((n_nodes - 1) / 63) wavefronts
    int32_t chunk;                                 // cuboids per blockIdx.y, a multiple of 8
    float inv_m;                                   // 2^-level
};

constexpr float kMotionSlack = 1e-6f;

// one interval: this lane's node and its right neighbour's against the travel bound (a NaN anywhere does not certify)
__device__ __forceinline__ int motion_interval_fails(float v, float lam, float inv_m) {
    const float w = __shfl_down(v, 1, 64);
    return !((v + w) - lam * inv_m > kMotionSlack);
}

// lambda over the joints lo_link < j <= hi_link for the capsule `c` (wave-uniform bounds: the branch is scalar, dq is indexed statically)
template <int D>
__device__ __forceinline__ float motion_lambda(const float* __restrict__ rho, const float (&dq)[D], int lo_link, int hi_link, int c) {
    float lam = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j)
        if (j > lo_link && j <= hi_link) lam = CPPF_FMA(dq[j], rho[j * CPPF_MAX_CAPSULES + c], lam);
    return lam;
}

// lambda_p of the self pair of capsules a, b on the links la, lb: the joints between the two links, the further capsule's bounds
template <int D>
__device__ __forceinline__ float motion_pair_lambda(const float* __restrict__ rho, const float (&dq)[D], int la, int lb, int a, int b) {
    return la <= lb ? motion_lambda<D>(rho, dq, la, lb, b) : motion_lambda<D>(rho, dq, lb, la, a);
}

// the self pairs [B, E) of a generated table: capsule and link ids are compile-time.  Ranges of more than 24 pairs are halved: one
// fully unrolled loop over all 55 pairs of Chain12 is beyond what the compiler unrolls, and a loop it leaves rolled indexes the
// capsules' registers at run time
template <class RB, int B, int E>
__device__ __forceinline__ void motion_self_static(const LaneCaps<RB, true>& caps, const float* __restrict__ rho,
                                                   const float (&dq)[RB::D], float inv_m, float& m, int& fail) {
    if constexpr (E - B > 24) {
        motion_self_static<RB, B, (B + E) / 2>(caps, rho, dq, inv_m, m, fail);
        motion_self_static<RB, (B + E) / 2, E>(caps, rho, dq, inv_m, m, fail);
    } else {
        using T = typename RB::Table;
#pragma unroll
        for (int pi = B; pi < E; ++pi) {
            const int a = T::pair_a[pi], b = T::pair_b[pi];
            const float d2 = seg_seg_dist2(caps.wc[a], caps.wh[a], caps.wc[b], caps.wh[b], T::cap_a[a], T::cap_ia[a], T::cap_a[b], T::cap_ia[b]);
            const float v = __builtin_sqrtf(d2) - (T::cap_r[a] + T::cap_r[b]);
            m = v < m ? v : m;
            fail |= motion_interval_fails(v, motion_pair_lambda<RB::D>(rho, dq, T::cap_link[a], T::cap_link[b], a, b), inv_m);
        }
    }
}
// every self pair of this lane's node: the generated table's, or CollK's over the capsules in LDS
template <class RB>
__device__ __forceinline__ void motion_self(const LaneCaps<RB>& caps, const float* __restrict__ rho, const float (&dq)[RB::D],
                                            float inv_m, float& m, int& fail) {
    if constexpr (RB::kStatic) {
        motion_self_static<RB, 0, RB::Table::P>(caps, rho, dq, inv_m, m, fail);
    } else {
        extern __shared__ float lds[];
        const CollK& co = caps.co;
        for (int pi = 0; pi < co.npairs; ++pi) {
            const int a = co.pair_a[pi], b = co.pair_b[pi];
            float ca[3], ha[3], cb[3], hb[3];
            lds_capsule(lds, caps.tid, a, ca, ha);
            lds_capsule(lds, caps.tid, b, cb, hb);
            const float d2 = seg_seg_dist2(ca, ha, cb, hb, co.cap_a[a], co.cap_ia[a], co.cap_a[b], co.cap_ia[b]);
            const float v = __builtin_sqrtf(d2) - (co.cap_r[a] + co.cap_r[b]);
            m = v < m ? v : m;
            fail |= motion_interval_fails(v, motion_pair_lambda<RB::D>(rho, dq, co.cap_link[a], co.cap_link[b], a, b), inv_m);
        }
    }
}

// lambda_c of every capsule against a cuboid.  The specialised form keeps them (slam); the generic one forms each where it is used.
template <class RB>
__device__ __forceinline__ void motion_cuboid_lambdas(const float* __restrict__ rho, const float (&dq)[RB::D],
                                                      float (&slam)[LaneCaps<RB>::L]) {
    if constexpr (RB::kStatic) {
        using T = typename RB::Table;
#pragma unroll
        for (int c = 0; c < T::L; ++c) slam[c] = motion_lambda<RB::D>(rho, dq, -1, T::cap_link[c], c);
    }
}
template <class RB, class Cap>
__device__ __forceinline__ float motion_cuboid_lambda(const float* __restrict__ rho, const float (&dq)[RB::D],
                                                      const float (&slam)[LaneCaps<RB>::L], const Cap& cap) {
    if constexpr (RB::kStatic)
        return slam[cap.c];
    else
        return motion_lambda<RB::D>(rho, dq, -1, cap.link(), cap.c);
}

// every cuboid the culling skips (see "Culling"): reach at both ends of the interval.  Depends on the level alone, not on a node:
// a caller evaluates it once and ORs it into the verdict of every interval (whenever the scene holds a cuboid at all).
template <class RB>
__device__ __forceinline__ int motion_far_fails(const LaneCaps<RB>& caps, const float* __restrict__ rho, const float (&dq)[RB::D],
                                                const float (&slam)[LaneCaps<RB>::L], float reach, float inv_m) {
    int fail = 0;
    caps.each([&](const auto& cap) { fail |= !((reach + reach) - motion_cuboid_lambda<RB>(rho, dq, slam, cap) * inv_m > kMotionSlack); });
    return fail;
}

// This lane's node (its capsules in `caps`, their box in blo / bhi, not yet reduced) against the self pairs (where `self`) and the
// cuboids [o_begin, o_end) of the scene: its smallest clearance into m, the verdict of its interval ORed into fail -- which the
// caller seeds with motion_far_fails.  The ONE definition of the node test: motion_kernel and motion_resolve_kernel agree bit for
// bit because both call it.
template <class RB>
__device__ __forceinline__ void motion_node_test(const LaneCaps<RB>& caps, const SceneCullK& sc, const float* __restrict__ rho,
                                                 const float (&dq)[RB::D], const float (&slam)[LaneCaps<RB>::L], float inv_m, bool self,
                                                 int o_begin, int o_end, int lane, float (&blo)[3], float (&bhi)[3], float& m, int& fail) {
    if (self) motion_self<RB>(caps, rho, dq, inv_m, m, fail);
    if (sc.n_obs > 0) {
        wave_box_reduce(blo, bhi);
        float best = INFINITY;
        scene_walk(sc, o_begin, o_end, lane, blo, bhi, [&](int, const float (&lo)[3], const float (&hi)[3]) {
            caps.each([&](const auto& cap) {
                if (cull_far(point_box_dist2(cap.wc, lo, hi), sc.cull2[cap.c])) return;
                const float v = __builtin_sqrtf(seg_box_dist2(cap.wc, cap.wh, lo, hi)) - cap.r();
                best = v < best ? v : best;
                fail |= motion_interval_fails(v < sc.reach ? v : sc.reach, motion_cuboid_lambda<RB>(rho, dq, slam, cap), inv_m);
            });
        });
        if (best < sc.reach) m = best < m ? best : m;  // (min_env as the scene kernel reports it: nothing beyond reach)
    }
}

template <class RB>
__global__ __launch_bounds__(kBlock, CPPF_WAVES_COLL) void motion_kernel(const ChainK ch, const CollK co, const MotionK mk,
                                                                          const float* __restrict__ q) {
    constexpr int D_ = RB::D;
    const RB rb{ch, co};
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t wave = (size_t)blockIdx.x * (kBlock / 64) + (size_t)(tid >> 6);
    if (wave >= (size_t)mk.S * (size_t)mk.waves_per_path) return;  // (wave-uniform)
    const int s = (int)(wave / (size_t)mk.waves_per_path);
    const int k = (int)(wave - (size_t)s * (size_t)mk.waves_per_path);
    const int last = mk.n_nodes - 1, M = 1 << mk.level;
    const int g0 = 63 * k + lane;
    const bool valid = g0 <= last;
    const int g = valid ? g0 : last;            // (a lane past the end: a copy of the last node)
    const int t = min(g >> mk.level, mk.W - 2);  // the node's transition -- and, where the lane has one, its interval's
    const int i = g - (t << mk.level);           // 0 .. M (M only at the end of the path)
    const bool has_interval = lane < 63 && g0 < last;
    const size_t tr = (size_t)s * (size_t)(mk.W - 1) + (size_t)t;

    float x[D_], dq[D_];
    int outside = 0;
    {
        float a[D_], b[D_];
        load_x<D_>(q, (size_t)s * (size_t)mk.W + (size_t)t, a);
        load_x<D_>(q, (size_t)s * (size_t)mk.W + (size_t)t + 1, b);
        const float f = (float)i * mk.inv_m;
#pragma unroll
        for (int j = 0; j < D_; ++j) {
            const float d = b[j] - a[j];
            x[j] = i == 0 ? a[j] : (i == M ? b[j] : CPPF_FMA(f, d, a[j]));
            dq[j] = fabsf(d);
            outside |= !(a[j] >= rb.lo(j) && a[j] <= rb.hi(j)) | !(b[j] >= rb.lo(j) && b[j] <= rb.hi(j));
        }
    }
    if (mk.nodes != nullptr && valid && blockIdx.y == 0) {
        float* o = mk.nodes + (tr * (size_t)(M + 1) + (size_t)i) * D_;
#pragma unroll
        for (int j = 0; j < D_; ++j) o[j] = x[j];
        if (i == 0 && t > 0) {  // the waypoint is node M of the transition before as well
            float* e = mk.nodes + ((tr - 1) * (size_t)(M + 1) + (size_t)M) * D_;
#pragma unroll
            for (int j = 0; j < D_; ++j) e[j] = x[j];
        }
    }

    LaneCaps<RB> caps(co, tid);
    float R[9], p[3], blo[3], bhi[3];
    wave_capsule_box<RB>(rb, co, x, caps, R, p, blo, bhi);

    // every chunk: the far-cuboid rule; chunk 0 also the joint limits and the self pairs
    int fail = 0;
    float m = INFINITY;  // the node's smallest clearance, untruncated
    float slam[LaneCaps<RB>::L];
    if (mk.cull.n_obs > 0) {
        motion_cuboid_lambdas<RB>(mk.rho, dq, slam);
        fail |= motion_far_fails<RB>(caps, mk.rho, dq, slam, mk.cull.reach, mk.inv_m);
    }
    if (blockIdx.y == 0) fail |= outside;
    const int o_begin = (int)blockIdx.y * mk.chunk;
    motion_node_test<RB>(caps, mk.cull, mk.rho, dq, slam, mk.inv_m, blockIdx.y == 0, o_begin, min(mk.cull.n_obs, o_begin + mk.chunk), lane,
                         blo, bhi, m, fail);

    // ---- meet the other lanes, wavefronts and chunks of the transition ------------------------------------------------------------------
    // (a lane past the end holds a copy of the last node: what it adds to a minimum the last node adds as well)
    if (has_interval && fail) atomicOr(&mk.fail[tr], 1u);
    if (m < 0.f) {
        atomicMin(&mk.hit[tr], i);
        if (i == 0 && t > 0) atomicMin(&mk.hit[tr - 1], M);
    }
    uint32_t key = scene_key(m);
    if (i == 0 && t > 0 && m < INFINITY) atomicMin(&mk.clear_key[tr - 1], key);
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {  // minimum over the lanes of one transition (t does not decrease along the lanes)
        const uint32_t ok = (uint32_t)__shfl_down((int)key, sft, 64);
        const int ot = __shfl_down(t, sft, 64);
        if (lane + sft < 64 && ot == t && ok < key) key = ok;
    }
    const int tp = __shfl_up(t, 1, 64);
    if ((lane == 0 || tp != t) && key < scene_key(INFINITY)) atomicMin(&mk.clear_key[tr], key);
}

// the workspace's words: fail = 0, clear_key = all-ones ("nothing finite"), hit = INT32_MAX
__global__ __launch_bounds__(256) void motion_init_kernel(uint32_t* __restrict__ fail, uint32_t* __restrict__ clear_key,
                                                          int32_t* __restrict__ hit, size_t n_tr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_tr) {
        fail[i] = 0u;
        clear_key[i] = ~0u;
        hit[i] = 0x7fffffff;
    }
}

__global__ __launch_bounds__(256) void motion_finish_kernel(const uint32_t* __restrict__ fail, const uint32_t* __restrict__ clear_key,
                                                            const int32_t* __restrict__ hit, size_t n_tr, uint8_t* __restrict__ status,
                                                            float* __restrict__ min_clear, int32_t* __restrict__ hit_node) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tr) return;
    const bool is_hit = hit[i] != 0x7fffffff;
    status[i] = (uint8_t)((fail[i] == 0u && !is_hit ? 1 : 0) | (is_hit ? 2 : 0));
    if (min_clear) min_clear[i] = clear_key[i] == ~0u ? INFINITY : scene_unkey(clear_key[i]);
    if (hit_node) hit_node[i] = is_hit ? hit[i] : -1;
}
