// kernels_scene.h -- obstacle scenes: all rows against up to CPPF_MAX_SCENE_OBSTACLES axis-aligned cuboids held in DEVICE memory
// (cppf_scene_env_collisions), and what EVERY kernel that tests capsules against such a scene shares -- the coupled step's scene form
// (kernels_coupled.h) and the two motion kernels (kernels_motion.h, kernels_motion_resolve.h) include behind this file:
//   SceneCullK        the scene and its culling thresholds (host: scene_cull_setup)
//   LaneCaps          this lane's capsules behind one loop, generated table + registers or CollK + LDS
//   wave_capsule_box  capsule FK, then the lane's box; wave_box_reduce makes it the wavefront's
//   scene_tile        "Shape" 1. below;   scene_walk  the tile loop and "Shape" 2.: f(o, lo, hi) per surviving cuboid, ascending
// The arguments "Shape", "Culling" (the truncation at reach) and "Combining" are stated here once; the other files refer to them.
// Included inside the anonymous namespace of cppflow_hip.hip; gfx950 only.
//
// Every number is the one collide_*<WANT_MIN = true> produces for a (row, capsule, cuboid): the capsule FK is fk_capsules_to_lds /
// capsule_fk_static, the distance sqrt_rn(seg_box_dist2) - cap_r[c], the mask-only form d2 < cap_thr[c].  With
//     d(r,c,o) that value,  D(r,o) = min_c d(r,c,o)
// the launch reports  env_mask[r] = any_o D(r,o) < 0,  min_env[r] = min_o D(r,o) where that is < reach (else +inf),  nearest_obs[r]
// = the lowest o attaining a finite min_env[r] (else -1),  obs_min[o] = min_r D(r,o) where that is < reach (else +inf).
//
// Shape.  grid = (256-row workgroups, chunks of cuboids): one row per lane as everywhere else, and the cuboids split over the second
// grid dimension, because one plan's few hundred rows cannot fill the chip by themselves.  A workgroup repeats the capsule FK of its
// rows (cheap next to a chunk of exact tests) and walks its chunk up to 64 cuboids at a time (the host cuts chunks in groups of 8:
// as many as it takes to give every SIMD four wavefronts, cppf_scene_env_collisions):
//   1. lane l holds cuboid base + l and tests it against the WAVEFRONT's box -- the bounding box of every capsule segment of every
//      row of the wavefront.  A segment lies in that box, so dist(segment, cuboid) >= dist(box, cuboid); a cuboid further from the
//      box than  r_max + reach + 1 cm  (squared, x (1 + 1e-4), rounded up: cull_threshold on the host) has d > reach for every
//      (row, capsule) of the wavefront and is skipped.  A ballot gives the survivors; an empty ballot skips the tile.
//   2. a wave-uniform loop over the set bits broadcasts the survivor's corners out of lane j's registers (v_readlane: they become
//      wave-uniform scalars, like the CollK tables of the other kernels) and runs, per capsule, the bounding-sphere test of cull_far
//      with the threshold (h + r + reach + 1 cm)^2 (1 + 1e-4) and then the exact test.
// Distances are truncated at `reach`, which is what makes the culling legal: whatever is skipped has d > reach, is not negative (the
// mask) and cannot be a minimum that is reported.  reach = +inf culls nothing; a mask-only call culls with reach = 0, i.e. with
// exactly cap_cull[] of the existing mask-only launches.
//
// Combining.  Chunks (and, for obs_min, wavefronts) meet in the caller's workspace through unsigned integer atomic MIN on keys
// that order like the floats they encode -- per row a 64-bit key { distance key : cuboid index }, whose minimum is the smallest
// distance and among equals the lowest index; per cuboid a 32-bit distance key.  min is associative and commutative on integers,
// so the result does not depend on which workgroup arrives first, how rows share a wavefront, or how the host cut the chunks: two
// runs are bit-identical.  No float atomic arithmetic.  The workspace is set to all-ones (the "nothing within reach" key) by
// scene_init_kernel ahead of the launch and decoded by scene_finish_kernel behind it; ordering is the stream's, no kernel waits on
// another.
#pragma once

// the culling arguments of a walk over a scene (scene_cull_setup in cppflow_hip.hip fills them); embedded in SceneK, MotionK, ResolveK
struct SceneCullK {
    const float* box_lo;  // DEVICE [n_obs, 3] world-frame corners
    const float* box_hi;
    int32_t n_obs;
    float reach;                     // (0 for a mask-only launch)
    float tile_cull2;                // (r_max + reach + 1 cm)^2 (1 + 1e-4), rounded up: wavefront box vs cuboid
    float cull2[CPPF_MAX_CAPSULES];  // (h + r + reach + 1 cm)^2 (1 + 1e-4), rounded up: capsule centre vs cuboid
};

struct SceneK {
    SceneCullK cull;
    unsigned long long* row_key;  // workspace: [n] 64-bit keys, then [n_obs] 32-bit keys
    uint32_t* obs_key;            // NULL: obs_min was not asked for (no cross-lane reduction)
    int32_t n, chunk;             // chunk: cuboids per blockIdx.y, a multiple of 8
};

// float -> unsigned key with  a < b  <=>  key(a) < key(b)  (no NaN reaches here: a NaN distance never passes "v < m")
__device__ __forceinline__ uint32_t scene_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float scene_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fminf(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
    return v;
}

__device__ __forceinline__ float readlane_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// grow the box [blo, bhi] by the segment { c + u h, |u| <= 1 }
__device__ __forceinline__ void box_add_segment(const float (&c)[3], const float (&h)[3], float (&blo)[3], float (&bhi)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = fabsf(h[k]);
        blo[k] = fminf(blo[k], c[k] - a);
        bhi[k] = fmaxf(bhi[k], c[k] + a);
    }
}

// one (capsule, cuboid): bounding-sphere cull on the centre, then the exact test.  WANT_MIN: D = min(D, sqrt(d2) - r); else hit |= d2 < thr
template <bool WANT_MIN, class Cap>
__device__ __forceinline__ void scene_test(const Cap& cap, const float (&lo)[3], const float (&hi)[3], float cull2, float& D, int& hit) {
    if (cull_far(point_box_dist2(cap.wc, lo, hi), cull2)) return;
    const float d2 = seg_box_dist2(cap.wc, cap.wh, lo, hi);
    if constexpr (WANT_MIN) {
        const float v = __builtin_sqrtf(d2) - cap.r();
        D = v < D ? v : D;
    } else {
        hit |= d2 < cap.thr();
    }
}

// This lane's capsules behind one loop: the specialised form keeps them in registers and reads radius, threshold and link from
// the generated table, everything indexed at compile time; the generic form (kStatic = false, whatever the robot: it needs CollK
// and the lane's LDS slots alone) stages them in LDS.  each(f) calls f(cap) for the capsules in ascending order: cap.c the index (a
// constant expression in the specialised form), cap.wc / cap.wh centre and half-axis, cap.r() / cap.thr() / cap.link() radius,
// mask threshold and link -- read where they are asked for, as the loops this replaces did.
template <class RB, bool kStatic = RB::kStatic>
struct LaneCaps {
    static constexpr int L = 1;  // (capsules held in registers: none)
    struct Cap {
        const CollK& co;
        int c;
        float wc[3], wh[3];
        __device__ __forceinline__ float r() const { return co.cap_r[c]; }
        __device__ __forceinline__ float thr() const { return co.cap_thr[c]; }
        __device__ __forceinline__ int link() const { return co.cap_link[c]; }
    };
    const CollK& co;
    int tid;
    __device__ __forceinline__ LaneCaps(const CollK& co_, int tid_) : co(co_), tid(tid_) {}
    __device__ __forceinline__ void fk(const RB& rb, const CollK& co, const float (&q)[RB::D], float (&R)[9], float (&p)[3]) {
        extern __shared__ float lds[];
        fk_capsules_to_lds<RB>(rb, co, q, lds, tid, R, p);  // (co: the kernel's own argument -- through this->co the FK costs 4 VGPRs)
    }
    template <class F>
    __device__ __forceinline__ void each(F&& f) const {
        extern __shared__ float lds[];
        for (int c = 0; c < co.ncaps; ++c) {
            Cap cap{co, c};
            lds_capsule(lds, tid, c, cap.wc, cap.wh);
            f(cap);
        }
    }
};
template <class RB>
struct LaneCaps<RB, true> {
    using T = typename RB::Table;
    static constexpr int L = T::L > 0 ? T::L : 1;
    template <int C>
    struct Cap {
        static constexpr int c = C;
        const float (&wc)[3];
        const float (&wh)[3];
        static __device__ __forceinline__ float r() { return T::cap_r[C]; }
        static __device__ __forceinline__ float thr() { return T::cap_thr[C]; }
        static __device__ __forceinline__ int link() { return T::cap_link[C]; }
    };
    float wc[L][3], wh[L][3];
    __device__ __forceinline__ LaneCaps(const CollK&, int) {}
    __device__ __forceinline__ void fk(const RB& rb, const CollK& co, const float (&q)[RB::D], float (&R)[9], float (&p)[3]) {
        capsule_fk_static<RB>(rb, q, R, p, wc, wh);
    }
    template <class F, int... C>
    __device__ __forceinline__ void each_of(F&& f, std::integer_sequence<int, C...>) const {
        (f(Cap<C>{wc[C], wh[C]}), ...);
    }
    template <class F>
    __device__ __forceinline__ void each(F&& f) const {
        each_of(f, std::make_integer_sequence<int, T::L>{});
    }
};

// the box of every capsule segment of this lane ...
template <class Caps>
__device__ __forceinline__ void capsule_box(const Caps& caps, float (&blo)[3], float (&bhi)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) blo[k] = INFINITY, bhi[k] = -INFINITY;
    caps.each([&](const auto& cap) { box_add_segment(cap.wc, cap.wh, blo, bhi); });
}
// ... and of every lane of the wavefront ("Shape", 1.; all 64 lanes must be here)
__device__ __forceinline__ void wave_box_reduce(float (&blo)[3], float (&bhi)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        blo[k] = wave_min(blo[k]);
        bhi[k] = wave_max(bhi[k]);
    }
}
// capsule FK of this lane's configuration into `caps` (R, p: the last link's frame; the caller's, because arrays of this function's
// own cost the generic kernels 2 .. 4 VGPRs), then the lane's box (a caller reduces it only where it walks a scene)
template <class RB>
__device__ __forceinline__ void wave_capsule_box(const RB& rb, const CollK& co, const float (&q)[RB::D], LaneCaps<RB>& caps, float (&R)[9],
                                                 float (&p)[3], float (&blo)[3], float (&bhi)[3]) {
    caps.fk(rb, co, q, R, p);
    capsule_box(caps, blo, bhi);
}

// "Shape", 1.: the cuboids base + lane < o_end, one per lane (corners into llo / lhi), against the wavefront's box -> the ballot of
// the lanes whose cuboid may come within the tile threshold of it
__device__ __forceinline__ unsigned long long scene_tile(const float* __restrict__ box_lo, const float* __restrict__ box_hi, int o_end,
                                                         float tile_cull2, int base, int lane, const float (&blo)[3],
                                                         const float (&bhi)[3], float (&llo)[3], float (&lhi)[3]) {
    const int ol = base + lane;
    const bool have = ol < o_end;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        llo[k] = have ? box_lo[(size_t)ol * 3 + k] : 0.f;
        lhi[k] = have ? box_hi[(size_t)ol * 3 + k] : 0.f;
    }
    float g2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float g = fmaxf(fmaxf(llo[k] - bhi[k], blo[k] - lhi[k]), 0.f);
        g2 = CPPF_FMA(g, g, g2);
    }
    return __builtin_amdgcn_ballot_w64(have && !(g2 > tile_cull2));
}

// The walk over the cuboids [o_begin, o_end): 64 at a time through scene_tile (tiles for which near(base) is false are not even
// read), then "Shape", 2.: f(o, lo, hi) once per surviving cuboid, for the whole wavefront (o, lo, hi are wave-uniform), cuboids
// ASCENDING -- the tie rule of scene_kernel and the bit-for-bit promise of the coupled step's scene form rest on that order.
template <class Near, class F>
__device__ __forceinline__ void scene_walk(const float* __restrict__ box_lo, const float* __restrict__ box_hi, int o_begin, int o_end,
                                           float tile_cull2, int lane, const float (&blo)[3], const float (&bhi)[3], Near&& near,
                                           F&& f) {
    for (int base = o_begin; base < o_end; base += 64) {
        if (!near(base)) continue;
        float llo[3], lhi[3];
        unsigned long long live = scene_tile(box_lo, box_hi, o_end, tile_cull2, base, lane, blo, bhi, llo, lhi);
        while (live != 0ull) {
            const int j = __builtin_ctzll(live);
            live &= live - 1ull;
            const float lo[3] = {readlane_f(llo[0], j), readlane_f(llo[1], j), readlane_f(llo[2], j)};
            const float hi[3] = {readlane_f(lhi[0], j), readlane_f(lhi[1], j), readlane_f(lhi[2], j)};
            f(base + j, lo, hi);
        }
    }
}
template <class F>
__device__ __forceinline__ void scene_walk(const SceneCullK& sc, int o_begin, int o_end, int lane, const float (&blo)[3],
                                           const float (&bhi)[3], F&& f) {
    scene_walk(sc.box_lo, sc.box_hi, o_begin, o_end, sc.tile_cull2, lane, blo, bhi, [](int) { return true; }, f);
}

template <class RB, bool WANT_MIN>
__global__ __launch_bounds__(kBlock, CPPF_WAVES_COLL) void scene_kernel(const ChainK ch, const CollK co, const SceneK sc,
                                                                         const float* __restrict__ x) {
    constexpr int D_ = RB::D;
    const RB rb{ch, co};
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t row0 = (size_t)blockIdx.x * kBlock + tid;
    // a wavefront with no row at all leaves (wave-uniform: row0 - lane is its first row); a lane past the end of a partly filled
    // one stays, because the tile test needs all 64 lanes, and works on a copy of the last row -- whatever a ballot or a wavefront
    // minimum sees of it, a real row shows as well -- but reports nothing
    if (row0 - (size_t)lane >= (size_t)sc.n) return;
    const bool valid = row0 < (size_t)sc.n;
    const size_t row = valid ? row0 : (size_t)sc.n - 1;
    float q[D_];
    load_x<D_>(x, row, q);

    LaneCaps<RB> caps(co, tid);
    float R[9], p[3], blo[3], bhi[3];
    wave_capsule_box<RB>(rb, co, q, caps, R, p, blo, bhi);
    wave_box_reduce(blo, bhi);

    const int o_begin = (int)blockIdx.y * sc.chunk;
    const int o_end = min(sc.cull.n_obs, o_begin + sc.chunk);
    float best = INFINITY;
    int best_o = -1, hit = 0;
    scene_walk(sc.cull, o_begin, o_end, lane, blo, bhi, [&](int o, const float (&lo)[3], const float (&hi)[3]) {
        float Dro = INFINITY;
        caps.each([&](const auto& cap) { scene_test<WANT_MIN>(cap, lo, hi, sc.cull.cull2[cap.c], Dro, hit); });
        if constexpr (WANT_MIN) {
            if (Dro < best) {  // (strict, cuboids ascending: the lowest index among equals)
                best = Dro;
                best_o = o;
            }
            if (sc.obs_key != nullptr && __builtin_amdgcn_ballot_w64(Dro < sc.cull.reach) != 0ull) {
                const float m = wave_min(Dro);
                if (lane == 0 && m < sc.cull.reach) atomicMin(&sc.obs_key[o], scene_key(m));
            }
        }
    });
    if (!valid) return;
    if constexpr (WANT_MIN) {
        // (a negative distance is below every legal reach, so the mask read off the key is exact whatever reach is)
        if (best < sc.cull.reach) atomicMin(&sc.row_key[row], ((unsigned long long)scene_key(best) << 32) | (unsigned long long)(uint32_t)best_o);
    } else {
        if (hit) atomicMin(&sc.row_key[row], 0ull);
    }
}

// every key of the workspace (as 32-bit words: two per row, one per cuboid) to all-ones
__global__ __launch_bounds__(256) void scene_init_kernel(uint32_t* __restrict__ words, size_t n_words) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) words[i] = ~0u;
}

// keys -> outputs.  One thread per row and per cuboid; want_min = 0: the keys of a mask-only launch (0 = hit).
__global__ __launch_bounds__(256) void scene_finish_kernel(const unsigned long long* __restrict__ row_key,
                                                           const uint32_t* __restrict__ obs_key, int n, int n_obs, int want_min,
                                                           uint8_t* __restrict__ env_mask, float* __restrict__ min_env,
                                                           int32_t* __restrict__ nearest_obs, float* __restrict__ obs_min) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) {
        const unsigned long long k = row_key[i];
        const bool none = k == ~0ull;
        const float m = (none || !want_min) ? INFINITY : scene_unkey((uint32_t)(k >> 32));
        env_mask[i] = (uint8_t)(want_min ? (m < 0.f) : !none);
        if (min_env) min_env[i] = m;
        if (nearest_obs) nearest_obs[i] = none ? -1 : (int32_t)(uint32_t)(k & 0xffffffffull);
    }
    if (obs_min != nullptr && i < (size_t)n_obs) {
        const uint32_t k = obs_key[i];
        obs_min[i] = k == ~0u ? INFINITY : scene_unkey(k);
    }
}
