// kernels_scene.h -- obstacle scenes: all rows against up to CPPF_MAX_SCENE_OBSTACLES axis-aligned cuboids held in DEVICE memory
// (cppf_scene_env_collisions).  Included inside the anonymous namespace of cppflow_hip.hip; gfx950 only.
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

struct SceneK {
    const float* box_lo;  // DEVICE [n_obs, 3] world-frame corners
    const float* box_hi;
    unsigned long long* row_key;  // workspace: [n] 64-bit keys, then [n_obs] 32-bit keys
    uint32_t* obs_key;            // NULL: obs_min was not asked for (no cross-lane reduction)
    int32_t n, n_obs, chunk;      // chunk: cuboids per blockIdx.y, a multiple of 8
    float reach;                  // (0 for a mask-only launch)
    float tile_cull2;             // (r_max + reach + 1 cm)^2 (1 + 1e-4), rounded up: wavefront box vs cuboid
    float cull2[CPPF_MAX_CAPSULES];  // (h + r + reach + 1 cm)^2 (1 + 1e-4), rounded up: capsule centre vs cuboid
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
template <bool WANT_MIN>
__device__ __forceinline__ void scene_test(const float (&wc)[3], const float (&wh)[3], const float (&lo)[3], const float (&hi)[3],
                                           float cull2, float r, float thr, float& D, int& hit) {
    if (cull_far(point_box_dist2(wc, lo, hi), cull2)) return;
    const float d2 = seg_box_dist2(wc, wh, lo, hi);
    if constexpr (WANT_MIN) {
        const float v = __builtin_sqrtf(d2) - r;
        D = v < D ? v : D;
    } else {
        hit |= d2 < thr;
    }
}

// capsules the specialised form keeps in registers (the generic form stages them in LDS and keeps none)
template <class RB, bool kStatic = RB::kStatic>
struct SceneCaps {
    static constexpr int L = 1;
};
template <class RB>
struct SceneCaps<RB, true> {
    static constexpr int L = RB::Table::L > 0 ? RB::Table::L : 1;
};

template <class RB, bool WANT_MIN>
__global__ __launch_bounds__(kBlock, CPPF_WAVES_COLL) void scene_kernel(const ChainK ch, const CollK co, const SceneK sc,
                                                                         const float* __restrict__ x) {
    extern __shared__ float lds[];
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
    float q[D_], R[9], p[3];
    load_x<D_>(x, row, q);

    constexpr int LS = SceneCaps<RB>::L;
    float swc[LS][3], swh[LS][3];  // (the specialised form's capsules: registers, static indices)
    float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if constexpr (RB::kStatic) {
        capsule_fk_static<RB>(rb, q, R, p, swc, swh);
#pragma unroll
        for (int c = 0; c < RB::Table::L; ++c) box_add_segment(swc[c], swh[c], blo, bhi);
    } else {
        fk_capsules_to_lds<RB>(rb, co, q, lds, tid, R, p);
        for (int c = 0; c < co.ncaps; ++c) {
            float wc[3], wh[3];
            lds_capsule(lds, tid, c, wc, wh);
            box_add_segment(wc, wh, blo, bhi);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        blo[k] = wave_min(blo[k]);
        bhi[k] = wave_max(bhi[k]);
    }

    const int o_begin = (int)blockIdx.y * sc.chunk;
    const int o_end = min(sc.n_obs, o_begin + sc.chunk);
    float best = INFINITY;
    int best_o = -1, hit = 0;
    for (int base = o_begin; base < o_end; base += 64) {
        // 1. 64 cuboids, one per lane, against the wavefront's box
        const int ol = base + lane;
        const bool have = ol < o_end;
        float llo[3], lhi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            llo[k] = have ? sc.box_lo[(size_t)ol * 3 + k] : 0.f;
            lhi[k] = have ? sc.box_hi[(size_t)ol * 3 + k] : 0.f;
        }
        float g2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float g = fmaxf(fmaxf(llo[k] - bhi[k], blo[k] - lhi[k]), 0.f);
            g2 = CPPF_FMA(g, g, g2);
        }
        unsigned long long live = __builtin_amdgcn_ballot_w64(have && !(g2 > sc.tile_cull2));
        // 2. the survivors, one after the other, for the whole wavefront
        while (live != 0ull) {
            const int j = __builtin_ctzll(live);
            live &= live - 1ull;
            const int o = base + j;
            const float lo[3] = {readlane_f(llo[0], j), readlane_f(llo[1], j), readlane_f(llo[2], j)};
            const float hi[3] = {readlane_f(lhi[0], j), readlane_f(lhi[1], j), readlane_f(lhi[2], j)};
            float Dro = INFINITY;
            if constexpr (RB::kStatic) {
                using T = typename RB::Table;
#pragma unroll
                for (int c = 0; c < T::L; ++c)
                    scene_test<WANT_MIN>(swc[c], swh[c], lo, hi, sc.cull2[c], T::cap_r[c], T::cap_thr[c], Dro, hit);
            } else {
                for (int c = 0; c < co.ncaps; ++c) {
                    float wc[3], wh[3];
                    lds_capsule(lds, tid, c, wc, wh);
                    scene_test<WANT_MIN>(wc, wh, lo, hi, sc.cull2[c], co.cap_r[c], co.cap_thr[c], Dro, hit);
                }
            }
            if constexpr (WANT_MIN) {
                if (Dro < best) {  // (strict, cuboids ascending: the lowest index among equals)
                    best = Dro;
                    best_o = o;
                }
                if (sc.obs_key != nullptr && __builtin_amdgcn_ballot_w64(Dro < sc.reach) != 0ull) {
                    const float m = wave_min(Dro);
                    if (lane == 0 && m < sc.reach) atomicMin(&sc.obs_key[o], scene_key(m));
                }
            }
        }
    }
    if (!valid) return;
    if constexpr (WANT_MIN) {
        // (a negative distance is below every legal reach, so the mask read off the key is exact whatever reach is)
        if (best < sc.reach) atomicMin(&sc.row_key[row], ((unsigned long long)scene_key(best) << 32) | (unsigned long long)(uint32_t)best_o);
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
