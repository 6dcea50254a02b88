// kernels_voxel.h -- obstacle scenes FROM SENSOR DATA: a point cloud or a depth image becomes the box_lo / box_hi list the scene
// kernels read (cppf_scene_from_points, cppf_scene_from_depth; the definitions are in include/cppflow_hip.h, "Scenes from sensor
// data", and restated in NumPy float32 by tests/voxel_scene.py).  Included inside the anonymous namespace of cppflow_hip.hip behind
// kernels_scene.h; gfx950 only.
//
// Six launches on the caller's stream, each ordered behind the one before by the stream alone:
//   voxel_clear_kernel      the bitset, the per-row counts and offsets, counts[0..7] to zero
//   voxel_self_kernel       (n_self > 0 only) one lane per configuration of q_self: the generic capsule FK -- the operation order of
//                           fk_capsules_to_lds -- to { C, H, 1 / H.H, thr2 } per (configuration, capsule) in the workspace
//   voxel_points_kernel     one input per lane: class, cell, one 64-bit atomic OR of the cell's bit unless a plain load shows it set;
//                           the four class counters by a ballot and a population count per wavefront into LDS, one integer
//                           atomic add per WORKGROUP and class
//   voxel_rows_kernel       one lane per row (y, z): its heads (runs that row y - 1 does not repeat identically) and its cells
//   voxel_scan_kernel       ONE workgroup: the exclusive prefix sum of the head counts in (z, y) order and counts[0..2]
//   voxel_emit_kernel       the same walk as voxel_rows_kernel; a head follows its run down y + 1, ... and stores its box at its offset
// The only atomics are integer OR (idempotent) and integer add (associative, commutative): the bitset and the counters do not
// depend on the order of arrival, and everything behind them is a function of the bitset, so two runs give the same bytes.
//
// Bitset: row (y, z) is wpr = ceil(nx / 64) 64-bit words at (z ny + y) wpr; bit x & 63 of word x >> 6 is cell x.  Bits at x >= nx
// are never set (a kept point has ix < nx), which is what lets a run that reaches the row's end stop at nx in every row alike.
#pragma once

struct VoxelK {
    float origin[3];
    float voxel, inv_voxel;  // inv_voxel = fp32 1 / voxel (host): the index ESTIMATE only, the planes decide
    int32_t nx, ny, nz;
    int32_t wpr, rows;  // words per row; rows = ny nz <= 2^18
    unsigned long long* bits;  // [rows wpr]
    int32_t* row_heads;        // [rows]
    int32_t* row_cells;        // [rows]
    int32_t* row_offset;       // [rows] exclusive prefix of row_heads
    const float* segs;         // [n_self ncaps][8]: C, H, 1 / H.H (0 for a sphere), thr2
    int32_t n_self, ncaps;
    int32_t capacity;
    int32_t* counts;  // [8]
    float* box_lo;
    float* box_hi;
};

// what voxel_self_kernel needs beside the robot: where the rows of q_self are and thr2[c] = fp32((r_c + margin)^2) (host, fp64)
struct VoxelSelfK {
    const float* q;
    float* segs;
    int32_t n_self;
    float thr2[CPPF_MAX_CAPSULES];
};

// the depth form's camera (host: ifx = 1.0f / fx, ify = 1.0f / fy in fp32)
struct VoxelDepthK {
    const float* depth;
    int32_t width;
    float ifx, ify, cx, cy;
    float R[9], t[3];
    float z_min, z_max;
};

// plane i of an axis: two roundings, on purpose not an fmaf (the library is compiled with -ffp-contract=off)
__device__ __forceinline__ float voxel_plane(float origin, float voxel, int i) { return origin + (float)i * voxel; }

// The cell of coordinate p on an axis of n cells: the unique i in [0, n) with P(i) <= p < P(i+1), else -1.  p is finite.  The
// estimate floor((p - o) / v) is clamped BEFORE the integer conversion (p - o may be +-inf) and then walked against the planes
// themselves -- strictly increasing (the host checked), so the walk ends, after at most one step for any sane grid.
__device__ __forceinline__ int voxel_cell(float p, float origin, float voxel, float inv_voxel, int n) {
    const float t = (p - origin) * inv_voxel;
    int i = (int)__builtin_floorf(fminf(fmaxf(t, 0.f), (float)(n - 1)));
    while (i > 0 && p < voxel_plane(origin, voxel, i)) --i;
    while (i < n - 1 && !(p < voxel_plane(origin, voxel, i + 1))) ++i;
    return (p >= voxel_plane(origin, voxel, i) && p < voxel_plane(origin, voxel, i + 1)) ? i : -1;
}

__global__ __launch_bounds__(256) void voxel_clear_kernel(uint4* __restrict__ ws16, size_t n16, int32_t* __restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) ws16[i] = make_uint4(0u, 0u, 0u, 0u);
    if (i < 8) counts[i] = 0;
}

// One lane per configuration.  The frames and the capsule transforms are those of fk_capsules_to_lds, capsule by capsule; only the
// destination differs (the workspace instead of LDS), so C and H are the bits every collision kernel sees for this configuration.
template <class RB>
__global__ __launch_bounds__(64) void voxel_self_kernel(const ChainK ch, const CollK co, const VoxelSelfK sk) {
    const RB rb{ch, co};
    const int cfg = threadIdx.x;
    if (cfg >= sk.n_self) return;
    float q[RB::D];
    load_x<RB::D>(sk.q, (size_t)cfg, q);
    const auto put = [&](int c, const float (&wc)[3], const float (&wh)[3]) {
        const float hh = CPPF_FMA(wh[2], wh[2], CPPF_FMA(wh[1], wh[1], wh[0] * wh[0]));
        float* s = sk.segs + ((size_t)cfg * co.ncaps + c) * 8;
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = wc[k], s[3 + k] = wh[k];
        s[6] = hh >= 1e-30f ? 1.f / hh : 0.f;
        s[7] = sk.thr2[c];
    };
    float R[9], p[3];
    frame_identity(R, p);
    for (int c = co.cap_begin[0]; c < co.cap_begin[1]; ++c) {
        const float wc[3] = {co.cap_c[c][0], co.cap_c[c][1], co.cap_c[c][2]};
        const float wh[3] = {co.cap_h[c][0], co.cap_h[c][1], co.cap_h[c][2]};
        put(c, wc, wh);
    }
#pragma unroll
    for (int j = 0; j < RB::D; ++j) {
        fk_fixed_joint(rb, j, R, p);
        fk_joint(R, p, rb.pris(j), q[j]);
        for (int c = co.cap_begin[j + 1]; c < co.cap_begin[j + 2]; ++c) {
            float wc[3], wh[3];
            xform_point(R, p, co.cap_c[c][0], co.cap_c[c][1], co.cap_c[c][2], wc);
            xform_dir(R, co.cap_h[c][0], co.cap_h[c][1], co.cap_h[c][2], wh);
            put(c, wc, wh);
        }
    }
}

// squared distance of p from the segment { C + u H, |u| <= 1 }: u = clamp(((p - C) . H) (1 / H.H), -1, 1), e = (p - C) - u H, e . e
__device__ __forceinline__ float voxel_point_seg_dist2(const float (&p)[3], const float* __restrict__ s) {
    const float d0 = p[0] - s[0], d1 = p[1] - s[1], d2 = p[2] - s[2];
    const float dh = CPPF_FMA(d2, s[5], CPPF_FMA(d1, s[4], d0 * s[3]));
    const float u = clampf(dh * s[6], -1.f, 1.f);
    const float e0 = CPPF_FMA(-u, s[3], d0), e1 = CPPF_FMA(-u, s[4], d1), e2 = CPPF_FMA(-u, s[5], d2);
    return CPPF_FMA(e2, e2, CPPF_FMA(e1, e1, e0 * e0));
}

__device__ __forceinline__ bool voxel_finite(float x) { return __builtin_fabsf(x) < INFINITY; }  // (false for NaN)

// a class counter of the workgroup (LDS): the wavefront's ballot, its population count, one LDS add by lane 0
__device__ __forceinline__ void voxel_count_class(bool mine, int lane, int* counter) {
    const unsigned long long b = __builtin_amdgcn_ballot_w64(mine);
    if (lane == 0 && b != 0ull) atomicAdd(counter, __builtin_popcountll(b));
}

// DEPTH = false: src = points [n, 3].  DEPTH = true: input i is pixel (row i / width, column i % width) of cam.depth.
// No lane leaves before the ballots and the barriers.
template <bool DEPTH>
__global__ __launch_bounds__(256) void voxel_points_kernel(const VoxelK g, const float* __restrict__ points, const VoxelDepthK cam,
                                                           size_t n) {
    __shared__ int cls[4];  // kept, outside, invalid, self of this workgroup
    if (threadIdx.x < 4) cls[threadIdx.x] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool have = i < n;
    float p[3] = {0.f, 0.f, 0.f};
    bool valid = have;
    if (have) {
        if constexpr (DEPTH) {
            const float z = cam.depth[i];
            valid = z > cam.z_min && z < cam.z_max;  // (a NaN fails both)
            if (valid) {
                const int v = (int)(i / (size_t)cam.width), u = (int)(i - (size_t)v * (size_t)cam.width);
                const float xc = ((float)u - cam.cx) * (z * cam.ifx);
                const float yc = ((float)v - cam.cy) * (z * cam.ify);
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = ((cam.R[3 * k] * xc + cam.R[3 * k + 1] * yc) + cam.R[3 * k + 2] * z) + cam.t[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = points[i * 3 + k];
        }
        valid = valid && voxel_finite(p[0]) && voxel_finite(p[1]) && voxel_finite(p[2]);
    }
    int ix = -1, iy = -1, iz = -1;
    if (valid) {
        ix = voxel_cell(p[0], g.origin[0], g.voxel, g.inv_voxel, g.nx);
        iy = voxel_cell(p[1], g.origin[1], g.voxel, g.inv_voxel, g.ny);
        iz = voxel_cell(p[2], g.origin[2], g.voxel, g.inv_voxel, g.nz);
    }
    const bool inside = valid && ix >= 0 && iy >= 0 && iz >= 0;
    bool self = false;
    if (inside) {
        // (wave-uniform addresses: every lane reads the same record)
        const int n_seg = g.n_self * g.ncaps;
        for (int s = 0; s < n_seg && !self; ++s) {
            const float* rec = g.segs + (size_t)s * 8;
            self = voxel_point_seg_dist2(p, rec) < rec[7];
        }
    }
    const bool kept = inside && !self;
    if (kept) {
        // A cell is hit by many points of a frame (19 in the mean in profiles/voxel_scene.txt), all of them the same atomic on the
        // same word.  A plain load first: a bit only ever goes from 0 to 1 during this launch, so a set bit that is seen is set, and
        // a stale 0 merely sends an OR that changes nothing.
        unsigned long long* const word = &g.bits[((size_t)iz * g.ny + iy) * g.wpr + (ix >> 6)];
        const unsigned long long bit = 1ull << (ix & 63);
        if (!(*word & bit)) atomicOr(word, bit);
    }
    voxel_count_class(kept, lane, &cls[0]);
    voxel_count_class(valid && !inside, lane, &cls[1]);
    voxel_count_class(have && !valid, lane, &cls[2]);
    voxel_count_class(self, lane, &cls[3]);
    // ... and one global add per workgroup and class: per wavefront they queue on four addresses (measured, the same file)
    __syncthreads();
    if (threadIdx.x < 4 && cls[threadIdx.x] != 0) atomicAdd(&g.counts[3 + threadIdx.x], cls[threadIdx.x]);
}

// the first position >= x of a row whose bit equals `set`, else wpr * 64
__device__ __forceinline__ int voxel_next(const unsigned long long* __restrict__ row, int wpr, int x, bool set) {
    int w = x >> 6;
    if (w >= wpr) return wpr * 64;
    unsigned long long m = (set ? row[w] : ~row[w]) & (~0ull << (x & 63));
    while (m == 0ull) {
        if (++w == wpr) return wpr * 64;
        m = set ? row[w] : ~row[w];
    }
    return w * 64 + __builtin_ctzll(m);
}
// does the row hold [x0, x1) as a MAXIMAL run?
__device__ __forceinline__ bool voxel_holds_run(const unsigned long long* __restrict__ row, int wpr, int x0, int x1) {
    if (!((row[x0 >> 6] >> (x0 & 63)) & 1ull)) return false;
    if (x0 > 0 && ((row[(x0 - 1) >> 6] >> ((x0 - 1) & 63)) & 1ull)) return false;
    return voxel_next(row, wpr, x0, false) == x1;
}
// f(k, x0, x1) for the heads of a row in ascending x0, k = 0, 1, ...; prev: row y - 1 (NULL at y = 0).  Returns their number.
template <class F>
__device__ __forceinline__ int voxel_row_heads(const unsigned long long* __restrict__ cur, const unsigned long long* __restrict__ prev,
                                               int wpr, F&& f) {
    int heads = 0;
    const int end = wpr * 64;
    int x0 = voxel_next(cur, wpr, 0, true);
    while (x0 < end) {
        const int x1 = voxel_next(cur, wpr, x0, false);
        if (prev == nullptr || !voxel_holds_run(prev, wpr, x0, x1)) f(heads++, x0, x1);
        x0 = voxel_next(cur, wpr, x1, true);
    }
    return heads;
}

__global__ __launch_bounds__(256) void voxel_rows_kernel(const VoxelK g) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= g.rows) return;
    const int y = r % g.ny;
    const unsigned long long* cur = g.bits + (size_t)r * g.wpr;
    const unsigned long long* prev = y > 0 ? cur - g.wpr : nullptr;
    int cells = 0;
    for (int w = 0; w < g.wpr; ++w) cells += __builtin_popcountll(cur[w]);
    g.row_cells[r] = cells;
    g.row_heads[r] = cells == 0 ? 0 : voxel_row_heads(cur, prev, g.wpr, [](int, int, int) {});
}

// ONE workgroup of 1024 lanes: tiles of 1024 rows in (z, y) order with a running carry; within a tile an inclusive scan per
// wavefront (shuffles), the sixteen wavefront sums through LDS.
__global__ __launch_bounds__(1024) void voxel_scan_kernel(const VoxelK g) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int carry = 0, cells = 0;
    for (int base = 0; base < g.rows; base += 1024) {
        const int i = base + tid;
        const int v = i < g.rows ? g.row_heads[i] : 0;
        cells += i < g.rows ? g.row_cells[i] : 0;
        int inc = v;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int t = __shfl_up(inc, s, 64);
            if (lane >= s) inc += t;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int s = wsum[k];
            before += k < wv ? s : 0;
            total += s;
        }
        if (i < g.rows) g.row_offset[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) cells += __shfl_xor(cells, s, 64);
    if (lane == 0) wsum[wv] = cells;
    __syncthreads();
    if (tid == 0) {
        int all = 0;
        for (int k = 0; k < 16; ++k) all += wsum[k];
        g.counts[0] = carry;
        g.counts[1] = min(carry, g.capacity);
        g.counts[2] = all;
    }
}

__global__ __launch_bounds__(256) void voxel_emit_kernel(const VoxelK g) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= g.rows) return;
    const int off = g.row_offset[r];
    if (g.row_heads[r] == 0 || off >= g.capacity) return;
    const int y = r % g.ny, z = r / g.ny;
    const unsigned long long* cur = g.bits + (size_t)r * g.wpr;
    const unsigned long long* prev = y > 0 ? cur - g.wpr : nullptr;
    const float lo_y = voxel_plane(g.origin[1], g.voxel, y);
    const float lo_z = voxel_plane(g.origin[2], g.voxel, z), hi_z = voxel_plane(g.origin[2], g.voxel, z + 1);
    voxel_row_heads(cur, prev, g.wpr, [&](int k, int x0, int x1) {
        const int o = off + k;
        if (o >= g.capacity) return;
        int y1 = y + 1;
        while (y1 < g.ny && voxel_holds_run(cur + (size_t)(y1 - y) * g.wpr, g.wpr, x0, x1)) ++y1;
        float* lo = g.box_lo + (size_t)o * 3;
        float* hi = g.box_hi + (size_t)o * 3;
        lo[0] = voxel_plane(g.origin[0], g.voxel, x0);
        lo[1] = lo_y;
        lo[2] = lo_z;
        hi[0] = voxel_plane(g.origin[0], g.voxel, x1);
        hi[1] = voxel_plane(g.origin[1], g.voxel, y1);
        hi[2] = hi_z;
    });
}
