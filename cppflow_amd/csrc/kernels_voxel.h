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
//
// Scenes FUSED OVER FRAMES (cppf_voxel_map_*, cppf_scene_from_map; "Scenes fused over frames" in the header, tests/voxel_map.py): a
// map of one uint8 hit counter per cell in the bitset's geometry (cell x of row r at byte r 64 wpr + x behind a 16-byte header), so
// that byte b of the bitset and the 64-bit word b of the counters speak of the same eight cells.
//   adding a frame      voxel_clear_kernel, voxel_self_kernel, voxel_points_kernel as above -- the frame's bitset -- and then
//     voxel_integrate_kernel   one lane per bitset byte: its eight counters + 1 where the bit is set, saturating at 255; the cells of
//                              the frame by a population count, summed per workgroup; lane 0 of the grid counts the frame
//   map to scene        voxel_clear_kernel (the per-row arrays and counts), then
//     voxel_threshold_kernel   one lane per bitset word: its 64 counters >= min_frames, stored whole; the cells seen at all likewise
//   and either voxel_rows_kernel / voxel_scan_kernel / voxel_emit_kernel, or, merging along z as well,
//     voxel_rows_z_kernel      one lane per row (y, z): its cells and its Z-HEADS (heads whose box layer z - 1 does not repeat)
//     voxel_scan_kernel        as above
//     voxel_emit_z_kernel      the same walk; a z-head follows its box up z + 1, ... and stores its cuboid at its offset
// No lane shares a counter or a bitset word with another, so these passes need no atomic but the integer add of a workgroup's
// population count (once per workgroup that counted anything): the map and the lists are again the same bytes in every run.
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

// ---- scenes fused over frames ---------------------------------------------------------------------------------------------------------
struct VoxelMapK {
    int32_t* header;               // the map's first 16 bytes: { frames, 0, 0, 0 }
    unsigned long long* counters;  // behind them: word b holds the uint8 counters of the eight cells of bitset byte b
    size_t n_bytes;                // rows wpr 8: the bitset's bytes, the counters' words
};

__global__ __launch_bounds__(256) void voxel_map_clear_kernel(uint4* __restrict__ map16, size_t n16) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) map16[i] = make_uint4(0u, 0u, 0u, 0u);
}

// the sum of v over the workgroup (256 lanes, every one of them here) onto *dst: shuffles, the four wavefront sums through LDS, one
// integer atomic add by lane 0 unless the sum is 0
__device__ __forceinline__ void voxel_block_add(int v, int32_t* dst) {
    __shared__ int wsum[4];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int all = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (all != 0) atomicAdd(dst, all);
    }
}

constexpr unsigned long long kVoxelByteTop = 0x8080808080808080ull, kVoxelByteOne = 0x0101010101010101ull;

// Byte k of the result is 1 where bit k of b is set, else 0: b in every byte, bit k kept in byte k, and + 0x7f carries any kept bit
// into the byte's top (a byte holds at most 0x80 + 0x7f: nothing leaves it).
__device__ __forceinline__ unsigned long long voxel_bits_to_bytes(unsigned b) {
    const unsigned long long own = ((unsigned long long)b * kVoxelByteOne) & 0x8040201008040201ull;
    return ((own + (kVoxelByteOne * 0x7full)) >> 7) & kVoxelByteOne;
}

// Bit k of the result: byte k of c >= m, unsigned, 1 <= m <= 255.  Per byte: (low seven bits | 0x80) - (m's low seven bits) lies
// in 1 .. 255 -- no borrow leaves the byte -- and keeps its top bit iff the low seven bits are >= m's; the top bits of c and m
// decide first.  The top bits are then gathered by one multiplication (its partial products fall on pairwise different bits).
__device__ __forceinline__ unsigned voxel_bytes_ge(unsigned long long c, unsigned m) {
    const unsigned long long low = ((c & ~kVoxelByteTop) | kVoxelByteTop) - (unsigned long long)(m & 127u) * kVoxelByteOne;
    const unsigned long long ge = ((m & 128u) ? (c & low) : (c | low)) & kVoxelByteTop;
    return (unsigned)(((ge >> 7) * 0x0102040810204080ull) >> 56);
}

// One lane per byte of the frame's bitset = per word of eight counters, which it alone reads and writes.  No lane leaves before the
// barrier of voxel_block_add.
__global__ __launch_bounds__(256) void voxel_integrate_kernel(const unsigned char* __restrict__ bits, const VoxelMapK m,
                                                              int32_t* __restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned b = i < m.n_bytes ? bits[i] : 0u;
    if (b != 0u) {
        const unsigned long long c = m.counters[i];
        // a counter at 255 stays: its byte is the one whose low seven bits + 1 reach the top bit while its own top bit is set
        const unsigned long long full = ((c & ~kVoxelByteTop) + kVoxelByteOne) & c & kVoxelByteTop;
        m.counters[i] = c + (voxel_bits_to_bytes(b) & ~(full >> 7));  // (no byte that is added to holds 255: no carry)
    }
    voxel_block_add(__builtin_popcount(b), &counts[2]);
    if (i == 0) {
        const int32_t f = m.header[0], g = f < INT32_MAX ? f + 1 : f;
        m.header[0] = g;
        counts[7] = g;
    }
}

// One lane per word of the bitset: its 64 counters are 64 consecutive bytes (four 16-byte loads).  Counters at x >= nx are 0 in a
// map only this library wrote; the last word of a row is masked all the same, so that no caller's byte can set a bit there.
__global__ __launch_bounds__(256) void voxel_threshold_kernel(const VoxelK g, const uint4* __restrict__ counters16,
                                                              const int32_t* __restrict__ header, int min_frames) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    int seen_cells = 0;
    if (w < (size_t)g.rows * g.wpr) {
        unsigned long long occ = 0ull, seen = 0ull;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = counters16[w * 4 + k];
            const unsigned long long c0 = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
            const unsigned long long c1 = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
            occ |= (unsigned long long)(voxel_bytes_ge(c0, (unsigned)min_frames) | (voxel_bytes_ge(c1, (unsigned)min_frames) << 8)) << (16 * k);
            seen |= (unsigned long long)(voxel_bytes_ge(c0, 1u) | (voxel_bytes_ge(c1, 1u) << 8)) << (16 * k);
        }
        const int tail = g.nx & 63;
        const unsigned long long valid = (tail != 0 && (int)(w % (size_t)g.wpr) == g.wpr - 1) ? (1ull << tail) - 1ull : ~0ull;
        g.bits[w] = occ & valid;
        seen_cells = __builtin_popcountll(seen & valid);
    }
    voxel_block_add(seen_cells, &g.counts[3]);
    if (w == 0) g.counts[7] = header[0];
}

// Does layer z' hold the box (x0, x1, y, y1) -- is it a member of B(z')?  row: row (y, z').  Row y holds the identical maximal run, row
// y - 1 does not (so the run is a head there), rows y + 1 .. y1 - 1 do, and row y1 does not (so the head's box ends where this one does).
__device__ __forceinline__ bool voxel_layer_holds_box(const unsigned long long* __restrict__ row, int wpr, int ny, int x0, int x1, int y,
                                                      int y1) {
    if (!voxel_holds_run(row, wpr, x0, x1)) return false;
    if (y > 0 && voxel_holds_run(row - wpr, wpr, x0, x1)) return false;
    for (int yy = y + 1; yy < y1; ++yy)
        if (!voxel_holds_run(row + (size_t)(yy - y) * wpr, wpr, x0, x1)) return false;
    return y1 == ny || !voxel_holds_run(row + (size_t)(y1 - y) * wpr, wpr, x0, x1);
}
// f(k, x0, x1, y1) for the z-heads of row (y, z) in ascending x0, k = 0, 1, ...; cur: that row.  Returns their number.
template <class F>
__device__ __forceinline__ int voxel_row_zheads(const VoxelK& g, const unsigned long long* __restrict__ cur, int y, int z, F&& f) {
    const size_t layer = (size_t)g.ny * g.wpr;
    int zheads = 0;
    voxel_row_heads(cur, y > 0 ? cur - g.wpr : nullptr, g.wpr, [&](int, int x0, int x1) {
        int y1 = y + 1;
        while (y1 < g.ny && voxel_holds_run(cur + (size_t)(y1 - y) * g.wpr, g.wpr, x0, x1)) ++y1;
        if (z > 0 && voxel_layer_holds_box(cur - layer, g.wpr, g.ny, x0, x1, y, y1)) return;
        f(zheads++, x0, x1, y1);
    });
    return zheads;
}

__global__ __launch_bounds__(256) void voxel_rows_z_kernel(const VoxelK g) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= g.rows) return;
    const unsigned long long* cur = g.bits + (size_t)r * g.wpr;
    int cells = 0;
    for (int w = 0; w < g.wpr; ++w) cells += __builtin_popcountll(cur[w]);
    g.row_cells[r] = cells;
    g.row_heads[r] = cells == 0 ? 0 : voxel_row_zheads(g, cur, r % g.ny, r / g.ny, [](int, int, int, int) {});
}

__global__ __launch_bounds__(256) void voxel_emit_z_kernel(const VoxelK g) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= g.rows) return;
    const int off = g.row_offset[r];
    if (g.row_heads[r] == 0 || off >= g.capacity) return;
    const int y = r % g.ny, z = r / g.ny;
    const unsigned long long* cur = g.bits + (size_t)r * g.wpr;
    const size_t layer = (size_t)g.ny * g.wpr;
    const float lo_y = voxel_plane(g.origin[1], g.voxel, y), lo_z = voxel_plane(g.origin[2], g.voxel, z);
    voxel_row_zheads(g, cur, y, z, [&](int k, int x0, int x1, int y1) {
        const int o = off + k;
        if (o >= g.capacity) return;
        int z1 = z + 1;
        while (z1 < g.nz && voxel_layer_holds_box(cur + (size_t)(z1 - z) * layer, g.wpr, g.ny, x0, x1, y, y1)) ++z1;
        float* lo = g.box_lo + (size_t)o * 3;
        float* hi = g.box_hi + (size_t)o * 3;
        lo[0] = voxel_plane(g.origin[0], g.voxel, x0);
        lo[1] = lo_y;
        lo[2] = lo_z;
        hi[0] = voxel_plane(g.origin[0], g.voxel, x1);
        hi[1] = voxel_plane(g.origin[1], g.voxel, y1);
        hi[2] = voxel_plane(g.origin[2], g.voxel, z1);
    });
}
