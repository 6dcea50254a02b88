// cppflow_hip.hip -- kernels + C ABI of libcppflow_hip.so (gfx950 only; see include/cppflow_hip.h for the contract).
//
// Layout of the work: one (seed, waypoint) row per lane, 256 rows per workgroup; rows are independent (no reduction
// across rows anywhere in the reference's pose-only step, cppflow/optimization.py:61-92), so there is no inter-workgroup
// communication and the blockIdx -> rows map needs no XCD awareness: every workgroup streams its own contiguous slab of
// x, and the only shared data (the [W,7] target path, <= 14 KB) sits in every XCD's L2.
//
// The fused kernel keeps x in registers across K iterations of
//     FK -> pose error -> geometric Jacobian -> row scaling -> damped solve -> x += delta -> clamp
// and then evaluates the pose-error metrics and (optionally) the capsule collision masks / search cost of the result
// in the same launch.  The damped normal equations are solved in their dual form
//     delta = Js^T (Js Js^T + lambda I6)^-1 es        ( == (Js^T Js + lambda I)^-1 Js^T es exactly, push-through identity)
// which is a 6x6 SPD system for every ndof, conditioned like Js Js^T instead of the rank-deficient Js^T Js the reference
// hands to LU, and cheaper than the primal form for ndof >= 6.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/cppflow_hip_debug.h"
#include "lmik_device.h"
#include "obstacle_reach.h"
#include "robots_gen.h"

using namespace cppf;

namespace cppf {
// fused_static.hip: lm_fused_kernel<StaRobot<table static_id>, coll> -- the row-shape fused kernel of the shipped robots lives in
// its own translation unit (another machine scheduler, see there)
bool launch_fused_static(int static_id, int coll, unsigned grid, size_t lds, hipStream_t st, const FusedArgs& args);
int fused_static_block();
}  // namespace cppf

namespace {

#ifndef CPPF_BLOCK
#define CPPF_BLOCK 256
#endif
constexpr int kBlock = CPPF_BLOCK;

// minimum resident waves per SIMD the register allocator must leave room for (2nd __launch_bounds__ argument)
#ifndef CPPF_WAVES_LM
#define CPPF_WAVES_LM 2
#endif
#ifndef CPPF_WAVES_COLL
#define CPPF_WAVES_COLL 2
#endif

// the device code, by topic (everything below lives in this anonymous namespace; the row-shape fused kernel of the shipped
// robots is instantiated in fused_static.hip instead)
#include "kernels_chain.h"
#include "kernels_collision.h"
#include "kernels_fused.h"
#include "kernels_track.h"
#include "kernels_quad.h"
#include "kernels_eval.h"
#include "kernels_scene.h"  // (ahead of the coupled step: its scene form shares the box / broadcast helpers)
#include "kernels_voxel.h"  // (scenes from sensor data: reads nothing of the above but the capsule FK)
#include "kernels_motion.h"
#include "kernels_motion_resolve.h"
#include "kernels_coupled.h"
#include "kernels_dp.h"
#include "kernels_optloop.h"

// ---- host side --------------------------------------------------------------------------------------------------------------

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define CPPF_REQUIRE(cond, msg) \
    do {                        \
        if (!(cond)) return fail(CPPF_ERR_INVALID, std::string("cppflow_hip: ") + (msg)); \
    } while (0)

#define CPPF_HIP(call)                                                                                       \
    do {                                                                                                     \
        hipError_t e__ = (call);                                                                             \
        if (e__ != hipSuccess)                                                                               \
            return fail(CPPF_ERR_HIP, std::string("cppflow_hip: " #call " failed: ") + hipGetErrorString(e__)); \
    } while (0)

inline unsigned grid_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }

struct RtcModule;  // rtc_specialize.h

}  // namespace

struct cppf_robot {
    cppf_robot_desc desc;
    ChainK chain;
    CollK coll;
    int device;
    int cu_count;      // compute units of `device` (0 for the host-only handle): what a resident launch's grid is held against
    int static_id;     // index into robots_gen.h when the description equals a generated table, else -1
    size_t lds_bytes;  // generic path only: capsule end points, 6 floats per capsule per lane
    void* d_quad;      // device: QuadPairRec[CPPF_MAX_PAIRS] then QuadCapRec[CPPF_MAX_CAPSULES] (quad shape's striped collision stage),
                       // then the travel-bound table rho[CPPF_MAX_DOF][CPPF_MAX_CAPSULES] of cppf_motion_clearance
    float rho[CPPF_MAX_DOF][CPPF_MAX_CAPSULES];  // host copy of that table (motion_rho_table)
    RtcModule* rtc;    // kernels compiled for this description by cppf_robot_specialize (hipRTC), else NULL
    // Test / tuning switches of THIS handle (cppf_debug_set, include/cppflow_hip_debug.h): no process-wide dispatch state, two
    // handles on two threads can hold different settings.  Atomics: a setter may race with a launch on another thread.
    mutable std::atomic<int> tune[CPPF_TUNE_COUNT];
    // Lifetime (cppflow_hip.h, "Ownership"): the number of live cppf_lm_batch objects bound to this handle, and kRobotDead once
    // cppf_robot_destroy has been called.  ONE word, so that whoever takes it to { dead, 0 batches } with its single atomic
    // read-modify-write is the one who frees the handle -- and nobody else touches it afterwards.
    mutable std::atomic<uint32_t> life;
};
constexpr uint32_t kRobotDead = 0x80000000u;

namespace {
// defaults of the switches (the measured crossovers; see include/cppflow_hip_debug.h)
constexpr int kTuneDefaults[CPPF_TUNE_COUNT] = {
    /* FORCE_GENERIC */ 0, /* PCR_MAX_ROWS */ -1, /* QUAD_MAX_ROWS */ 16384, /* DP_PERSISTENT */ 1,
    /* FULL_ROWS */ 1,     /* PCR_LDS */ 2,       /* ROWS_POSE */ 0,         /* QUAD_MFMA */ 0,
    /* SPREAD_KB */ 42,    /* DP_SPIN_LOG2 */ 22,    /* GATE_REL_PPM */ (int)(kGateRel * 1e6f + 0.5f), /* CU_COUNT */ -1,
    /* LM_PACE */ 0,
};
inline int tune(const cppf_robot* rb, int key) { return rb->tune[key].load(std::memory_order_relaxed); }

// static LDS of a fused kernel: the gate's slots of its four wavefronts + the summary staging -- the bound the kernel itself
// static_asserts next to its __shared__ declarations (fused_static_lds_bound, kernels_fused.h)
inline size_t fused_static_lds(const cppf_robot* rb) { return fused_static_lds_bound(rb->desc.ndof); }
// Dynamic LDS (bytes) a fused row-shape launch of n rows claims purely to bound how many of its workgroups share a compute unit
// (CPPF_TUNE_SPREAD_KB; 0 = none): static LDS (the conditioning gate's slots: 13 KB at 7 joints, 17 KB at 12) + the claim stays
// under the 64 KB a workgroup may have without asking, and two such workgroups fit on a unit's 160 KB where a third does not.  Only
// launches of at most 128 workgroups take it -- half a workgroup per compute unit, so the four launches the hardware keeps in
// flight (profiles/r3_streams_sweep.txt) still all fit.  Measured on a 32 768-row shard, four launches in flight: 8.46 -> 7.1 ..
// 7.8 us per step (the dispatcher otherwise stacks the launches four deep on the units it tries first and leaves others idle);
// at 65 536 rows the same claim would hold two of the four launches back (10.1 -> 12.8 us), hence the bound.
inline size_t fused_spread_lds(const cppf_robot* rb, size_t n) {
    const int kb = tune(rb, CPPF_TUNE_SPREAD_KB);
    if (kb <= 0 || n > (size_t)128 * kBlock) return 0;
    const size_t stat = fused_static_lds(rb);
    const size_t room = stat + 512 < 65536 ? 65536 - 512 - stat : 0;
    return std::min((size_t)kb * 1024, room);
}
}  // namespace

#include "rtc_specialize.h"

namespace {

// smallest fp32 y with sqrt_rn(y) >= r (host sqrtf is correctly rounded): sqrtf(d2) - r < 0  <=>  d2 < y for all d2 >= 0
float sqrt_threshold(float r) {
    if (!(r > 0.f)) return 0.f;
    float y = r * r;
    while (std::sqrt(y) >= r) y = std::nextafterf(y, 0.f);
    while (std::sqrt(y) < r) y = std::nextafterf(y, INFINITY);
    return y;
}

// A capsule as the kernels use it: centre c = 0.5 (p0 + p1), half-axis h = 0.5 (p1 - p0), a = |h|^2, 1 / a -- double arithmetic
// on the fp32 end points of the description, each rounded to fp32 once (a over the ROUNDED h, summed (h0 h0 + h1 h1) + h2 h2).
// The same lines are in cppflow_amd/gen_robots.py (capsule_centred) and oracle/lmik_oracle.c (orc_robot_create).
struct CapsuleCentred {
    float c[3], h[3], a, ia;
    double half_length;  // sqrt of the unrounded a
};
CapsuleCentred capsule_centred(const cppf_robot_desc& d, int cap) {
    CapsuleCentred r;
    for (int k = 0; k < 3; ++k) {
        r.c[k] = (float)(0.5 * ((double)d.cap_p0[cap][k] + (double)d.cap_p1[cap][k]));
        r.h[k] = (float)(0.5 * ((double)d.cap_p1[cap][k] - (double)d.cap_p0[cap][k]));
    }
    const double h0 = r.h[0], h1 = r.h[1], h2 = r.h[2];
    const double a = (h0 * h0 + h1 * h1) + h2 * h2;
    r.a = (float)a;
    r.ia = a >= 0x1p-100 ? (float)(1.0 / a) : 0.f;  // a zero-length capsule is a sphere: its parameter stays 0 (as rcp_rn would have it)
    r.half_length = std::sqrt(a);
    return r;
}

// broad-phase thresholds (see cull_far): (reach + 1 cm)^2 (1 + 1e-4), rounded up to fp32
double cap_half_length(const cppf_robot_desc& d, int c) { return capsule_centred(d, c).half_length; }

float cull_threshold(double reach) {
    const double y = (reach + 0.01) * (reach + 0.01) * (1.0 + 1e-4);
    float f = (float)y;
    if ((double)f < y) f = std::nextafterf(f, INFINITY);
    return f;
}

// certain-hit threshold on the centre's squared distance from a cuboid: max(r - 1 cm, 0)^2 (1 - 1e-4), rounded DOWN
// (gen_robots.py: inside_threshold; env_item_undecided in kernels_collision.h)
float inside_threshold(float r) {
    const double m = (double)r - 0.01 > 0.0 ? (double)r - 0.01 : 0.0;
    const double y = m * m * (1.0 - 1e-4);
    float f = (float)y;
    if ((double)f > y) f = std::nextafterf(f, 0.f);
    return f;
}

// Travel bounds of cppf_motion_clearance (kernels_motion.h): rho[j][c] >= the distance of any point of capsule c from the axis of
// revolute joint j <= cap_link[c] -- the translations of the fixed transforms between joint j and the capsule's link, the largest
// excursion of every prismatic joint in between, and the capsule's own extent from its link's origin; 1 for a prismatic joint
// j <= cap_link[c] (a point moves as far as the joint does); 0 for a joint behind the link.  fp64, rounded UP to fp32.
constexpr int kQuadTableRecs = CPPF_MAX_PAIRS + CPPF_MAX_CAPSULES;  // uint4 records of d_quad in front of the rho table
float round_up_f32(double y) {
    float f = (float)y;
    if ((double)f < y) f = std::nextafterf(f, INFINITY);
    return f;
}
void motion_rho_table(const cppf_robot_desc& d, float (&rho)[CPPF_MAX_DOF][CPPF_MAX_CAPSULES]) {
    const auto norm3 = [](const float* v) { return std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); };
    for (int j = 0; j < CPPF_MAX_DOF; ++j)
        for (int c = 0; c < CPPF_MAX_CAPSULES; ++c) rho[j][c] = 0.f;
    for (int c = 0; c < d.n_capsules; ++c) {
        const int l = d.cap_link[c];
        const double tail = std::max(norm3(d.cap_p0[c]), norm3(d.cap_p1[c])) + (double)d.cap_r[c];
        for (int j = 0; j <= l; ++j) {
            if (d.jtype[j] == CPPF_JOINT_PRISMATIC) {
                rho[j][c] = 1.f;
                continue;
            }
            double sum = tail;
            for (int i = j + 1; i <= l; ++i) {
                sum += norm3(&d.F[i][9]);
                if (d.jtype[i] == CPPF_JOINT_PRISMATIC) sum += std::max(std::fabs((double)d.lo[i]), std::fabs((double)d.hi[i]));
            }
            rho[j][c] = round_up_f32(sum);
        }
    }
}

// does a description equal a generated compile-time table exactly?
template <class T>
bool desc_matches(const cppf_robot_desc& d) {
    if (d.ndof != T::D || d.n_capsules != T::L || d.n_pairs != T::P) return false;
    uint32_t pm = 0;
    for (int j = 0; j < T::D; ++j) {
        if (d.jtype[j] == CPPF_JOINT_PRISMATIC) pm |= 1u << j;
        for (int k = 0; k < 12; ++k)
            if (d.F[j][k] != T::F[j][k]) return false;
        if (d.lo[j] != T::lo[j] || d.hi[j] != T::hi[j]) return false;
    }
    if (pm != T::pris_mask) return false;
    for (int k = 0; k < 12; ++k)
        if (d.F_ee[k] != T::Fee[k]) return false;
    for (int c = 0; c < T::L; ++c) {
        if (d.cap_link[c] != T::cap_link[c] || d.cap_r[c] != T::cap_r[c]) return false;
        for (int k = 0; k < 3; ++k)
            if (d.cap_p0[c][k] != T::cap_p0[c][k] || d.cap_p1[c][k] != T::cap_p1[c][k]) return false;
    }
    for (int p = 0; p < T::P; ++p)
        if (d.pairs[p][0] != T::pair_a[p] || d.pairs[p][1] != T::pair_b[p]) return false;
    return true;
}

int find_static_robot(const cppf_robot_desc& d) {
#define CPPF_MATCH(idx, Type) \
    if (desc_matches<Type>(d)) return idx;
    CPPF_FOR_EACH_STATIC_ROBOT(CPPF_MATCH)
#undef CPPF_MATCH
    return -1;
}

// ---- dispatch: which instantiation a launch takes ---------------------------------------------------------------------------
// Each dispatcher calls a generic lambda with a tag VALUE; the lambda names what the tag carries (`constexpr int D =
// decltype(dof)::D;`, `using RB = typename decltype(tag)::type;`) and returns a CPPF_* code, which the dispatcher hands on.
template <int N>
struct Dof {
    static constexpr int D = N;
};
template <class T>
struct RobotTag {
    using type = T;  // the kernels' accessor type: DynRobot<D> or StaRobot<generated table>
};

// on ndof: the light kernels are instantiated for the degrees of freedom of the shipped robots
template <class F>
int for_ndof(int d, F&& f) {
    switch (d) {
        case 3: return f(Dof<3>{});
        case 4: return f(Dof<4>{});
        case 5: return f(Dof<5>{});
        case 6: return f(Dof<6>{});
        case 7: return f(Dof<7>{});
        case 8: return f(Dof<8>{});
        case 9: return f(Dof<9>{});
        case 10: return f(Dof<10>{});
        case 11: return f(Dof<11>{});
        case 12: return f(Dof<12>{});
        default: return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: kernels are built for ndof in 3..12");
    }
}

// the generic instantiations of the heavy kernels only (the caller has dealt with the generated tables)
template <class F>
int for_dyn_robot(const cppf_robot* rb, F&& f) {
    return for_ndof(rb->desc.ndof, [&](auto dof) { return f(RobotTag<DynRobot<decltype(dof)::D>>{}); });
}

// does a launch on this handle take the kernels of a generated table?
inline bool use_table(const cppf_robot* rb) { return rb->static_id >= 0 && !tune(rb, CPPF_TUNE_FORCE_GENERIC); }

// the heavy kernels on the robot: a generated table if the description matched one, else the generic instantiation for its ndof
template <class F>
int for_robot(const cppf_robot* rb, F&& f) {
    if (!use_table(rb)) return for_dyn_robot(rb, f);
    switch (rb->static_id) {
#define CPPF_TABLE_CASE(idx, Type) \
    case idx: return f(RobotTag<StaRobot<Type>>{});
        CPPF_FOR_EACH_STATIC_ROBOT(CPPF_TABLE_CASE)
#undef CPPF_TABLE_CASE
        default: return CPPF_OK;  // (a matched table without a case here: nothing is launched)
    }
}

constexpr int kNoDevice = -12345;  // cppf_robot_create's host-only mode (no HIP call), for cppf_debug_rtc_compile
// coupled step: parallel-in-time elimination up to this many (trajectory, waypoint) rows -- the measured crossovers with the
// two-ended row-per-lane kernels at d <= 7 (x 0.5 at d = 8): 512 trajectories x 256 waypoints with the state in LDS (W <= 256: one
// workgroup per compute unit, so the time steps up at every multiple of 256 trajectories), 192 x 256 with the state in the workspace
constexpr int kPcrMaxRowsLds = 131072, kPcrMaxRowsGlobal = 49152;
// the split form of the LDS-resident reduction (two wavefront-uniform halves per waypoint) up to this many joints: -6 ... -8 % at
// d = 7 (one Panda trajectory 64.4 -> 59.1 us), -5 % at d = 8 (Fetch 85.6 -> 81.4 us) since round 4 -- in round 3 it spilled 300 B
// per lane there and lost 9 %; profiles/r4_pcr_ab.txt
constexpr int kPcrSplitMaxD = 8;

inline bool use_rtc(const cppf_robot* rb) { return rb->rtc != nullptr && !tune(rb, CPPF_TUNE_FORCE_GENERIC); }

int check_launch() {
    CPPF_HIP(hipGetLastError());
    return CPPF_OK;
}

// Launches go to the robot's device; the calling thread's current device is put back on return (a caller -- torch included --
// that had another device current must not find it changed behind its back).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// has cppf_robot_destroy been called on the handle (it is then only kept allocated for its live batches)?
inline bool robot_destroyed(const cppf_robot* rb) { return (rb->life.load(std::memory_order_acquire) & kRobotDead) != 0; }

// what every call that reads the handle asks of it before anything else, in the short words of the calls that check their arguments
// before they select a device (CPPF_ENTER, which selects it, says more)
#define CPPF_ROBOT_ALIVE(rb)                                 \
    CPPF_REQUIRE((rb) != nullptr, "robot handle is NULL"); \
    CPPF_REQUIRE(!robot_destroyed(rb), "the robot handle was destroyed")

#define CPPF_ENTER(rb)                                                                                              \
    CPPF_REQUIRE((rb) != nullptr, "robot handle is NULL");                                                          \
    CPPF_REQUIRE(!robot_destroyed(rb),                                                                               \
                 "the robot handle was destroyed (cppf_robot_destroy; it is only kept allocated for its live batches)"); \
    DeviceGuard device_guard__((rb)->device);                                                                        \
    if (device_guard__.err != hipSuccess)                                                                            \
        return fail(CPPF_ERR_HIP, std::string("cppflow_hip: selecting the robot's device failed: ") +               \
                                      hipGetErrorString(device_guard__.err))

// ---- launches ------------------------------------------------------------------------------------------------------------------
// A launch that claims `lds` bytes of dynamic LDS: beyond 64 KB the limit of THIS kernel is raised first (per device: set whenever
// it is needed, a host-side table update).  Errors of the launch itself are the caller's check_launch().
template <class K, class... A>
int launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
    if (lds > (size_t)64 * 1024)
        CPPF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    return CPPF_OK;
}

// The one place that turns a kernel and its arguments into the untyped (function, void**) pair hipLaunchKernel and
// hipModuleLaunchKernel take.  That route copies sizeof(parameter) bytes from each address and converts nothing, so the arguments'
// types must BE the parameter list of the typed kernel -- which the compiler checks here.  Lvalues only: the addresses are read by
// the launch that follows, where a temporary would be gone.
template <class...>
struct Types {};
template <class... P>
struct KernelArgs {
    const void* fn;
    void* ptr[sizeof...(P)];
    template <class... A>
    explicit KernelArgs(void (*kernel)(P...), A&... a) : fn(reinterpret_cast<const void*>(kernel)), ptr{(void*)&a...} {
        static_assert(std::is_same<Types<P...>, Types<std::decay_t<A>...>>::value,
                      "the arguments are not the kernel's parameter list (this route applies no implicit conversion)");
    }
};

// Launch kernel `which` of the handle's run-time-specialised module.  `same` is a compiled-in instantiation of the same kernel
// template -- of any robot type, the parameter list does not depend on it -- and is what the arguments are checked against.
template <class... P, class... A>
int rtc_launch(const cppf_robot* rb, RtcKernel which, void (*same)(P...), unsigned grid, unsigned block, size_t lds, hipStream_t st,
               const A&... args) {
    hipFunction_t f = rb->rtc->fn[which];
    if (!f) return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: this kernel is not part of the handle's specialised module");
    KernelArgs<P...> ka(same, args...);
    CPPF_HIP(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, (unsigned)lds, st, ka.ptr, nullptr));
    return CPPF_OK;
}

// The route of the heavy kernels that exist in all three forms (collision, quad, track): the handle's specialised module, else the
// kernel of a generated table, else the generic one.  pick(tag) names the compiled-in instantiation for a robot type (NULL: there is
// none for this type, nothing is launched); kernel `which` of the module takes the same arguments, checked against the generic
// six-joint instantiation, which every one of these kernels has.
template <class Pick, class... A>
int launch_routed(const cppf_robot* rb, RtcKernel which, Pick&& pick, unsigned grid, unsigned block, size_t lds, hipStream_t st,
                  const A&... args) {
    if (use_rtc(rb)) return rtc_launch(rb, which, pick(RobotTag<DynRobot<6>>{}), grid, block, lds, st, args...);
    return for_robot(rb, [&](auto tag) {
        const auto kernel = pick(tag);
        return kernel ? launch(kernel, dim3(grid), dim3(block), lds, st, args...) : CPPF_OK;
    });
}

// ---- what the calls over a scene in device memory share (kernels_scene.h) ----------------------------------------------------------
// the culling block of a walk over the scene's cuboids at this reach (reach = 0: cull2[c] is cull_threshold of the same double sum
// as cap_cull[c], i.e. cap_cull[c] itself, and tile_cull2 the coupled step's)
float tile_cull_threshold(const cppf_robot* robot, float reach) {  // wavefront box vs cuboid: the widest capsule decides
    double r_max = 0.0;
    for (int c = 0; c < robot->coll.ncaps; ++c) r_max = std::max(r_max, (double)robot->desc.cap_r[c]);
    return cull_threshold(r_max + (double)reach);
}
SceneCullK scene_cull_setup(const cppf_robot* robot, const float* box_lo, const float* box_hi, int n_obs, float reach) {
    SceneCullK sc;
    sc.box_lo = box_lo;
    sc.box_hi = box_hi;
    sc.n_obs = n_obs;
    sc.reach = reach;
    for (int c = 0; c < CPPF_MAX_CAPSULES; ++c) sc.cull2[c] = 0.f;
    for (int c = 0; c < robot->coll.ncaps; ++c)
        sc.cull2[c] = cull_threshold(cap_half_length(robot->desc, c) + (double)robot->desc.cap_r[c] + (double)reach);
    sc.tile_cull2 = tile_cull_threshold(robot, reach);
    return sc;
}

// Chunks of cuboids (grid.y) for a launch of `blocks` workgroups along grid.x: enough workgroups for four per compute unit (four
// wavefronts per SIMD) where those alone do not give them, in groups of 8 cuboids -- a lone wavefront per SIMD issues at a fraction
// of the rate, and one plan's rows are a single workgroup (measured: 1 x 256 rows, 64 cuboids, reach = inf, one chunk of 64: 253 us).
// A chunk repeats the capsule FK of its rows, which is small beside 8 cuboids x every capsule.  The result does not depend on the
// cut (integer min over keys).
struct CuboidChunks {
    int n_chunks, chunk;  // chunk: cuboids per blockIdx.y, a multiple of 8
};
CuboidChunks cut_cuboid_chunks(const cppf_robot* robot, unsigned blocks, int n_obs) {
    const int groups = (n_obs + 7) / 8;
    if (groups == 0 || blocks == 0) return {1, 64};
    const unsigned want_blocks = 4u * (unsigned)(robot->cu_count > 0 ? robot->cu_count : 256);
    int n_chunks = (int)std::min<unsigned>((unsigned)groups, std::max(1u, (want_blocks + blocks - 1) / blocks));
    const int groups_per_chunk = (groups + n_chunks - 1) / n_chunks;
    n_chunks = (groups + groups_per_chunk - 1) / groups_per_chunk;
    return {n_chunks, groups_per_chunk * 8};
}

// The argument rules of cppf_scene_env_collisions, cppf_motion_clearance and cppf_motion_resolve, in the order a caller meets them.
// The call's own rules sit between the shared ones: `shape` (its sizes), `io_ok` (q and its first output), `need` (its workspace
// size); `kernel` names its generic kernel.  Every argument is checked before the device is selected (CPPF_ENTER), so that the checks
// hold for a host-only handle too.  *lds: the dynamic LDS of the launch (a handle specialised at run time takes the generic form:
// same bits).
template <class Shape, class Need>
int check_scene_call(const cppf_robot* robot, Shape&& shape, int n_obs, float reach_m, bool io_ok, const char* io_msg, const float* box_lo,
                     const float* box_hi, const void* workspace, size_t workspace_bytes, Need&& need, const char* need_msg,
                     const char* kernel, size_t* lds) {
    CPPF_ROBOT_ALIVE(robot);
    if (int rc = shape()) return rc;
    CPPF_REQUIRE(n_obs >= 0 && n_obs <= CPPF_MAX_SCENE_OBSTACLES, "n_obs out of range (0 .. CPPF_MAX_SCENE_OBSTACLES)");
    CPPF_REQUIRE(reach_m >= 0.f, "reach_m must be in [0, +inf] (not NaN, not negative)");
    CPPF_REQUIRE(io_ok, io_msg);
    CPPF_REQUIRE(n_obs == 0 || (box_lo && box_hi), "box_lo / box_hi is NULL");
    CPPF_REQUIRE(workspace, "workspace is NULL");
    CPPF_REQUIRE(((uintptr_t)workspace & 15u) == 0, "workspace must be 16-byte aligned");
    size_t bytes = 0;
    if (int rc = need(&bytes)) return rc;
    CPPF_REQUIRE(workspace_bytes >= bytes, need_msg);
    if (robot->desc.ndof < 3) return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: kernels are built for ndof in 3..12");
    *lds = use_table(robot) ? 0 : robot->lds_bytes;
    if (*lds > (size_t)160 * 1024 - 1024)
        return fail(CPPF_ERR_UNSUPPORTED, std::string("cppflow_hip: the generic ") + kernel + " kernel cannot stage this many capsules");
    return CPPF_OK;
}

// a cuboid (min corner, max corner in its own frame) under Rt = [R | t] -> its corners in the world; R must be the identity
int cuboid_corners(const float* cuboid, const float* Rt, float (&lo)[3], float (&hi)[3]) {
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k)
        CPPF_REQUIRE(std::fabs(Rt[k] - I[k]) < 1e-8f, "only axis-aligned cuboids are supported (R must be I)");
    for (int k = 0; k < 3; ++k) {
        lo[k] = Rt[9 + k] + cuboid[k];
        hi[k] = Rt[9 + k] + cuboid[3 + k];
    }
    return CPPF_OK;
}

}  // namespace

extern "C" {

int cppf_abi_version(void) { return CPPF_ABI_VERSION; }

#ifndef CPPF_BUILD_ID
#define CPPF_BUILD_ID "unversioned"
#endif
// (the marker lets cppflow_amd/build.py read the id out of the file without loading the library)
static const char kBuildIdMarker[] = "CPPF_BUILD_ID=" CPPF_BUILD_ID;
const char* cppf_build_id(void) { return kBuildIdMarker + 14; }

const char* cppf_last_error(void) { return g_err.c_str(); }

int cppf_robot_create(const cppf_robot_desc* desc, int device, cppf_robot** out) {
    CPPF_REQUIRE(desc && out, "desc / out is NULL");
    *out = nullptr;
    const int d = desc->ndof;
    CPPF_REQUIRE(d >= 1 && d <= CPPF_MAX_DOF, "ndof out of range");
    CPPF_REQUIRE(desc->n_capsules >= 0 && desc->n_capsules <= CPPF_MAX_CAPSULES, "n_capsules out of range");
    CPPF_REQUIRE(desc->n_pairs >= 0 && desc->n_pairs <= CPPF_MAX_PAIRS, "n_pairs out of range");
    for (int j = 0; j < d; ++j) {
        CPPF_REQUIRE(desc->jtype[j] == CPPF_JOINT_REVOLUTE || desc->jtype[j] == CPPF_JOINT_PRISMATIC, "bad joint type");
        CPPF_REQUIRE(desc->lo[j] <= desc->hi[j], "joint limits: lo > hi");
        for (int k = 0; k < 12; ++k) CPPF_REQUIRE(std::isfinite(desc->F[j][k]), "non-finite chain constant");
    }
    int prev = -1;
    for (int c = 0; c < desc->n_capsules; ++c) {
        const int l = desc->cap_link[c];
        CPPF_REQUIRE(l >= -1 && l < d, "capsule link index out of range");
        CPPF_REQUIRE(l >= prev, "capsules must be ordered by link (base first)");
        prev = l;
        float len2 = 0.f;
        for (int k = 0; k < 3; ++k) {
            const float dd = desc->cap_p1[c][k] - desc->cap_p0[c][k];
            len2 += dd * dd;
        }
        // p0 == p1 exactly is a SPHERE (its 1 / |h|^2 is 0, capsule_centred); a segment shorter than a micrometre is a mistake
        CPPF_REQUIRE(len2 == 0.f || len2 > 1e-12f, "degenerate capsule (|p1 - p0| < 1e-6 but not 0; use p0 == p1 for a sphere)");
        CPPF_REQUIRE(desc->cap_r[c] >= 0.f, "negative capsule radius");
    }
    for (int p = 0; p < desc->n_pairs; ++p) {
        const int a = desc->pairs[p][0], b = desc->pairs[p][1];
        CPPF_REQUIRE(a >= 0 && a < desc->n_capsules && b >= 0 && b < desc->n_capsules && a != b, "bad capsule pair");
    }
    if (device != kNoDevice) {  // (kNoDevice: the host-only handle cppf_debug_rtc_compile builds)
        int ndev = 0;
        CPPF_HIP(hipGetDeviceCount(&ndev));
        CPPF_REQUIRE(device >= 0 && device < ndev, "device index out of range");
    }

    cppf_robot* rb = new (std::nothrow) cppf_robot();
    if (!rb) return fail(CPPF_ERR_HIP, "cppflow_hip: out of host memory");
    rb->desc = *desc;
    rb->device = device;
    rb->cu_count = 0;
    if (device != kNoDevice) (void)hipDeviceGetAttribute(&rb->cu_count, hipDeviceAttributeMultiprocessorCount, device);
    rb->life.store(0u, std::memory_order_relaxed);
    for (int k = 0; k < CPPF_TUNE_COUNT; ++k) rb->tune[k].store(kTuneDefaults[k], std::memory_order_relaxed);
    std::memset(&rb->chain, 0, sizeof(ChainK));
    std::memset(&rb->coll, 0, sizeof(CollK));
    rb->chain.ndof = d;
    for (int j = 0; j < d; ++j) {
        std::memcpy(rb->chain.F[j], desc->F[j], sizeof(float) * 12);
        rb->chain.lo[j] = desc->lo[j];
        rb->chain.hi[j] = desc->hi[j];
        if (desc->jtype[j] == CPPF_JOINT_PRISMATIC) rb->chain.pris_mask |= (1u << j);
    }
    std::memcpy(rb->chain.Fee, desc->F_ee, sizeof(float) * 12);
    CollK& co = rb->coll;
    co.ncaps = desc->n_capsules;
    co.npairs = desc->n_pairs;
    for (int c = 0; c < co.ncaps; ++c) {
        const CapsuleCentred cc = capsule_centred(*desc, c);
        for (int k = 0; k < 3; ++k) {
            co.cap_c[c][k] = cc.c[k];
            co.cap_h[c][k] = cc.h[k];
        }
        co.cap_a[c] = cc.a;
        co.cap_ia[c] = cc.ia;
        co.cap_r[c] = desc->cap_r[c];
        co.cap_link[c] = (int8_t)desc->cap_link[c];
        co.cap_thr[c] = sqrt_threshold(desc->cap_r[c]);
        co.cap_cull[c] = cull_threshold(cap_half_length(*desc, c) + (double)desc->cap_r[c]);
        co.cap_in[c] = inside_threshold(desc->cap_r[c]);
        co.cap_box[c] = cull_threshold((double)desc->cap_r[c]);
    }
    // cap_begin[l+1] = first capsule whose link >= l
    for (int l = -1; l <= d; ++l) {
        int first = co.ncaps;
        for (int c = co.ncaps - 1; c >= 0; --c)
            if (desc->cap_link[c] >= l) first = c;
        co.cap_begin[l + 1] = first;
    }
    for (int p = 0; p < co.npairs; ++p) {
        co.pair_a[p] = (uint8_t)desc->pairs[p][0];
        co.pair_b[p] = (uint8_t)desc->pairs[p][1];
        co.pair_thr[p] = sqrt_threshold(desc->cap_r[desc->pairs[p][0]] + desc->cap_r[desc->pairs[p][1]]);
        const int a = desc->pairs[p][0], b = desc->pairs[p][1];
        co.pair_cull[p] = cull_threshold(cap_half_length(*desc, a) + cap_half_length(*desc, b) + (double)desc->cap_r[a] +
                                         (double)desc->cap_r[b]);
    }
    rb->lds_bytes = (size_t)co.ncaps * 6 * kBlock * sizeof(float);
    rb->static_id = find_static_robot(*desc);
    if (fused_static_block() != kBlock) rb->static_id = -1;  // (the two translation units were built for different workgroup sizes)
    rb->rtc = nullptr;
    rb->d_quad = nullptr;
    motion_rho_table(*desc, rb->rho);
    // device tables of the quad shape (static per robot: pair list, thresholds) and, behind them, the travel bounds
    if (device != kNoDevice) {
        static_assert(sizeof(rb->rho) % sizeof(uint4) == 0, "the rho table is a whole number of uint4 records");
        std::vector<uint4> host(kQuadTableRecs + sizeof(rb->rho) / sizeof(uint4), uint4{0, 0, 0, 0});
        std::memcpy(&host[kQuadTableRecs], rb->rho, sizeof(rb->rho));
        for (int p = 0; p < co.npairs; ++p) {
            QuadPairRec r{co.pair_a[p], co.pair_b[p], co.pair_thr[p], co.pair_cull[p]};
            std::memcpy(&host[p], &r, sizeof r);
        }
        for (int c = 0; c < co.ncaps; ++c) {
            QuadCapRec r{co.cap_thr[c], co.cap_cull[c], co.cap_a[c], co.cap_ia[c]};
            std::memcpy(&host[CPPF_MAX_PAIRS + c], &r, sizeof r);
        }
        DeviceGuard guard(device);
        hipError_t e = guard.err;
        rb->d_quad = nullptr;
        if (e == hipSuccess) e = hipMalloc(&rb->d_quad, host.size() * sizeof(uint4));
        if (e == hipSuccess) e = hipMemcpy(rb->d_quad, host.data(), host.size() * sizeof(uint4), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (rb->d_quad) (void)hipFree(rb->d_quad);
            delete rb;
            return fail(CPPF_ERR_HIP, std::string("cppflow_hip: device tables: ") + hipGetErrorString(e));
        }
    }
    *out = rb;
    return CPPF_OK;
}

namespace {
void robot_free(cppf_robot* robot) {
    if (robot->device != kNoDevice) {  // (a host-only handle owns nothing on a device, and selecting "its" device would leave an error behind)
        DeviceGuard guard(robot->device);
        if (robot->d_quad) (void)hipFree(robot->d_quad);
        if (robot->rtc) {
            if (robot->rtc->module) (void)hipModuleUnload(robot->rtc->module);
            delete robot->rtc;
        }
    }
    delete robot;
}
}  // namespace

void cppf_robot_destroy(cppf_robot* robot) {
    if (!robot) return;
    // Live batches keep the handle allocated (their launches then fail with CPPF_ERR_INVALID instead of reading freed memory); the
    // last cppf_lm_batch_destroy frees it.  A second destroy of a handle that is only kept for its batches is ignored.
    const uint32_t before = robot->life.fetch_or(kRobotDead, std::memory_order_acq_rel);
    if (before == 0u) robot_free(robot);
}

int cppf_robot_specialize(cppf_robot* robot, const char* cache_dir) {
    CPPF_REQUIRE(robot != nullptr, "robot handle is NULL");
    if (robot->static_id >= 0 || robot->rtc) return CPPF_OK;
    const bool with_quad = robot->desc.ndof >= 6;  // the quad shape solves the dual 6x6 system
    const std::string source = rtc_program_source(*robot);
    if (const char* dump = std::getenv("CPPF_RTC_DUMP")) {  // developer aid: the generated program, for scripts/rtc_try.py
        std::ofstream f(dump);
        f << source;
    }
    uint64_t key = fnv1a(source);
    for (int i = 0; i < kEmbeddedCount; ++i) key = fnv1a(kEmbeddedSources[i], key);
    for (int i = 0; i < kRtcOptionCount; ++i) key = fnv1a(kRtcOptions[i], key);
    key = fnv1a(rtc_version_string(), key);  // (and the compiler that would produce it)
    char hex[32];
    std::snprintf(hex, sizeof hex, "%016llx", (unsigned long long)key);
    const std::string dir = rtc_cache_dir(cache_dir), file = dir + "/robot_" + hex + ".cppfrtc";
    std::vector<std::string> names;
    std::string code;
    if (!rtc_cache_read(dir, file, names, code)) {
        if (int rc = rtc_compile(source, with_quad, names, code)) return rc;
        rtc_cache_write(dir, file, names, code);
    }
    // (compiling and caching need no device; loading does)
    DeviceGuard device_guard__(robot->device);
    if (device_guard__.err != hipSuccess)
        return fail(CPPF_ERR_HIP, std::string("cppflow_hip: selecting the robot's device failed: ") + hipGetErrorString(device_guard__.err));
    RtcModule* m = new (std::nothrow) RtcModule();
    if (!m) return fail(CPPF_ERR_HIP, "cppflow_hip: out of host memory");
    hipError_t e = hipModuleLoadData(&m->module, code.data());
    for (int i = 0; e == hipSuccess && i < RTC_COUNT; ++i) {
        if (!with_quad && (i == RTC_QUAD0 || i == RTC_QUAD1)) continue;
        e = hipModuleGetFunction(&m->fn[i], m->module, names[(size_t)i].c_str());
    }
    if (e != hipSuccess) {
        if (m->module) (void)hipModuleUnload(m->module);
        delete m;
        return fail(CPPF_ERR_HIP, std::string("cppflow_hip: loading the specialised code object failed: ") + hipGetErrorString(e));
    }
    robot->rtc = m;
    return CPPF_OK;
}

int cppf_robot_ndof(const cppf_robot* robot) { return robot ? robot->desc.ndof : CPPF_ERR_INVALID; }

int cppf_debug_fused_single_offset(void) { return (int)__builtin_offsetof(FusedArgs, single); }

int cppf_debug_rtc_compile(const cppf_robot_desc* desc, const char* cache_dir) {
    cppf_robot* rb = nullptr;
    if (int rc = cppf_robot_create(desc, kNoDevice, &rb)) return rc;
    rb->static_id = -1;  // compile even a shipped description: this hook exercises the run-time path itself
    rb->device = kNoDevice;
    const int rc = cppf_robot_specialize(rb, cache_dir);
    delete rb;
    // without a device the last stage (loading the code object) fails by design; the compile + cache stages have run.  That failure
    // (selecting a device that does not exist) stays behind as the calling thread's last HIP error, and the next launch check of that
    // thread -- this library's or torch's -- would report it as its own: take it back here.
    (void)hipGetLastError();
    return rc;
}

int cppf_robot_specialization(const cppf_robot* robot) {
    if (!robot) return CPPF_ERR_INVALID;
    return robot->static_id >= 0 ? robot->static_id : (robot->rtc ? CPPF_SPECIALIZATION_RTC : -1);
}

int cppf_debug_set(cppf_robot* robot, int key, int value) {
    CPPF_REQUIRE(robot, "robot handle is NULL");
    CPPF_REQUIRE(key >= 0 && key < CPPF_TUNE_COUNT, "unknown tuning key");
    robot->tune[key].store(value == CPPF_TUNE_DEFAULT ? kTuneDefaults[key] : value, std::memory_order_relaxed);
    return CPPF_OK;
}

int cppf_debug_get(const cppf_robot* robot, int key, int* value) {
    CPPF_REQUIRE(robot && value, "robot / value is NULL");
    CPPF_REQUIRE(key >= 0 && key < CPPF_TUNE_COUNT, "unknown tuning key");
    *value = tune(robot, key);
    return CPPF_OK;
}

int cppf_set_obstacles(cppf_robot* robot, int n_obs, const float* cuboids, const float* Rt) {
    CPPF_REQUIRE(robot, "robot handle is NULL");
    CPPF_REQUIRE(n_obs >= 0 && n_obs <= CPPF_MAX_OBSTACLES, "n_obs out of range");
    CPPF_REQUIRE(n_obs == 0 || (cuboids && Rt), "cuboids / Rt is NULL");
    for (int o = 0; o < n_obs; ++o) {
        float lo[3], hi[3];
        if (int rc = cuboid_corners(cuboids + o * 6, Rt + o * 12, lo, hi)) return rc;
        for (int k = 0; k < 3; ++k) {
            CPPF_REQUIRE(cuboids[o * 6 + k] <= cuboids[o * 6 + 3 + k], "cuboid min corner > max corner");
            robot->coll.obs_lo[o][k] = lo[k];
            robot->coll.obs_hi[o][k] = hi[k];
        }
    }
    robot->coll.nobs = n_obs;
    // the capsules that can reach any of these cuboids at all (obstacle_reach.h): the mask-only collision stage skips the others
    const CapsuleReach live = capsule_reach(robot->desc, robot->coll.cap_c, robot->coll.cap_cull, n_obs, robot->coll.obs_lo, robot->coll.obs_hi);
    robot->coll.cap_live_any = live.any;
    robot->coll.cap_live_lim = live.lim;
    return CPPF_OK;
}

int cppf_set_joint_limit_padding(cppf_robot* robot, const float* lo_padded, const float* hi_padded) {
    CPPF_REQUIRE(robot, "robot handle is NULL");
    if (!lo_padded || !hi_padded) {
        robot->coll.has_jl = 0;
        return CPPF_OK;
    }
    for (int j = 0; j < robot->desc.ndof; ++j) {
        robot->coll.jl_lo[j] = lo_padded[j];
        robot->coll.jl_hi[j] = hi_padded[j];
    }
    robot->coll.has_jl = 1;
    return CPPF_OK;
}

int cppf_forward_kinematics(const cppf_robot* robot, const float* x, int n, float* poses, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return CPPF_OK;
    CPPF_REQUIRE(x && poses, "x / poses is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((fk_kernel<decltype(dof)::D>), dim3(grid_for(n)), dim3(kBlock), 0, st, robot->chain, robot->coll, n, x, poses);
        return check_launch();
    });
}

int cppf_jacobian(const cppf_robot* robot, const float* x, int n, float* J, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return CPPF_OK;
    CPPF_REQUIRE(x && J, "x / J is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((jacobian_kernel<decltype(dof)::D>), dim3(grid_for(n)), dim3(kBlock), 0, st, robot->chain, robot->coll, n, x, J);
        return check_launch();
    });
}

int cppf_pose_errors(const cppf_robot* robot, const float* x, const float* target, int S, int W, float* e,
                     float* current_poses, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(S >= 0 && W >= 0, "S / W < 0");
    const size_t n = (size_t)S * W;
    if (n == 0) return CPPF_OK;
    CPPF_REQUIRE(n <= 0x7fffffffu, "S*W exceeds 2^31-1 rows");
    CPPF_REQUIRE(x && target, "x / target is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((pose_errors_kernel<decltype(dof)::D>), dim3(grid_for(n)), dim3(kBlock), 0, st, robot->chain, robot->coll,
                           (int)n, W, x, target, e, current_poses);
        return check_launch();
    });
}

int cppf_clamp_to_joint_limits(const cppf_robot* robot, float* x, int n, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return CPPF_OK;
    CPPF_REQUIRE(x, "x is NULL");
    const size_t total = (size_t)n * robot->desc.ndof;
    hipLaunchKernelGGL(clamp_kernel, dim3(grid_for(total)), dim3(kBlock), 0, (hipStream_t)stream, robot->chain, total, x);
    return check_launch();
}

}  // extern "C"

namespace {

// cppf_lm_params -> the kernels' LmK (validation included); n / W are the caller's to fill
int make_lm_kernel_params(const cppf_robot* robot, const cppf_lm_params* params, LmK& prm) {
    CPPF_REQUIRE(params, "params is NULL");
    CPPF_REQUIRE(params->n_steps >= 1, "n_steps must be >= 1");
    CPPF_REQUIRE(params->clamp == 1 || params->n_steps == 1, "clamp = 0 is only defined for a single step");
    CPPF_REQUIRE(params->lm_lambda > 0.f, "lm_lambda must be > 0");
    CPPF_REQUIRE(params->alpha_position > 0.f && params->alpha_rotation > 0.f, "alpha_position / alpha_rotation must be > 0");
    CPPF_REQUIRE(params->solver == CPPF_SOLVER_AUTO || params->solver == CPPF_SOLVER_F32 || params->solver == CPPF_SOLVER_F64,
                 "unknown solver");
    CPPF_REQUIRE(params->solver_gate >= 0.f, "solver_gate must be >= 0 (0 = the default tolerance)");
    CPPF_REQUIRE(params->shape == CPPF_SHAPE_AUTO || params->shape == CPPF_SHAPE_ROW || params->shape == CPPF_SHAPE_QUAD,
                 "unknown kernel shape");
    CPPF_REQUIRE(params->tol_pos_m >= 0.f && params->tol_rot_rad >= 0.f, "early-out tolerances must be >= 0");
    CPPF_REQUIRE((params->tol_pos_m > 0.f) == (params->tol_rot_rad > 0.f), "set both early-out tolerances or neither");
    prm.lm_lambda = params->lm_lambda;
    prm.a_pos = params->alpha_position;
    prm.a_rot = params->alpha_rotation;
    // the damping per row of the dual system (kernels_chain.h), formed once here instead of by every wavefront
    prm.lam_r_d = (double)params->lm_lambda / ((double)params->alpha_rotation * (double)params->alpha_rotation);
    prm.lam_p_d = (double)params->lm_lambda / ((double)params->alpha_position * (double)params->alpha_position);
    prm.lam_r = (float)prm.lam_r_d;
    prm.lam_p = (float)prm.lam_p_d;
    // conditioning gate (lm_solve_gated): redo a row's solve in double precision when eps * a_max * max diag(A) * max |y| > tau
    const float tau = params->solver_gate > 0.f ? params->solver_gate : CPPF_SOLVER_GATE_DEFAULT;
    const float a_max = std::fmax(params->alpha_position, params->alpha_rotation);
    prm.gate_thr = params->solver == CPPF_SOLVER_F32 ? INFINITY : params->solver == CPPF_SOLVER_F64 ? -INFINITY : tau / (6e-8f * a_max);
    // ... and, in the lean iterations of a fused launch, only when that estimate is also more than kGateRel of the residual the step
    // reduces (kernels_fused.h: an intermediate iterate needs a step that is accurate RELATIVE to its residual)
    const float rel = 1e-6f * (float)tune(robot, CPPF_TUNE_GATE_REL_PPM) / (6e-8f * a_max);  // (kGateRel unless a test changed it)
    prm.gate_rel2 = rel * rel;
    // fair-share pacing (kernels_fused.h: lm_pace), opt-in per handle: CPPF_TUNE_LM_PACE = 0 off (default), > 0 ticks per iteration,
    // < 0 the built-in estimate: 0.55 x the iteration's ~(200 + 56 d) VALU instructions ~ four wavefronts' share of a SIMD that issues
    // one every ~2.6 cycles (+ the longer first / last iterations), in 10 ns ticks (Panda: 326; the measured plateau is 300 .. 360).  launch_fused_rows drops it for launches
    // that do not fill the chip; early-out launches have no schedule.
    const int pace = tune(robot, CPPF_TUNE_LM_PACE);
    prm.pace_ticks = (pace == 0 || params->tol_pos_m > 0.f || params->n_steps < 3) ? 0 : (pace > 0 ? pace : (int)(0.55f * (200.f + 56.f * (float)robot->desc.ndof) + 0.5f));
    prm.n_steps = params->n_steps;
    prm.clamp = params->clamp;
    prm.n = 0;
    prm.W = 0;
    // (squared tolerances; a positive tolerance whose square underflows still means "early-out on": the smallest normal float)
    prm.tol_pos2 = params->tol_pos_m > 0.f ? std::fmax(params->tol_pos_m * params->tol_pos_m, 1.17549435e-38f) : 0.f;
    prm.tol_rot2 = params->tol_rot_rad > 0.f ? std::fmax(params->tol_rot_rad * params->tol_rot_rad, 1.17549435e-38f) : 0.f;
    return CPPF_OK;
}

inline bool outputs_want_collision(const cppf_lm_outputs& o) {
    return o.self_mask || o.env_mask || o.jlim_mask || o.ext_cost || o.min_self || o.min_env || o.seed_summary;
}
// the per-seed summary is an epilogue of the fused launch when a 256-row workgroup holds whole seeds (W = 64, 128, 256)
inline bool summary_in_launch(int W) { return W >= 64 && kBlock % W == 0 && (W & (W - 1)) == 0; }

// One launch of the row-shape fused kernel over `grid` workgroups: the problem `single` (table == NULL) or the problems of a device
// table (cppf_lm_batch_*).  coll = lm_fused_kernel's COLL; n_rows = all rows of the launch (what the residency claim goes by).
int launch_fused_rows(const cppf_robot* robot, int coll, size_t n_rows, unsigned grid, hipStream_t st, const LmK& prm,
                      const BatchItemK& single, const void* table) {
    // Dynamic LDS: what the generic kernels stage their capsules in, or -- for a launch of at most two workgroups per compute
    // unit -- a claim sized so that only two workgroups FIT on one (fused_spread_lds): several such launches in flight then
    // spread over the whole chip instead of stacking four deep on the compute units the dispatcher tries first.
    const bool generic = !use_rtc(robot) && !use_table(robot);
    const size_t spread = fused_spread_lds(robot, n_rows);
    const size_t lds_need = (generic && coll) ? robot->lds_bytes : 0;
    // the generic kernels stage 6 floats per capsule per lane: with the gate's slots beside them, 12 joints x 24 capsules no longer
    // fit the 160 KB of a compute unit (the launch would take the process down) -- such a robot has to be specialised
    if (generic && coll && lds_need + fused_static_lds(robot) > (size_t)160 * 1024)
        return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: the generic kernels cannot stage this many capsules at this ndof; cppf_robot_specialize() the robot");
    FusedArgs fa;
    fa.ch = robot->chain;
    fa.co = robot->coll;
    fa.prm = prm;
    // (the schedule is that of ONE resident round of FOUR wavefronts per SIMD: a launch that leaves a quarter of the chip's slots empty, or
    // needs a second round, or whose kernel holds fewer wavefronts per SIMD -- lm_waves(): specialised chains beyond 7 joints, generic
    // ones beyond 6 -- is not paced: measured on Fetch, 8 joints, three per SIMD: +2 .. 3 %, profiles/r5_pace_sweep.txt)
    {
        const unsigned long long slots = (unsigned long long)(robot->cu_count > 0 ? robot->cu_count : 256) * 4ull;  // workgroups of 256 rows at four wavefronts per SIMD
        const int d = robot->desc.ndof;
        const bool four = (use_rtc(robot) || use_table(robot)) ? d <= 7 : d <= 6;
        if (!four || (unsigned long long)grid * 4ull < 3ull * slots || (unsigned long long)grid > slots) fa.prm.pace_ticks = 0;
    }
    fa.single = single;
    fa.table = table;
    if (use_rtc(robot)) {
        if (int rc = rtc_launch(robot, coll == 0 ? RTC_FUSED0 : (coll == 2 ? RTC_FUSED2 : RTC_FUSED1), &lm_fused_kernel<DynRobot<6>, 0>, grid,
                                kBlock, spread, st, fa.ch, fa.co, fa.prm, fa.single, fa.table))
            return rc;
    } else if (!generic) {
        // a generated table: the kernel lives in fused_static.hip
        if (!launch_fused_static(robot->static_id, coll, grid, spread, st, fa))
            return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: no fused kernel for this generated table");
    } else {
        const size_t lds = std::max(lds_need, spread);
        const int rc = for_dyn_robot(robot, [&](auto tag) {
            using RB = typename decltype(tag)::type;
            const auto kernel = coll == 2 ? lm_fused_kernel<RB, 2> : coll == 1 ? lm_fused_kernel<RB, 1> : lm_fused_kernel<RB, 0>;
            return launch(kernel, dim3(grid), dim3(kBlock), lds, st, fa.ch, fa.co, fa.prm, fa.single, fa.table);
        });
        if (rc) return rc;
    }
    return check_launch();
}

// One launch of the quad-shape kernel (kernels_quad.h) over n rows; `gate` = { NULL } unless the optimiser loop on the device asks.
// The callers hold ndof >= 6 (quad_possible, cppf_lm_optimize_enqueue_pinned): below that there is no such kernel on any route.
int launch_quad(const cppf_robot* robot, bool coll, size_t n, hipStream_t st, const LmK& prm, const float* x_in, const float* target,
                const cppf_lm_outputs& oq, const StepGateK gate) {
    const unsigned grid = (unsigned)((n + kQuadRows - 1) / kQuadRows);
    const size_t lds_q = coll ? sizeof(float) * (4 * (CPPF_MAX_PAIRS + CPPF_MAX_CAPSULES) +
                                                 (size_t)kQuadRows * quad_row_stride(robot->coll.ncaps))
                              : 0;
    const uint4* tab = static_cast<const uint4*>(robot->d_quad);
    const bool mfma = tune(robot, CPPF_TUNE_QUAD_MFMA) && use_table(robot);
    using QuadKernel = decltype(&lm_quad_kernel<DynRobot<6>, 0, false>);
    const auto pick = [&](auto tag) -> QuadKernel {
        using RB = typename decltype(tag)::type;
        if constexpr (RB::D >= 6) {  // (the quad shape solves the dual 6x6 system)
            constexpr bool kTable = RB::kStatic;  // the MFMA form is instantiated for the generated tables only
            return coll ? (mfma ? lm_quad_kernel<RB, 1, kTable> : lm_quad_kernel<RB, 1, false>)
                        : (mfma ? lm_quad_kernel<RB, 0, kTable> : lm_quad_kernel<RB, 0, false>);
        } else
            return nullptr;
    };
    return launch_routed(robot, coll ? RTC_QUAD1 : RTC_QUAD0, pick, grid, kBlock, lds_q, st, robot->chain, robot->coll, prm, x_in, target, oq, tab,
                         gate);
}

inline bool quad_possible(const cppf_robot* robot, const cppf_lm_outputs& out) {
    return robot->desc.ndof >= 6 && !out.J_out && !out.e_out && !out.min_self && !out.min_env &&
           (!out.seed_summary || (out.x_out && out.pos_err_m && out.rot_err_rad && out.self_mask && out.env_mask && out.jlim_mask &&
                                  out.ext_cost));
}

// cppf_collision_masks; with a gate (the optimiser loop on the device) only the trajectories it opens are evaluated
int collision_masks_gated(const cppf_robot* robot, const float* q, int S, int W, uint8_t* self_mask, uint8_t* env_mask,
                          uint8_t* jlim_mask, float* ext_cost, float* min_self, float* min_env, void* stream, const StepGateK gate) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(S >= 0 && W >= 0, "S / W < 0");
    const size_t n = (size_t)S * W;
    if (n == 0) return CPPF_OK;
    CPPF_REQUIRE(n <= 0x7fffffffu, "S*W exceeds 2^31-1 rows");
    CPPF_REQUIRE(q, "q is NULL");
    hipStream_t st = (hipStream_t)stream;
    const bool want_min = min_self || min_env;
    const size_t lds = (use_rtc(robot) || use_table(robot)) ? 0 : robot->lds_bytes;  // only the generic kernel stages its capsules
    const auto pick = [&](auto tag) {
        using RB = typename decltype(tag)::type;
        return want_min ? collision_kernel<RB, true> : collision_kernel<RB, false>;
    };
    const int rc = launch_routed(robot, want_min ? RTC_COLL_MIN : RTC_COLL_MASK, pick, grid_for(n), kBlock, lds, st, robot->chain, robot->coll,
                                 (int)n, q, self_mask, env_mask, jlim_mask, ext_cost, min_self, min_env, gate, W);
    return rc ? rc : check_launch();
}

// Which elimination a coupled step of S trajectories of W waypoints resolves to on this handle (see the comments at the launches
// in run_full_step).  Depends on the sizes, the parameters and the handle's tuning only (t_pcr_lds: CPPF_TUNE_PCR_LDS as the plan
// read it), so plan_full_step knows it before anything is launched.
enum class FullStepForm {
    LaneVar,  // individually weighted differencing rows: one lane per trajectory, couplings read from memory
    Pcr,      // parallel in time
    Rows,     // one block row per lane
    Wave,     // one wavefront per trajectory (takes no pinned end)
    Lane,     // one lane per trajectory
    Local,    // the pose block without differencing rows: no elimination, every waypoint solved where its block is built, in fp64
};
FullStepForm full_step_form(const cppf_robot* robot, size_t n, int W, bool use_pose, bool use_diff, bool var_coupling, int t_pcr_lds) {
    const int ndof = robot->desc.ndof;
    const int t_pcr_rows = tune(robot, CPPF_TUNE_PCR_MAX_ROWS);
    const bool g_rows_pose = tune(robot, CPPF_TUNE_ROWS_POSE) != 0, g_full_rows = tune(robot, CPPF_TUNE_FULL_ROWS) != 0;
    const size_t pcr_rows = t_pcr_rows >= 0 ? (size_t)t_pcr_rows : (size_t)((W <= 256 && t_pcr_lds != 0) ? kPcrMaxRowsLds : kPcrMaxRowsGlobal);
    const size_t pcr_limit = pcr_rows * (ndof <= 7 ? 100 : 50) / 100;
    if (use_pose && !use_diff) return FullStepForm::Local;
    if (var_coupling) return FullStepForm::LaneVar;
    if (!use_pose && W <= 512 && n <= pcr_limit && ndof >= 3 && ndof <= 8) return FullStepForm::Pcr;
    if ((!use_pose || g_rows_pose) && g_full_rows && ndof >= 3 && ndof <= 12 && W <= (1 << 19)) return FullStepForm::Rows;
    // with the pose block the one-lane kernel keeps the case (see run_full_step); 9 .. 12 joints have no one-wavefront form
    return ndof <= 8 && !use_pose ? FullStepForm::Wave : FullStepForm::Lane;
}

// Everything a coupled step is once its arguments are known: made and checked by plan_full_step, launched by run_full_step
enum class FullBlocks { Plain, Occ, Scene };  // full_blocks_kernel: the handle's cuboids, at two occupancies, or a scene's
struct FullStepPlan {
    FullK prm;  // (fold included)
    FullStepForm form;
    FullBlocks blocks;  // (under FullStepForm::Local the fp64 build of Plain or Scene)
    // the parallel-in-time sub-form: the state in LDS, and then split over 512 lanes | its lanes per trajectory (256 or 512), the
    // workgroups of the row-per-lane pair and of the one-lane kernels | the LDS bytes of the first two, and where in work_G the
    // individually weighted couplings live (in floats)
    bool pcr_in_lds, pcr_split;
    unsigned pcr_block, rows_wgs, lane_grid;
    size_t pcr_lds, rows_lds, w2next;
};

// The one place a coupled step is checked and decided: cppf_lm_full_step(_pinned), _scene (`scene`: its cuboids; never together with
// `gated`) and the differencing step of the optimiser loop on the device (`gated`).  From the arguments and the handle's tuning alone,
// each switch read once: no device is touched and nothing launched, so every refusal holds for a host-only handle too.
int plan_full_step(const cppf_robot* robot, int S, int W, const cppf_full_params* params, int pin, bool gated, const SceneStepK* scene,
                   FullStepPlan& plan) {
    CPPF_ROBOT_ALIVE(robot);
    CPPF_REQUIRE(params, "params is NULL");
    CPPF_REQUIRE(pin >= 0 && pin <= (CPPF_PIN_FIRST | CPPF_PIN_LAST), "pin_mask must be a combination of CPPF_PIN_FIRST and CPPF_PIN_LAST");
    CPPF_REQUIRE(S >= 0 && W >= 1, "S < 0 or W < 1");
    const size_t n = (size_t)S * W;
    CPPF_REQUIRE(n <= 0x7fffffffu, "S*W exceeds 2^31-1 rows");
    CPPF_REQUIRE(!scene || (scene->n_obs >= 0 && scene->n_obs <= CPPF_MAX_SCENE_OBSTACLES), "n_obs out of range (0 .. CPPF_MAX_SCENE_OBSTACLES)");
    CPPF_REQUIRE(!scene || scene->n_obs == 0 || (scene->box_lo && scene->box_hi), "box_lo / box_hi is NULL");
    CPPF_REQUIRE(params->lm_lambda > 0.f, "lm_lambda must be > 0");
    CPPF_REQUIRE(!params->use_virtual_configs || (params->n_virtual_configs > 0 && 2 * params->n_virtual_configs < W),
                 "2 * n_virtual_configs must be < number of waypoints (optimization_utils.py:449-451)");
    // the "satisfied" row options (cppflow/optimization_utils.py:514-533, 548-606)
    CPPF_REQUIRE(params->differencing_mode >= 0 && params->differencing_mode <= 2, "differencing_mode must be 0, 1 or 2");
    CPPF_REQUIRE(!params->pose_do_scale_down_satisfied || (params->pose_scale_down >= 0.f && params->pose_scale_down < 1.f),
                 "pose scale-down must be in [0, 1) (optimization_utils.py:305)");
    CPPF_REQUIRE(params->differencing_mode != 2 || (params->differencing_scale_down >= 0.f && params->differencing_scale_down < 1.f),
                 "differencing scale-down must be in [0, 1) (optimization_utils.py:367)");
    if (pin != 0 && (params->differencing_mode != 0 || params->pose_do_scale_down_satisfied))
        return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: a pinned end waypoint is not combined with the \"satisfied\" row options "
                                          "(differencing_mode != 0, pose_do_scale_down_satisfied)");
    FullK& prm = plan.prm;
    prm.lm_lambda = params->lm_lambda;
    prm.a_pos = params->alpha_position;
    prm.a_rot = params->alpha_rotation;
    prm.a_diff = params->alpha_differencing;
    prm.a_diff_pris = params->alpha_differencing_prismatic_scaling;
    prm.a_vq = params->alpha_virtual_configs;
    prm.a_self = params->alpha_self_collision;
    prm.a_env = params->alpha_env_collision;
    prm.use_pose = params->use_pose;
    prm.use_diff = params->use_differencing;
    prm.use_vq = params->use_virtual_configs;
    prm.n_vq = params->n_virtual_configs;
    prm.use_self = params->use_self_collisions;
    prm.use_env = params->use_env_collisions;
    prm.S = S;
    prm.W = W;
    prm.pin = pin;
    prm.pose_scale_satisfied = params->use_pose && params->pose_do_scale_down_satisfied;
    prm.pose_thr_m = params->pose_threshold_m;
    prm.pose_thr_rad = params->pose_threshold_rad;
    prm.pose_scale = params->pose_scale_down;
    prm.diff_mode = params->use_differencing ? params->differencing_mode : 0;
    prm.diff_thr_rad = params->differencing_threshold_rad;
    prm.diff_thr_m = params->differencing_threshold_m;
    prm.diff_scale = params->differencing_scale_down;
    prm.diff_shift_invalid = params->differencing_shift_invalid_to_threshold;
    // Individually weighted differencing rows: the coupling between waypoints t and t + 1 is no longer the same constant for
    // every t, which the tuned elimination kernels assume; such a step goes through the one-lane-per-trajectory kernel with the
    // couplings read from memory (w2next: the spare tail of work_G -- that kernel keeps d(d+1)/2 of the d*d floats per row).
    const int d = robot->desc.ndof;
    plan.w2next = n * (size_t)(d * (d + 1) / 2);
    const int t_pcr_lds = tune(robot, CPPF_TUNE_PCR_LDS);
    plan.form = full_step_form(robot, n, W, prm.use_pose != 0, prm.use_diff != 0, /*var_coupling=*/prm.diff_mode != 0, t_pcr_lds);
    prm.fold = plan.form != FullStepForm::Pcr;  // (the parallel-in-time kernel assembles the terms itself: FullK::fold)
    // full_solve_wave_kernel: up to 8 joints, no pose block, and neither the parallel-in-time nor the row-per-lane form -- which is
    // CPPF_TUNE_FULL_ROWS = 0 beyond the parallel-in-time sizes, and also fewer than 3 joints or more than 2^19 waypoints, where the
    // row-per-lane form does not exist.
    if (pin != 0 && S >= 1 && plan.form == FullStepForm::Wave)
        return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: the one-wavefront-per-trajectory elimination (what a step resolves to under "
                                          "CPPF_TUNE_FULL_ROWS = 0, with fewer than 3 joints or beyond 2^19 waypoints) takes no "
                                          "pinned end waypoint");
    if (gated && plan.form != FullStepForm::Pcr && plan.form != FullStepForm::Rows)
        return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: the device-side optimiser loop gates the parallel-in-time and the row-per-lane "
                                          "elimination only (no pose block, no individually weighted differencing rows, CPPF_TUNE_FULL_ROWS on)");
    // Local -- six pose rows against seven or eight joints and nothing else on the diagonal but lambda: the blocks in fp64, solved
    // by the lane that builds them (full_local_solve), which writes x_out.  The unconstrained build at every size: the fp64 block
    // is 2 x d(d+3)/2 registers on top of the rows'.
    // A scene -- outside Local, too, ONE instantiation per robot, the unconstrained build: a planner steps S <= 8 trajectories, far
    // below the row count at which the occupancy-bound build of the handle form pays.  (A handle specialised at run time takes the
    // generic form, like every coupled step: for_robot.)
    plan.blocks = scene ? FullBlocks::Scene : n >= 131072 && plan.form != FullStepForm::Local ? FullBlocks::Occ : FullBlocks::Plain;
    // the parallel-in-time sub-forms: the state in LDS (W <= 256: 256 x ((d(d+1)/2 + d + d^2) | 1) floats), on 256 lanes or split over
    // 512 (see kPcrSplitMaxD; CPPF_TUNE_PCR_LDS = 3 forces the split form), else in the workspace, on 256 or 512 lanes
    plan.pcr_in_lds = W <= 256 && t_pcr_lds != 0;
    plan.pcr_split = plan.pcr_in_lds && t_pcr_lds != 1 && (d <= kPcrSplitMaxD || t_pcr_lds == 3);
    plan.pcr_block = plan.pcr_split || W > 256 ? 512 : 256;
    plan.pcr_lds = plan.pcr_in_lds ? 256 * (size_t)((d * (d + 1) / 2 + d + d * d) | 1) * sizeof(float) : 0;
    // row-per-lane kernels: 8 trajectories per one-wavefront workgroup and two workgroups (the two ends of the path) per 8
    // trajectories; the LDS reservation caps the workgroups per compute unit at ceil(#workgroups / 256) (160 KB per compute
    // unit), which spreads a small launch over distinct compute units
    const int rows_tpw = d <= 8 ? 8 : 4;  // trajectories per wavefront: 8 or 16 lanes each
    plan.rows_wgs = 2u * (unsigned)((S + rows_tpw - 1) / rows_tpw);
    const unsigned rows_per_cu = (plan.rows_wgs + 255) / 256;
    plan.rows_lds = rows_per_cu == 1 ? 96 * 1024 : rows_per_cu == 2 ? 64 * 1024 : rows_per_cu == 3 ? 48 * 1024 : 0;
    plan.lane_grid = (unsigned)((S + 63) / 64);
    return CPPF_OK;
}

// The launches of a planned coupled step.  With a gate (the optimiser loop on the device) only the trajectories it opens are stepped;
// `scene` is the one the plan was made with (the environment rows come from its cuboids, not the handle's).  The pointers are the
// last thing checked, still before the device is selected.
int run_full_step(const cppf_robot* robot, const FullStepPlan& plan, const float* x_in, const float* target, const float* virtual_configs,
                  float* work_blocks, float* work_G, float* work_y, float* x_out, void* stream, const StepGateK gate,
                  const SceneStepK* scene = nullptr) {
    const FullK& prm = plan.prm;
    const int S = prm.S;
    CPPF_REQUIRE(x_out != x_in, "x_out must not alias x_in (the back substitution reads x_in)");
    CPPF_REQUIRE(S == 0 || (x_in && target && work_blocks && work_G && work_y && x_out), "NULL pointer");
    CPPF_ENTER(robot);
    if (S == 0) return CPPF_OK;
    float* const w2next = work_G + plan.w2next;
    hipStream_t st = (hipStream_t)stream;
    const bool local = plan.form == FullStepForm::Local;
    const int rc = for_robot(robot, [&](auto tag) {
        using RB = typename decltype(tag)::type;
        // one argument list for the five instantiations in use; they differ in the tail: the scene's cuboids or the gate
        const auto blocks = [&](auto kernel, const auto& tail) {
            return launch(kernel, dim3(grid_for((size_t)S * prm.W)), dim3(kBlock), robot->lds_bytes, st, robot->chain, robot->coll, prm, x_in,
                          target, virtual_configs, work_blocks, w2next, tail, local ? x_out : (float*)nullptr);
        };
        if (plan.blocks == FullBlocks::Scene) {
            SceneStepK sc = *scene;
            sc.tile_cull2 = tile_cull_threshold(robot, 0.f);
            // (dynamic LDS as for the handle form beside it: chain12's 13 capsules are 78 KB in both)
            return blocks(local ? full_blocks_kernel<RB, 0, true, true> : full_blocks_kernel<RB, 0, true>, sc);
        }
        return blocks(local                             ? full_blocks_kernel<RB, 0, false, true>
                      : plan.blocks == FullBlocks::Occ ? full_blocks_kernel<RB, full_blocks_occ<RB>()>
                                                        : full_blocks_kernel<RB>,
                      gate);
    });
    if (rc) return rc;
    const uint32_t pris_mask = robot->chain.pris_mask;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        constexpr int D = decltype(dof)::D;
        switch (plan.form) {
            case FullStepForm::LaneVar:
                hipLaunchKernelGGL((full_solve_kernel<D, true>), dim3(plan.lane_grid), dim3(64), 0, st, prm, pris_mask, x_in, work_blocks,
                                   work_G, work_y, x_out, w2next);
                break;
            case FullStepForm::Pcr:
                // Up to ~128k rows (the planner's cadence is one trajectory): parallel cyclic reduction, one workgroup per
                // trajectory, one lane per waypoint; beyond that its O(T log T) work and traffic lose against the
                // waypoint-after-waypoint kernels.
                if constexpr (D <= 8) {  // (full_step_form: the parallel-in-time form exists for 3 .. 8 joints)
                    const auto kernel = plan.pcr_split          ? full_solve_pcr_kernel<D, 512, true, true>
                                        : plan.pcr_in_lds       ? full_solve_pcr_kernel<D, 256, true>
                                        : plan.pcr_block == 256 ? full_solve_pcr_kernel<D, 256>
                                                                : full_solve_pcr_kernel<D, 512>;
                    if (int rc2 = launch(kernel, dim3((unsigned)S), dim3(plan.pcr_block), plan.pcr_lds, st, robot->chain, prm, x_in,
                                         virtual_configs, work_blocks, work_G, x_out, gate))
                        return rc2;
                }
                break;
            case FullStepForm::Rows:  // (every ndof; sixteen lanes per trajectory at 9 .. 12 joints, see rows_tpw)
                if (int rc2 = launch(full_rows_eliminate_kernel<D>, dim3(plan.rows_wgs), dim3(64), plan.rows_lds, st, prm, pris_mask,
                                     work_blocks, work_G, work_y, gate))
                    return rc2;
                if (int rc2 = launch(full_rows_substitute_kernel<D>, dim3(plan.rows_wgs), dim3(64), plan.rows_lds, st, prm, pris_mask, x_in,
                                     work_blocks, work_G, work_y, x_out, gate))
                    return rc2;
                break;
            case FullStepForm::Wave:  // one trajectory per wavefront (8 x 8 lane tile), up to 8 joints
                if constexpr (D <= 8)
                    hipLaunchKernelGGL((full_solve_wave_kernel<D>), dim3((unsigned)S), dim3(64), 0, st, prm, pris_mask, x_in, work_blocks,
                                       work_G, work_y, x_out);
                break;
            case FullStepForm::Local: break;  // (full_blocks_kernel solved it)
            case FullStepForm::Lane:
                // With the pose block and differencing rows the d x d blocks are J^T J + a small diagonal (rank 6 of 7, cond ~1e7): this kernel's Cholesky
                // with floored pivots copes with that better than the explicit Gauss-Jordan inverse, so it keeps that case.
                hipLaunchKernelGGL((full_solve_kernel<D>), dim3(plan.lane_grid), dim3(64), 0, st, prm, pris_mask, x_in, work_blocks, work_G,
                                   work_y, x_out, nullptr);
                break;
        }
        return check_launch();
    });
}

}  // namespace

// A batched fused launch (cppflow_hip.h): the item descriptors live in a device table the batch object owns.
struct cppf_lm_batch {
    const cppf_robot* robot;  // counted in robot->life from create to destroy: never dangling
    int device;               // the robot's, copied: destroy does not need the robot for anything but the count
    LmK prm;
    void* d_table;        // { BatchHeadK ; BatchItemK[n_items] }
    int n_items, coll;
    unsigned grid;
    size_t n_rows;
    std::vector<cppf_lm_batch_item> after;  // items whose per-seed summary needs the separate reduction launch (W not 64 / 128 / 256)
};

extern "C" {

int cppf_lm_pose_steps(const cppf_robot* robot, const float* x_in, const float* target, int S, int W,
                       const cppf_lm_params* params, const cppf_lm_outputs* out, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(params && out, "params / out is NULL");
    CPPF_REQUIRE(S >= 0 && W >= 0, "S / W < 0");
    LmK prm;
    if (int rc = make_lm_kernel_params(robot, params, prm)) return rc;
    const size_t n = (size_t)S * W;
    if (n == 0) return CPPF_OK;
    CPPF_REQUIRE(n <= 0x7fffffffu, "S*W exceeds 2^31-1 rows");
    CPPF_REQUIRE(x_in && target, "x_in / target is NULL");
    prm.n = (int)n;
    prm.W = W;
    CPPF_REQUIRE(!(params->tol_pos_m > 0.f && (out->J_out || out->e_out)), "early-out is not combinable with J_out / e_out");
    const bool coll = outputs_want_collision(*out);
    hipStream_t st = (hipStream_t)stream;
    // per-seed summary: fused into the launch when a workgroup holds whole seeds, else the separate reduction afterwards
    cppf_lm_outputs outk = *out;
    float* const summary_dst = out->seed_summary;
    const bool summary_after = out->seed_summary && !summary_in_launch(W);
    if (summary_after) {
        CPPF_REQUIRE(out->x_out && out->pos_err_m && out->rot_err_rad && out->self_mask && out->env_mask &&
                         out->jlim_mask && out->ext_cost,
                     "seed_summary with W not in {64, 128, 256} needs x_out, pos_err_m, rot_err_rad, the three masks and ext_cost");
        outk.seed_summary = nullptr;
    }
    // kernel shape: four lanes per row for batches that cannot fill the chip (kernels_quad.h), one row per lane otherwise
    const bool quad_can = quad_possible(robot, *out);
    CPPF_REQUIRE(params->shape != CPPF_SHAPE_QUAD || quad_can,
                 "CPPF_SHAPE_QUAD needs ndof >= 6, no J_out / e_out / min_self / min_env, and (with seed_summary) every per-row output");
    // AUTO: the quad shape when the batch is at most one of its wavefronts per SIMD AND no per-seed summary is asked for (in
    // this shape a seed's rows span several workgroups, so the summary needs the separate reduction launch, which costs more
    // than the shape saves: measured 28.5 against 26.2 us for K = 10 + collision + summary at <= 16 384 rows)
    const bool quad = params->shape == CPPF_SHAPE_QUAD ||
                      (params->shape == CPPF_SHAPE_AUTO && quad_can && !out->seed_summary && n <= (size_t)tune(robot, CPPF_TUNE_QUAD_MAX_ROWS));
    if (quad) {
        cppf_lm_outputs oq = *out;
        oq.seed_summary = nullptr;  // rows of a seed span several workgroups in this shape: the reduction kernel follows
        if (int rc = launch_quad(robot, coll, n, st, prm, x_in, target, oq, StepGateK{nullptr, 0, 0u})) return rc;
        if (int rc = check_launch()) return rc;
        if (summary_dst)
            return cppf_seed_summary(robot, oq.x_out, S, W, oq.ext_cost, oq.pos_err_m, oq.rot_err_rad, oq.self_mask, oq.env_mask,
                                     oq.jlim_mask, summary_dst, stream);
        return CPPF_OK;
    }
    // (the kernel gets `outk`: with the separate reduction its seed_summary is NULL -- handing it `*out` there made the in-launch
    // summary run on a W it is not built for and write up to n / 64 - S rows past the caller's [S,8] buffer before the reduction
    // kernel put the right values in: found by the sentinel-arena test of tests/test_gpu_round3.py)
    BatchItemK item;
    item.x_in = x_in, item.target = target, item.out = outk, item.n = (int)n, item.W = W;
    const int c = !coll ? 0 : ((out->min_self || out->min_env) ? 2 : 1);
    if (int rc = launch_fused_rows(robot, c, n, grid_for(n), st, prm, item, nullptr)) return rc;
    if (summary_after)
        return cppf_seed_summary(robot, outk.x_out, S, W, outk.ext_cost, outk.pos_err_m, outk.rot_err_rad, outk.self_mask,
                                 outk.env_mask, outk.jlim_mask, summary_dst, stream);
    return CPPF_OK;
}

int cppf_lm_batch_create(const cppf_robot* robot, int n_items, const cppf_lm_batch_item* items, const cppf_lm_params* params,
                         cppf_lm_batch** out) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(out, "out is NULL");
    *out = nullptr;
    CPPF_REQUIRE(items && n_items >= 1 && n_items <= CPPF_MAX_BATCH, "n_items must be in 1 .. CPPF_MAX_BATCH");
    LmK prm;
    if (int rc = make_lm_kernel_params(robot, params, prm)) return rc;
    CPPF_REQUIRE(params->shape != CPPF_SHAPE_QUAD, "a batched launch is the row shape (CPPF_SHAPE_AUTO or CPPF_SHAPE_ROW)");
    std::vector<unsigned char> host(sizeof(BatchHeadK) + (size_t)n_items * sizeof(BatchItemK));
    BatchHeadK* head = reinterpret_cast<BatchHeadK*>(host.data());
    BatchItemK* tab = reinterpret_cast<BatchItemK*>(host.data() + sizeof(BatchHeadK));
    std::vector<cppf_lm_batch_item> after;
    size_t blocks = 0, rows = 0;
    bool coll = false;
    for (int i = 0; i < n_items; ++i) {
        const cppf_lm_batch_item& it = items[i];
        CPPF_REQUIRE(it.S >= 1 && it.W >= 1, "every item needs S >= 1 and W >= 1");
        const size_t n = (size_t)it.S * it.W;
        CPPF_REQUIRE(n <= 0x7fffffffu, "S*W exceeds 2^31-1 rows");
        CPPF_REQUIRE(it.x_in && it.target, "x_in / target is NULL");
        CPPF_REQUIRE(!it.out.J_out && !it.out.e_out && !it.out.min_self && !it.out.min_env,
                     "J_out / e_out / min_self / min_env are not available in a batched launch");
        BatchItemK k;
        k.x_in = it.x_in, k.target = it.target, k.out = it.out, k.n = (int)n, k.W = it.W;
        if (it.out.seed_summary && !summary_in_launch(it.W)) {
            CPPF_REQUIRE(it.out.x_out && it.out.pos_err_m && it.out.rot_err_rad && it.out.self_mask && it.out.env_mask &&
                             it.out.jlim_mask && it.out.ext_cost,
                         "seed_summary with W not in {64, 128, 256} needs x_out, pos_err_m, rot_err_rad, the three masks and ext_cost");
            k.out.seed_summary = nullptr;
            after.push_back(it);
        }
        coll = coll || outputs_want_collision(it.out);
        tab[i] = k;
        blocks += grid_for(n);
        rows += n;
        head->block_end[i] = (uint32_t)blocks;
    }
    CPPF_REQUIRE(blocks <= 0x7fffffffu, "the batch exceeds 2^31-1 workgroups");
    for (int i = n_items; i < CPPF_MAX_BATCH; ++i) head->block_end[i] = 0xffffffffu;
    cppf_lm_batch* b = new (std::nothrow) cppf_lm_batch();
    if (!b) return fail(CPPF_ERR_HIP, "cppflow_hip: out of host memory");
    b->robot = robot, b->device = robot->device, b->prm = prm, b->d_table = nullptr, b->n_items = n_items, b->coll = coll ? 1 : 0;
    b->grid = (unsigned)blocks, b->n_rows = rows;
    b->after = after;
    hipError_t e = hipMalloc(&b->d_table, host.size());
    if (e == hipSuccess) e = hipMemcpy(b->d_table, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (b->d_table) (void)hipFree(b->d_table);
        delete b;
        return fail(CPPF_ERR_HIP, std::string("cppflow_hip: the batch's device table: ") + hipGetErrorString(e));
    }
    robot->life.fetch_add(1u, std::memory_order_acq_rel);  // (CPPF_ENTER saw the handle alive; the caller may not destroy it DURING this call)
    *out = b;
    return CPPF_OK;
}

int cppf_lm_batch_launch(const cppf_lm_batch* batch, void* stream) {
    CPPF_REQUIRE(batch, "batch is NULL");
    const cppf_robot* robot = batch->robot;
    CPPF_ENTER(robot);
    BatchItemK none;
    std::memset(&none, 0, sizeof none);
    if (int rc = launch_fused_rows(robot, batch->coll, batch->n_rows, batch->grid, (hipStream_t)stream, batch->prm, none, batch->d_table))
        return rc;
    for (const cppf_lm_batch_item& it : batch->after)
        if (int rc = cppf_seed_summary(robot, it.out.x_out, it.S, it.W, it.out.ext_cost, it.out.pos_err_m, it.out.rot_err_rad,
                                       it.out.self_mask, it.out.env_mask, it.out.jlim_mask, it.out.seed_summary, stream))
            return rc;
    return CPPF_OK;
}

void cppf_lm_batch_destroy(cppf_lm_batch* batch) {
    if (!batch) return;
    {
        DeviceGuard guard(batch->device);
        if (batch->d_table) (void)hipFree(batch->d_table);
    }
    cppf_robot* robot = const_cast<cppf_robot*>(batch->robot);
    delete batch;
    // the last batch of a handle that was destroyed meanwhile frees it
    if (robot->life.fetch_sub(1u, std::memory_order_acq_rel) == (kRobotDead | 1u)) robot_free(robot);
}

int cppf_collision_masks(const cppf_robot* robot, const float* q, int S, int W, uint8_t* self_mask, uint8_t* env_mask,
                         uint8_t* jlim_mask, float* ext_cost, float* min_self, float* min_env, void* stream) {
    return collision_masks_gated(robot, q, S, W, self_mask, env_mask, jlim_mask, ext_cost, min_self, min_env, stream,
                                 StepGateK{nullptr, 0, 0u});
}

int cppf_self_collision_distances(const cppf_robot* robot, const float* x, int n, float* dists, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(n >= 0, "n < 0");
    if (n == 0 || robot->coll.npairs == 0) return CPPF_OK;
    CPPF_REQUIRE(x && dists, "x / dists is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((distances_kernel<decltype(dof)::D, false>), dim3(grid_for(n)), dim3(kBlock), robot->lds_bytes, st,
                           robot->chain, robot->coll, n, x, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, dists);
        return check_launch();
    });
}

int cppf_env_collision_distances(const cppf_robot* robot, const float* x, int n, const float* cuboid, const float* Rt,
                                 float* dists, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(n >= 0, "n < 0");
    CPPF_REQUIRE(cuboid && Rt, "cuboid / Rt is NULL");
    float lo[3], hi[3];
    if (int rc = cuboid_corners(cuboid, Rt, lo, hi)) return rc;
    if (n == 0 || robot->coll.ncaps == 0) return CPPF_OK;
    CPPF_REQUIRE(x && dists, "x / dists is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((distances_kernel<decltype(dof)::D, true>), dim3(grid_for(n)), dim3(kBlock), robot->lds_bytes, st,
                           robot->chain, robot->coll, n, x, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], dists);
        return check_launch();
    });
}

int cppf_self_collision_distances_jacobian(const cppf_robot* robot, const float* x, int n, float* jac, float* dists,
                                           void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(n >= 0, "n < 0");
    if (n == 0 || robot->coll.npairs == 0) return CPPF_OK;
    CPPF_REQUIRE(x && jac, "x / jac is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((distance_jacobians_kernel<decltype(dof)::D, false>), dim3(grid_for(n)), dim3(kBlock), robot->lds_bytes, st,
                           robot->chain, robot->coll, n, x, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, jac, dists);
        return check_launch();
    });
}

int cppf_env_collision_distances_jacobian(const cppf_robot* robot, const float* x, int n, const float* cuboid,
                                          const float* Rt, float* jac, float* dists, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(n >= 0, "n < 0");
    CPPF_REQUIRE(cuboid && Rt, "cuboid / Rt is NULL");
    float lo[3], hi[3];
    if (int rc = cuboid_corners(cuboid, Rt, lo, hi)) return rc;
    if (n == 0 || robot->coll.ncaps == 0) return CPPF_OK;
    CPPF_REQUIRE(x && jac, "x / jac is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((distance_jacobians_kernel<decltype(dof)::D, true>), dim3(grid_for(n)), dim3(kBlock), robot->lds_bytes, st,
                           robot->chain, robot->coll, n, x, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], jac, dists);
        return check_launch();
    });
}

int cppf_pose_error_metrics(const cppf_robot* robot, const float* x, const float* target, int S, int W, float* pos_err_m,
                            float* rot_err_rad, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(S >= 0 && W >= 0, "S / W < 0");
    const size_t n = (size_t)S * W;
    if (n == 0) return CPPF_OK;
    CPPF_REQUIRE(n <= 0x7fffffffu, "S*W exceeds 2^31-1 rows");
    CPPF_REQUIRE(x && target, "x / target is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((pose_metrics_kernel<decltype(dof)::D>), dim3(grid_for(n)), dim3(kBlock), 0, st, robot->chain, robot->coll,
                           (int)n, W, x, target, pos_err_m, rot_err_rad);
        return check_launch();
    });
}

int cppf_track_paths(const cppf_robot* robot, const float* target, int T, int k, int S, const cppf_track_params* params,
                     const float* q0, float* q_out, float* pos_err_m, float* rot_err_rad, uint8_t* status, void* stream) {
    // every argument is checked before the device is selected (CPPF_ENTER), so that the checks hold for a host-only handle too
    CPPF_ROBOT_ALIVE(robot);
    CPPF_REQUIRE(params, "params is NULL");
    CPPF_REQUIRE(T >= 0 && k >= 0, "T / k < 0");
    CPPF_REQUIRE(S >= 1, "S (segments) must be >= 1");
    CPPF_REQUIRE(params->n_restart >= 1 && params->n_track >= 1, "n_restart / n_track must be >= 1");
    CPPF_REQUIRE(params->n_random_restarts >= 0, "n_random_restarts must be >= 0");
    CPPF_REQUIRE(params->max_jump_rad >= 0.f && params->max_jump_m >= 0.f, "max_jump_rad / max_jump_m must be >= 0 (0 = off)");
    cppf_lm_params lp = {};
    lp.lm_lambda = params->lm_lambda;
    lp.alpha_position = params->alpha_position;
    lp.alpha_rotation = params->alpha_rotation;
    lp.n_steps = std::max(params->n_restart, params->n_track);
    lp.clamp = 1;
    lp.tol_pos_m = params->tol_pos_m;
    lp.tol_rot_rad = params->tol_rot_rad;
    lp.shape = CPPF_SHAPE_ROW;
    lp.solver = CPPF_SOLVER_AUTO;
    lp.solver_gate = 0.f;
    LmK prm;
    if (int rc = make_lm_kernel_params(robot, &lp, prm)) return rc;
    prm.pace_ticks = 0;  // (a latency launch: no fair-share schedule)
    if (T == 0 || k == 0) return CPPF_OK;
    CPPF_REQUIRE(S <= T, "S (segments) must be <= T: every segment needs a waypoint");
    CPPF_REQUIRE((size_t)k * (size_t)S <= 0x7fffffffu && (size_t)k * (size_t)T <= 0x7fffffffu, "k*S / k*T exceeds 2^31-1");
    CPPF_REQUIRE(target && q_out && pos_err_m && rot_err_rad && status, "target / q_out / pos_err_m / rot_err_rad / status is NULL");
    CPPF_ENTER(robot);
    TrackK tk;
    tk.target = target, tk.q0 = q0, tk.q_out = q_out, tk.pos_err = pos_err_m, tk.rot_err = rot_err_rad, tk.status = status;
    tk.T = T, tk.k = k, tk.S = S;
    tk.n_restart = params->n_restart, tk.n_track = params->n_track, tk.n_random = params->n_random_restarts;
    tk.max_jump_rad = params->max_jump_rad, tk.max_jump_m = params->max_jump_m;
    tk.seed = params->seed, tk.call_index = params->call_index;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(((size_t)k * S + kTrackBlock - 1) / kTrackBlock);
    const auto pick = [](auto tag) { return &track_kernel<typename decltype(tag)::type>; };
    const int rc = launch_routed(robot, RTC_TRACK, pick, grid, kTrackBlock, 0, st, robot->chain, robot->coll, prm, tk);
    return rc ? rc : check_launch();
}

int cppf_seed_validity(const cppf_robot* robot, const float* x, const float* target, int S, int W, float* out,
                       void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(S >= 0 && W >= 1, "S < 0 or W < 1");
    if (S == 0) return CPPF_OK;
    CPPF_REQUIRE(x && target && out, "x / target / out is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((seed_validity_kernel<decltype(dof)::D>), dim3(S), dim3(64), 0, st, robot->chain, robot->coll, S, W, x, target, out);
        return check_launch();
    });
}

int cppf_seed_summary(const cppf_robot* robot, const float* x, int S, int W, const float* ext_cost, const float* pos_err_m,
                      const float* rot_err_rad, const uint8_t* self_mask, const uint8_t* env_mask,
                      const uint8_t* jlim_mask, float* out, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(S >= 0 && W >= 1, "S < 0 or W < 1");
    if (S == 0) return CPPF_OK;
    CPPF_REQUIRE(x && ext_cost && pos_err_m && rot_err_rad && self_mask && env_mask && jlim_mask && out, "NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((seed_summary_kernel<decltype(dof)::D>), dim3(S), dim3(64), 0, st, robot->chain, S, W, x, ext_cost, pos_err_m,
                           rot_err_rad, self_mask, env_mask, jlim_mask, out);
        return check_launch();
    });
}

int cppf_select_valid_seed_gathered(const cppf_robot* robot, const float* gathered, int n_chunks, int n_groups, int S_chunk,
                                    const cppf_constraints* constraints, int32_t* out, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(n_chunks >= 1 && n_groups >= 1 && S_chunk >= 0, "n_chunks, n_groups must be >= 1 and S_chunk >= 0");
    CPPF_REQUIRE((size_t)n_chunks * S_chunk <= 0x7fffffffu, "n_chunks * S_chunk exceeds 2^31-1 seeds");
    CPPF_REQUIRE(constraints && out && (gathered || S_chunk == 0), "NULL pointer");
    CPPF_REQUIRE(((uintptr_t)gathered & 15u) == 0, "the summaries must be 16-byte aligned");
    SelectK k;
    k.thr[0] = constraints->max_allowed_position_error_cm;
    k.thr[1] = constraints->max_allowed_rotation_error_deg;
    k.thr[2] = constraints->max_allowed_mjac_deg;
    k.thr[3] = constraints->max_allowed_mjac_cm;
    k.ignore_self = constraints->self_collisions_ignored;
    k.ignore_env = constraints->env_collisions_ignored;
    k.S_chunk = S_chunk, k.n_chunks = n_chunks, k.n_groups = n_groups;
    hipLaunchKernelGGL(select_valid_seed_kernel, dim3((unsigned)n_groups), dim3(256), 0, (hipStream_t)stream, gathered, k, out);
    return check_launch();
}

int cppf_select_valid_seed(const cppf_robot* robot, const float* seed_summary, int S, const cppf_constraints* constraints,
                           int32_t* out, void* stream) {
    return cppf_select_valid_seed_gathered(robot, seed_summary, 1, 1, S, constraints, out, stream);
}

int cppf_plan_metrics(const cppf_robot* robot, const float* x, const float* target, int S, int W, const uint8_t* self_mask,
                      const uint8_t* env_mask, const float* q_init, float* out, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(S >= 0 && W >= 1, "S < 0 or W < 1");
    if (S == 0) return CPPF_OK;
    CPPF_REQUIRE((size_t)S * W <= 0x7fffffffu, "S*W exceeds 2^31-1 rows");
    CPPF_REQUIRE(x && target && out, "x / target / out is NULL");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((plan_metrics_kernel<decltype(dof)::D>), dim3(S), dim3(64), 0, st, robot->chain, robot->coll, S, W, x, target,
                           self_mask, env_mask, q_init, out);
        return check_launch();
    });
}

int cppf_lm_full_step_pinned(const cppf_robot* robot, const float* x_in, const float* target, const float* virtual_configs, int S,
                             int W, const cppf_full_params* params, int pin_mask, float* work_blocks, float* work_G, float* work_y,
                             float* x_out, void* stream) {
    FullStepPlan plan;
    if (int rc = plan_full_step(robot, S, W, params, pin_mask, false, nullptr, plan)) return rc;
    return run_full_step(robot, plan, x_in, target, virtual_configs, work_blocks, work_G, work_y, x_out, stream, StepGateK{nullptr, 0, 0u});
}

int cppf_lm_full_step(const cppf_robot* robot, const float* x_in, const float* target, const float* virtual_configs, int S,
                      int W, const cppf_full_params* params, float* work_blocks, float* work_G, float* work_y,
                      float* x_out, void* stream) {
    return cppf_lm_full_step_pinned(robot, x_in, target, virtual_configs, S, W, params, 0, work_blocks, work_G, work_y, x_out,
                                    stream);
}

int cppf_lm_full_step_scene(const cppf_robot* robot, const float* x_in, const float* target, const float* virtual_configs, int S,
                            int W, const cppf_full_params* params, int pin_mask, const float* box_lo, const float* box_hi,
                            int n_obs, float* work_blocks, float* work_G, float* work_y, float* x_out, void* stream) {
    const SceneStepK scene{box_lo, box_hi, n_obs, 0.f};  // (the tile threshold: run_full_step, from the handle's radii)
    FullStepPlan plan;
    if (int rc = plan_full_step(robot, S, W, params, pin_mask, false, &scene, plan)) return rc;
    return run_full_step(robot, plan, x_in, target, virtual_configs, work_blocks, work_G, work_y, x_out, stream, StepGateK{nullptr, 0, 0u},
                         &scene);
}

}  // extern "C"

namespace {
// workspace of cppf_lm_optimize_enqueue, in floats (every section a multiple of 4 floats): snapshot | x_new | blocks | G | y |
// metrics [S,16] | self mask | env mask (one byte per row each)
struct OptloopLayout {
    size_t snapshot, x_new, blocks, G, y, metrics, self_mask, env_mask, total;
};
OptloopLayout optloop_layout(int d, size_t S, size_t W) {
    auto up = [](size_t v) { return (v + 3) & ~(size_t)3; };
    const size_t n = S * W, nt = (size_t)d * (d + 1) / 2;
    OptloopLayout L;
    L.snapshot = 0;
    L.x_new = L.snapshot + up(n * d);
    L.blocks = L.x_new + up(n * d);
    L.G = L.blocks + up(n * (nt + d));
    L.y = L.G + up(n * d * d);
    L.metrics = L.y + up(n * d);
    L.self_mask = L.metrics + up(S * 16);
    L.env_mask = L.self_mask + up((n + 3) / 4);
    L.total = L.env_mask + up((n + 3) / 4);
    return L;
}
}  // namespace

extern "C" {

int cppf_lm_optimize_workspace_bytes(const cppf_robot* robot, int S, int W, size_t* bytes) {
    CPPF_ROBOT_ALIVE(robot);
    CPPF_REQUIRE(bytes, "bytes is NULL");
    CPPF_REQUIRE(S >= 1 && W >= 1 && (size_t)S * W <= 0x7fffffffu, "S / W must be >= 1 and S*W at most 2^31-1");
    *bytes = optloop_layout(robot->desc.ndof, (size_t)S, (size_t)W).total * sizeof(float);
    return CPPF_OK;
}

int cppf_lm_optimize_control_bytes(int S, const cppf_optloop_params* params, size_t* bytes) {
    CPPF_REQUIRE(params && bytes, "params / bytes is NULL");
    CPPF_REQUIRE(S >= 1, "S must be >= 1");
    CPPF_REQUIRE(params->trace_capacity >= 0, "trace_capacity must be >= 0");
    *bytes = optloop_control_words(S, *params) * 4;
    return CPPF_OK;
}

int cppf_lm_optimize_enqueue(const cppf_robot* robot, float* x, const float* target, int S, int W,
                             const cppf_optloop_params* params, void* workspace, int32_t* control, int n_iterations,
                             void* stream) {
    return cppf_lm_optimize_enqueue_pinned(robot, x, target, S, W, params, 0, workspace, control, n_iterations, stream);
}

int cppf_lm_optimize_enqueue_pinned(const cppf_robot* robot, float* x, const float* target, int S, int W,
                                    const cppf_optloop_params* params, int pin_mask, void* workspace, int32_t* control,
                                    int n_iterations, void* stream) {
    // every argument is checked before the device is selected (CPPF_ENTER), so that the checks hold for a host-only handle too
    CPPF_ROBOT_ALIVE(robot);
    CPPF_REQUIRE(params, "params is NULL");
    CPPF_REQUIRE(S >= 1 && W >= 1, "S / W must be >= 1");
    CPPF_REQUIRE((size_t)S * W <= 0x7fffffffu, "S*W exceeds 2^31-1 rows");
    CPPF_REQUIRE(n_iterations >= 0, "n_iterations < 0");
    CPPF_REQUIRE(params->max_n_steps >= 1, "max_n_steps must be >= 1");
    CPPF_REQUIRE(params->return_if_valid_after_n_steps >= -1, "return_if_valid_after_n_steps must be >= 0, or -1 for none");
    CPPF_REQUIRE(params->on_pose_valid >= 0 && params->on_pose_valid <= 2, "on_pose_valid must be one of CPPF_OPT_ON_POSE_VALID_*");
    CPPF_REQUIRE(params->per_trajectory == 0 || params->per_trajectory == 1, "per_trajectory must be 0 or 1");
    CPPF_REQUIRE(params->trace_capacity >= 0, "trace_capacity must be >= 0");
    CPPF_REQUIRE(params->convergence_threshold >= 0.0, "convergence_threshold must be >= 0");
    cppf_lm_params lp = {};
    lp.lm_lambda = params->pose_lm_lambda;
    lp.alpha_position = params->pose_alpha_position;
    lp.alpha_rotation = params->pose_alpha_rotation;
    lp.n_steps = 1;
    lp.clamp = 0;
    lp.shape = CPPF_SHAPE_AUTO;
    lp.solver = CPPF_SOLVER_AUTO;
    LmK prm;
    if (int rc = make_lm_kernel_params(robot, &lp, prm)) return rc;
    CPPF_REQUIRE(x && target && workspace && control, "x / target / workspace / control is NULL");
    CPPF_REQUIRE(((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)control & 3u) == 0, "workspace must be 16-byte, control 4-byte aligned");
    const int d = robot->desc.ndof;
    const size_t n = (size_t)S * W;
    // the gated steps are the kernels the host loop's launches resolve to at these sizes (same instructions, same bits)
    if (use_rtc(robot))
        return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: the device-side optimiser loop runs the compiled-in kernels; this handle was specialised at run time");
    if (d < 6 || n > (size_t)tune(robot, CPPF_TUNE_QUAD_MAX_ROWS))
        return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: the device-side optimiser loop needs the quad-shape pose step (ndof >= 6, S*W within its row limit)");
    if (params->diff.use_pose || params->diff.differencing_mode != 0)
        return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: the device-side optimiser loop takes a coupled step without pose block and without weighted differencing rows");
    // ... and so is the coupled step, whole: checked and decided here, once for every iteration, before the pose step's launch
    // writes x_new
    FullStepPlan diff_step;
    if (int rc = plan_full_step(robot, S, W, &params->diff, pin_mask, true, nullptr, diff_step)) return rc;
    if (n_iterations == 0) return CPPF_OK;
    CPPF_ENTER(robot);
    prm.n = (int)n;
    prm.W = W;
    hipStream_t st = (hipStream_t)stream;
    const OptloopLayout L = optloop_layout(d, (size_t)S, (size_t)W);
    float* const ws = static_cast<float*>(workspace);
    float* const x_new = ws + L.x_new;
    float* const metrics = ws + L.metrics;
    const bool want_masks = !(params->constraints.self_collisions_ignored && params->constraints.env_collisions_ignored);
    uint8_t* const self_m = reinterpret_cast<uint8_t*>(ws + L.self_mask);
    uint8_t* const env_m = reinterpret_cast<uint8_t*>(ws + L.env_mask);
    const StepGateK g_pose{control, params->per_trajectory, 1u << CPPF_OPT_MODE_POSE};
    const StepGateK g_diff{control, params->per_trajectory, 1u << CPPF_OPT_MODE_DIFF};
    const StepGateK g_live{control, params->per_trajectory, (1u << CPPF_OPT_MODE_POSE) | (1u << CPPF_OPT_MODE_DIFF)};
    cppf_lm_outputs oq;
    std::memset(&oq, 0, sizeof oq);
    oq.x_out = x_new;
    const int C = params->per_trajectory ? S : 1;
    const size_t total = n * (size_t)d;
    for (int it = 0; it < n_iterations; ++it) {
        if (int rc = launch_quad(robot, false, n, st, prm, x, target, oq, g_pose)) return rc;
        if (int rc = run_full_step(robot, diff_step, x, target, x, ws + L.blocks, ws + L.G, ws + L.y, x_new, stream, g_diff)) return rc;
        hipLaunchKernelGGL(optloop_clamp_kernel, dim3(grid_for(total)), dim3(kBlock), 0, st, robot->chain, total, W, pin_mask, x_new, x, g_live);
        if (want_masks)
            if (int rc = collision_masks_gated(robot, x, S, W, self_m, env_m, nullptr, nullptr, nullptr, nullptr, stream, g_live)) return rc;
        const uint8_t* const sm = params->constraints.self_collisions_ignored ? nullptr : self_m;
        const uint8_t* const em = params->constraints.env_collisions_ignored ? nullptr : env_m;
        const int rc = for_ndof(d, [&](auto dof) {
            hipLaunchKernelGGL((optloop_metrics_kernel<decltype(dof)::D>), dim3(S), dim3(64), 0, st, robot->chain, robot->coll, S, W, x, target,
                               sm, em, metrics, g_live);
            return CPPF_OK;
        });
        if (rc) return rc;
        hipLaunchKernelGGL(optloop_decide_kernel, dim3(C), dim3(64), 0, st, *params, S, W, d, metrics, x, ws + L.snapshot, control);
        if (int rc2 = check_launch()) return rc2;
    }
    return CPPF_OK;
}

int cppf_mjacs(const cppf_robot* robot, const float* q, int k, int T, float prismatic_scaling, float* mjacs, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(k >= 1 && T >= 1, "k, T must be >= 1");
    if (T == 1) return CPPF_OK;
    CPPF_REQUIRE(q && mjacs, "q / mjacs is NULL");
    const size_t total = (size_t)k * k * (size_t)(T - 1);
    CPPF_REQUIRE(total <= ((size_t)1 << 40), "k*k*(T-1) exceeds 2^40 entries");
    CPPF_REQUIRE((total + 255) / 256 <= 0x7fffffffu, "grid too large");
    hipStream_t st = (hipStream_t)stream;
    return for_ndof(robot->desc.ndof, [&](auto dof) {
        hipLaunchKernelGGL((mjacs_kernel<decltype(dof)::D>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, q, k, T,
                           robot->chain.pris_mask, prismatic_scaling, mjacs);
        return check_launch();
    });
}

constexpr int kDpResidentMaxK = 1024;  // four destinations per workgroup x 256 compute units (dp_resident_kernel)

// dynamic LDS of dp_backtrace_kernel: the memo table as bytes when it fits (k <= 256, T k <= 60 KB), else 0 = walk it in global memory
static size_t dp_stage_bytes(int k, int T) { return (k <= 256 && (size_t)k * T <= 60 * 1024) ? (size_t)k * T : 0; }

// what cppf_dp_search and cppf_dp_search_tabled start with: q [k, T, d] -> qT [T, k, d], the cost row of the first waypoint, memo[:,0]
static int dp_transpose_launch(hipStream_t st, const float* q, const float* ext_cost, int k, int T, int d, float* work_qT,
                               float* work_costsT, int32_t* work_memoT) {
    const size_t total = (size_t)k * T * d;
    hipLaunchKernelGGL(dp_transpose_kernel, dim3(grid_for(total > (size_t)k ? total : (size_t)k)), dim3(256), 0, st, q, ext_cost, k, T, d,
                       work_qT, work_costsT);
    // memo[:,0] is never read by the back-trace's result but is read as a value: define it (search.py:154 zero-inits memo)
    CPPF_HIP(hipMemsetAsync(work_memoT, 0, sizeof(int32_t) * (size_t)k, st));
    return CPPF_OK;
}

// ... and end with: the best last candidate and its path, walked back through the memo table
static int dp_backtrace_launch(hipStream_t st, const float* q, const float* work_costsT, const int32_t* work_memoT, int k, int T, int d,
                               int32_t* best_idx, float* best_path) {
    const size_t stage = dp_stage_bytes(k, T);
    hipLaunchKernelGGL(dp_backtrace_kernel, dim3(1), dim3(256), stage, st, q, work_costsT, work_memoT, k, T, d, stage != 0, best_idx, best_path);
    return check_launch();
}

int cppf_dp_search(const cppf_robot* robot, const float* q, const float* ext_cost, int k, int T, float prismatic_scaling,
                   float* work_qT, float* work_costsT, int32_t* work_memoT, float* best_path, int32_t* best_idx, int mode,
                   void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(k >= 1 && T >= 1, "k, T must be >= 1");
    CPPF_REQUIRE(q && ext_cost && work_qT && work_costsT && work_memoT && best_path && best_idx, "NULL pointer");
    CPPF_REQUIRE((size_t)k * T * robot->desc.ndof <= 0x7fffffffu, "k*T*d exceeds 2^31-1");
    CPPF_REQUIRE(mode == CPPF_DP_AUTO || mode == CPPF_DP_RESIDENT || mode == CPPF_DP_LAUNCHES, "unknown dp_search mode");
    CPPF_REQUIRE(mode != CPPF_DP_RESIDENT || k <= kDpResidentMaxK, "CPPF_DP_RESIDENT: the resident launch holds at most 1024 candidates");
    hipStream_t st = (hipStream_t)stream;
    const int d = robot->desc.ndof;
    bool persistent = T >= 2 && k <= kDpResidentMaxK &&
                      (mode == CPPF_DP_RESIDENT || (mode == CPPF_DP_AUTO && tune(robot, CPPF_TUNE_DP_PERSISTENT)));
    DpResidentForm form{nullptr, 0, 0};
    if (persistent) {
        // The resident form is only CORRECT while all its workgroups are on the device together (they wait for each other's cost words).
        // Hold the grid against what this device can hold of this kernel -- occupancy x compute units -- instead of finding out by
        // spinning 2^22 reads: a partitioned / CU-masked / smaller device takes the per-waypoint launches straight away (AUTO), and a
        // forced CPPF_DP_RESIDENT is refused.  (Other work on the device -- a second resident search on another stream, a full-width
        // fused launch -- can still delay workgroups; the bounded waits stay as the safety net for that.)
        const int rc = for_ndof(d, [&](auto dof) {
            form = dp_resident_form<decltype(dof)::D>(k, tune(robot, CPPF_TUNE_DP_PERSISTENT));
            return CPPF_OK;
        });
        if (rc) return rc;
        int per_cu = 0;
        CPPF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, form.fn, form.block, 0));
        const int cus = tune(robot, CPPF_TUNE_CU_COUNT) >= 0 ? tune(robot, CPPF_TUNE_CU_COUNT) : robot->cu_count;  // (the test hook: a smaller device)
        if ((unsigned long long)per_cu * (unsigned long long)cus < form.grid) {
            if (mode == CPPF_DP_RESIDENT)
                return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: CPPF_DP_RESIDENT: this device cannot hold the resident launch's workgroups "
                                                  "together (occupancy x compute units < grid): use CPPF_DP_AUTO or CPPF_DP_LAUNCHES");
            persistent = false;
        }
    }
    if (persistent)  // every cost word starts as "not yet" (kernels_dp.h); 16-byte multiple, from the allocation's start
        CPPF_HIP(hipMemsetAsync(work_costsT, 0xFF, sizeof(float) * (size_t)k * T, st));
    if (int rc = dp_transpose_launch(st, q, ext_cost, k, T, d, work_qT, work_costsT, work_memoT)) return rc;
    if (persistent) {
        const int spin_log2 = tune(robot, CPPF_TUNE_DP_SPIN_LOG2);
        const uint32_t spin = spin_log2 <= 0 ? 0u : (1u << (spin_log2 > 30 ? 30 : spin_log2));
        const float* const qT = work_qT;
        KernelArgs args(form.fn, qT, ext_cost, k, T, robot->chain.pris_mask, prismatic_scaling, work_costsT, work_memoT, spin);
        CPPF_HIP(hipLaunchKernel(args.fn, dim3(form.grid), dim3((unsigned)form.block), args.ptr, 0, st));
        return dp_backtrace_launch(st, q, work_costsT, work_memoT, k, T, d, best_idx, best_path);
    }
    const int bpb = k >= 4096 ? 4 : (k >= 2048 ? 2 : 1);
    const unsigned blocks = (unsigned)((k + bpb - 1) / bpb);
    for (int t = 1; t < T; ++t) {
        const float* qp = work_qT + (size_t)(t - 1) * k * d;
        const float* qc = work_qT + (size_t)t * k * d;
        const int rc = for_ndof(d, [&](auto dof) {
            constexpr int D = decltype(dof)::D;
            // (the destinations per workgroup are a constant of the kernel)
            const auto step = bpb == 4 ? dp_step_kernel<D, 4> : bpb == 2 ? dp_step_kernel<D, 2> : dp_step_kernel<D, 1>;
            hipLaunchKernelGGL(step, dim3(blocks), dim3(256), 0, st, qp, qc, work_costsT + (size_t)(t - 1) * k, ext_cost, k, T, t,
                               robot->chain.pris_mask, prismatic_scaling, work_costsT + (size_t)t * k, work_memoT + (size_t)t * k);
            return CPPF_OK;
        });
        if (rc) return rc;
    }
    return dp_backtrace_launch(st, q, work_costsT, work_memoT, k, T, d, best_idx, best_path);
}

int cppf_dp_table_floats(int k, int T, size_t* n_floats) {
    if (!n_floats || k < 1 || T < 1) return fail(CPPF_ERR_INVALID, "cppf_dp_table_floats: k, T must be >= 1, n_floats non-NULL");
    const size_t kp = (size_t)((k + 63) / 64 * 64);
    *n_floats = (size_t)(T > 1 ? T - 1 : 0) * (size_t)k * kp + 32 * kp;  // + 32 rows the chain may read past the last slab
    return CPPF_OK;
}

int cppf_dp_search_tabled(const cppf_robot* robot, const float* q, const float* ext_cost, int k, int T, float prismatic_scaling,
                          float* work_qT, float* work_costsT, int32_t* work_memoT, float* work_table, float* best_path,
                          int32_t* best_idx, void* stream) {
    CPPF_ENTER(robot);
    CPPF_REQUIRE(k >= 1 && k <= 256 && T >= 1, "cppf_dp_search_tabled: 1 <= k <= 256, T >= 1 (cppf_dp_search has no limit on k)");
    CPPF_REQUIRE(q && ext_cost && work_qT && work_costsT && work_memoT && best_path && best_idx, "NULL pointer");
    CPPF_REQUIRE(T == 1 || work_table, "work_table is NULL");
    hipStream_t st = (hipStream_t)stream;
    const int d = robot->desc.ndof, kp = (k + 63) / 64 * 64;
    if (int rc = dp_transpose_launch(st, q, ext_cost, k, T, d, work_qT, work_costsT, work_memoT)) return rc;
    if (T >= 2) {
        CPPF_REQUIRE(T - 1 <= 65535, "cppf_dp_search_tabled: T <= 65536");
        const int rc = for_ndof(d, [&](auto dof) {
            hipLaunchKernelGGL((dp_table_kernel<decltype(dof)::D>), dim3((unsigned)((kp + 255) / 256), (unsigned)((k + 7) / 8), (unsigned)(T - 1)),
                               dim3(256), 0, st, work_qT, k, kp, T, robot->chain.pris_mask, prismatic_scaling,
                               reinterpret_cast<uint32_t*>(work_table));
            return CPPF_OK;
        });
        if (rc) return rc;
        const uint32_t* tab = reinterpret_cast<const uint32_t*>(work_table);
        const auto chain = kp == 64 ? dp_chain_kernel<64> : kp == 128 ? dp_chain_kernel<128> : kp == 192 ? dp_chain_kernel<192> : dp_chain_kernel<256>;
        hipLaunchKernelGGL(chain, dim3(1), dim3(512), 0, st, tab, ext_cost, k, T, work_costsT);
        hipLaunchKernelGGL(dp_memo_kernel, dim3((unsigned)((k + 63) / 64), (unsigned)(T - 1)), dim3(256), 0, st, tab, ext_cost,
                           work_costsT, k, kp, T, work_memoT);
    }
    return dp_backtrace_launch(st, q, work_costsT, work_memoT, k, T, d, best_idx, best_path);
}

static size_t dp_nbest_workspace_words(int k, int T, int n_paths) {  // idxT [T][k], order / alive / far [k], sel [n_paths]
    return (size_t)T * k + 3 * (size_t)k + (size_t)n_paths;
}

int cppf_dp_nbest_workspace_bytes(int k, int T, int n_paths, size_t* bytes) {
    CPPF_REQUIRE(bytes, "bytes is NULL");
    CPPF_REQUIRE(k >= 1 && T >= 1 && n_paths >= 1, "k, T, n_paths must be >= 1");
    CPPF_REQUIRE((size_t)k * T <= 0x7fffffffu, "k*T exceeds 2^31-1");
    *bytes = up16(dp_nbest_workspace_words(k, T, n_paths) * sizeof(int32_t));
    return CPPF_OK;
}

int cppf_dp_nbest(const cppf_robot* robot, const float* q, const float* costsT, const int32_t* memoT, int k, int T, int n_paths,
                  float min_separation, float prismatic_scaling, void* workspace, float* paths, int32_t* path_idx, float* path_cost,
                  int32_t* n_found, void* stream) {
    // every argument is checked before the device is selected (CPPF_ENTER), so that the checks hold for a host-only handle too
    CPPF_ROBOT_ALIVE(robot);
    CPPF_REQUIRE(k >= 1 && T >= 1 && n_paths >= 1, "k, T, n_paths must be >= 1");
    CPPF_REQUIRE(std::isfinite(min_separation) && min_separation >= 0.f, "min_separation must be finite and >= 0");
    CPPF_REQUIRE(q && costsT && memoT && workspace && paths && path_idx && path_cost && n_found, "NULL pointer");
    CPPF_REQUIRE(((uintptr_t)workspace & 15u) == 0, "workspace must be 16-byte aligned");
    const int d = robot->desc.ndof;
    CPPF_REQUIRE((size_t)k * T * d <= 0x7fffffffu, "k*T*d exceeds 2^31-1");
    CPPF_REQUIRE((size_t)n_paths * T * d <= 0x7fffffffu, "n_paths*T*d exceeds 2^31-1");
    CPPF_ENTER(robot);
    hipStream_t st = (hipStream_t)stream;
    int32_t* const idxT = static_cast<int32_t*>(workspace);
    int32_t* const order = idxT + (size_t)T * k;
    int32_t* const alive = order + k;
    int32_t* const far = alive + k;
    int32_t* const sel = far + k;
    const size_t stage = dp_stage_bytes(k, T);
    // (the memo table staged in LDS by one workgroup of 1024 lanes where it fits, else walked in global memory, one lane per candidate)
    hipLaunchKernelGGL(dp_trace_all_kernel, dim3(stage ? 1u : (unsigned)((k + 255) / 256)), dim3(stage ? 1024 : 256), stage, st, memoT, k, T,
                       stage ? 1 : 0, idxT);
    const int rc = for_ndof(d, [&](auto dof) {
        hipLaunchKernelGGL((dp_nbest_select_kernel<decltype(dof)::D>), dim3(1), dim3(1024), 0, st, q, costsT, memoT, k, T, n_paths,
                           min_separation, robot->chain.pris_mask, prismatic_scaling, idxT, order, alive, far, sel, n_found);
        return CPPF_OK;
    });
    if (rc) return rc;
    const size_t total = (size_t)n_paths * T * d;
    hipLaunchKernelGGL(dp_nbest_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, q, costsT, k, T, d, n_paths, idxT,
                       sel, n_found, paths, path_idx, path_cost);
    return check_launch();
}

// ---- obstacle scenes (kernels_scene.h) --------------------------------------------------------------------------------------------
int cppf_scene_workspace_bytes(int n_rows, int n_obs, size_t* bytes) {
    CPPF_REQUIRE(bytes, "bytes is NULL");
    CPPF_REQUIRE(n_rows >= 0, "n_rows < 0");
    CPPF_REQUIRE(n_obs >= 0 && n_obs <= CPPF_MAX_SCENE_OBSTACLES, "n_obs out of range (0 .. CPPF_MAX_SCENE_OBSTACLES)");
    // one 64-bit key per row, one 32-bit key per cuboid (kernels_scene.h); never 0, so that "workspace is NULL" stays a refusal
    *bytes = up16((size_t)n_rows * sizeof(unsigned long long) + (size_t)n_obs * sizeof(uint32_t)) + 16;
    return CPPF_OK;
}

int cppf_scene_env_collisions(const cppf_robot* robot, const float* q, int S, int W, const float* box_lo, const float* box_hi, int n_obs,
                              float reach_m, uint8_t* env_mask, float* min_env, int32_t* nearest_obs, float* obs_min, void* workspace,
                              size_t workspace_bytes, void* stream) {
    const size_t n = (size_t)S * W;
    const auto shape = [&]() -> int {
        CPPF_REQUIRE(S >= 0 && W >= 0, "S / W < 0");
        CPPF_REQUIRE(n <= 0x7fffffffu, "S*W exceeds 2^31-1 rows");
        return CPPF_OK;
    };
    size_t lds = 0;
    if (int rc = check_scene_call(robot, shape, n_obs, reach_m, n == 0 || (q && env_mask), "q / env_mask is NULL", box_lo, box_hi, workspace,
                                  workspace_bytes, [&](size_t* bytes) { return cppf_scene_workspace_bytes((int)n, n_obs, bytes); },
                                  "workspace is smaller than cppf_scene_workspace_bytes(S*W, n_obs)", "scene", &lds))
        return rc;
    CPPF_ENTER(robot);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 && (n_obs == 0 || !obs_min)) return CPPF_OK;

    const bool want_min = min_env || nearest_obs || obs_min;
    SceneK sc;
    sc.cull = scene_cull_setup(robot, box_lo, box_hi, n_obs, want_min ? reach_m : 0.f);
    sc.row_key = static_cast<unsigned long long*>(workspace);
    uint32_t* const obs_key = reinterpret_cast<uint32_t*>(sc.row_key + n);
    sc.obs_key = obs_min ? obs_key : nullptr;
    sc.n = (int)n;
    const unsigned row_blocks = grid_for(n);
    const CuboidChunks cut = cut_cuboid_chunks(robot, row_blocks, n_obs);
    sc.chunk = cut.chunk;

    {
        // (a launch, not a memset node: a captured hipMemsetAsync of this odd byte count did not take effect on replay)
        const size_t words = 2 * n + (size_t)n_obs;
        hipLaunchKernelGGL(scene_init_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(workspace), words);
    }
    if (n > 0 && n_obs > 0) {
        const int rc = for_robot(robot, [&](auto tag) {
            using RB = typename decltype(tag)::type;
            return launch(want_min ? scene_kernel<RB, true> : scene_kernel<RB, false>, dim3(row_blocks, (unsigned)cut.n_chunks), dim3(kBlock), lds,
                          st, robot->chain, robot->coll, sc, q);
        });
        if (rc) return rc;
        if (int rc2 = check_launch()) return rc2;
    }
    const size_t items = std::max(n, obs_min ? (size_t)n_obs : (size_t)0);
    hipLaunchKernelGGL(scene_finish_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, sc.row_key, obs_key, (int)n, n_obs,
                       want_min ? 1 : 0, env_mask, min_env, nearest_obs, obs_min);
    return check_launch();
}

// ---- scenes from sensor data (kernels_voxel.h) ----------------------------------------------------------------------------------------
namespace {
// the workspace, every part a multiple of 16 bytes: bitset | row_heads | row_cells | row_offset | self segments
struct VoxelLayout {
    int wpr, rows;
    size_t bits, row, segs, total;  // bytes: the bitset, ONE per-row array, the segments, everything (+ 16: never 0)
};
// the grid's rules (cppflow_hip.h, "Grid" and "Planes"); fills *lay where given
int voxel_check_grid(const cppf_voxel_grid* grid, int n_self, VoxelLayout* lay) {
    CPPF_REQUIRE(grid, "grid is NULL");
    for (int k = 0; k < 3; ++k)
        CPPF_REQUIRE(grid->dims[k] >= 1 && grid->dims[k] <= CPPF_VOXEL_MAX_DIM, "grid dims out of range (1 .. CPPF_VOXEL_MAX_DIM each)");
    const int wpr = (grid->dims[0] + 63) / 64;
    const size_t rows = (size_t)grid->dims[1] * grid->dims[2];
    CPPF_REQUIRE((size_t)wpr * 64 * rows <= (size_t)CPPF_VOXEL_MAX_CELLS, "grid has too many cells (64 ceil(nx / 64) ny nz <= CPPF_VOXEL_MAX_CELLS)");
    CPPF_REQUIRE(n_self >= 0 && n_self <= CPPF_VOXEL_MAX_SELF, "n_self out of range (0 .. CPPF_VOXEL_MAX_SELF)");
    CPPF_REQUIRE(std::isfinite(grid->voxel_m) && grid->voxel_m > 0.f, "voxel_m must be positive and finite");
    for (int k = 0; k < 3; ++k) {
        float prev = 0.f;
        for (int i = 0; i <= grid->dims[k]; ++i) {
            // (volatile: two roundings whatever the host compiler would like to contract)
            volatile float step = (float)i * grid->voxel_m;
            volatile float plane = grid->origin[k] + step;
            const float pl = plane;
            CPPF_REQUIRE(std::isfinite(pl) && (i == 0 || pl > prev), "the grid's planes are not finite and strictly increasing in fp32");
            prev = pl;
        }
    }
    if (lay) {
        lay->wpr = wpr;
        lay->rows = (int)rows;
        lay->bits = up16(rows * wpr * sizeof(unsigned long long));
        lay->row = up16(rows * sizeof(int32_t));
        lay->segs = up16((size_t)n_self * CPPF_MAX_CAPSULES * 8 * sizeof(float));
        lay->total = lay->bits + 3 * lay->row + lay->segs + 16;
    }
    return CPPF_OK;
}

struct VoxelSource {
    const float* points;  // the point form, else NULL
    VoxelDepthK cam;      // the depth form
    size_t n;
};

// the source's own checks: the point form ...
int voxel_points_source(const float* points, int n_points, VoxelSource* src) {
    CPPF_REQUIRE(n_points >= 0, "n_points < 0");
    CPPF_REQUIRE(n_points == 0 || points, "points is NULL");
    src->points = points;
    src->n = (size_t)n_points;
    return CPPF_OK;
}
// ... and the depth form
int voxel_depth_source(const float* depth, int height, int width, const float intrinsics[4], const float cam_to_world[12], float z_min,
                       float z_max, VoxelSource* src) {
    CPPF_REQUIRE(height >= 0 && width >= 0, "height / width < 0");
    const size_t n = (size_t)height * (size_t)width;
    CPPF_REQUIRE(n < ((size_t)1 << 31), "height*width exceeds 2^31-1 pixels");
    CPPF_REQUIRE(n == 0 || depth, "depth is NULL");
    CPPF_REQUIRE(intrinsics && cam_to_world, "intrinsics / cam_to_world is NULL");
    CPPF_REQUIRE(z_min < z_max, "z_min must be below z_max (neither NaN)");
    src->cam.depth = depth;
    src->cam.width = width;
    src->cam.ifx = 1.0f / intrinsics[0], src->cam.ify = 1.0f / intrinsics[1];
    CPPF_REQUIRE(std::isfinite(intrinsics[0]) && std::isfinite(intrinsics[1]) && intrinsics[0] != 0.f && intrinsics[1] != 0.f &&
                     std::isfinite(src->cam.ifx) && std::isfinite(src->cam.ify),
                 "fx / fy must be finite and non-zero (and 1 / fx, 1 / fy finite)");
    src->cam.cx = intrinsics[2], src->cam.cy = intrinsics[3];
    for (int k = 0; k < 9; ++k) src->cam.R[k] = cam_to_world[k];
    for (int k = 0; k < 3; ++k) src->cam.t[k] = cam_to_world[9 + k];
    src->cam.z_min = z_min, src->cam.z_max = z_max;
    src->n = n;
    // (the point kernel tells the forms apart by its template argument; src->points stays NULL)
    return CPPF_OK;
}

// the refusals of everything that takes a frame in: the grid (fills *lay), the handle and q_self, the margin
int voxel_check_frame(const cppf_robot* robot, const cppf_voxel_grid* grid, const float* q_self, int n_self, float self_margin_m,
                      VoxelLayout* lay) {
    if (int rc = voxel_check_grid(grid, n_self, lay)) return rc;
    if (n_self > 0) {
        CPPF_REQUIRE(robot != nullptr, "robot handle is NULL (only n_self = 0 needs none)");
        CPPF_ROBOT_ALIVE(robot);
        CPPF_REQUIRE(q_self, "q_self is NULL");
    }
    CPPF_REQUIRE(self_margin_m >= 0.f && std::isfinite(self_margin_m), "self_margin_m must be finite and >= 0 (not NaN)");
    return CPPF_OK;
}
int voxel_check_boxes(int capacity, const float* box_lo, const float* box_hi) {
    CPPF_REQUIRE(capacity >= 0 && capacity <= CPPF_MAX_SCENE_OBSTACLES, "capacity out of range (0 .. CPPF_MAX_SCENE_OBSTACLES)");
    CPPF_REQUIRE(capacity == 0 || (box_lo && box_hi), "box_lo / box_hi is NULL");
    return CPPF_OK;
}
int voxel_check_scratch(const int32_t* counts, const void* workspace, size_t workspace_bytes, const VoxelLayout& lay) {
    CPPF_REQUIRE(counts, "counts is NULL");
    CPPF_REQUIRE(workspace, "workspace is NULL");
    CPPF_REQUIRE(((uintptr_t)workspace & 15u) == 0, "workspace must be 16-byte aligned");
    CPPF_REQUIRE(workspace_bytes >= lay.total, "workspace is smaller than cppf_voxel_scene_workspace_bytes(grid, n_self)");
    return CPPF_OK;
}
// the map of a grid: 16 bytes of header, then one uint8 per cell of the padded grid
size_t voxel_map_size(const VoxelLayout& lay) { return 16 + (size_t)lay.rows * lay.wpr * 64; }
int voxel_check_map(const void* map, size_t map_bytes, const VoxelLayout& lay) {
    CPPF_REQUIRE(map, "map is NULL");
    CPPF_REQUIRE(((uintptr_t)map & 15u) == 0, "map must be 16-byte aligned");
    CPPF_REQUIRE(map_bytes == voxel_map_size(lay), "map_bytes is not cppf_voxel_map_bytes(grid)");
    return CPPF_OK;
}

// (without a handle the launches go to the calling thread's current device, where the caller's pointers live)
int voxel_device(const cppf_robot* robot, int n_self, int* device) {
    if (n_self > 0)
        *device = robot->device;
    else
        CPPF_HIP(hipGetDevice(device));
    return CPPF_OK;
}

// the kernels' view of a grid and its workspace; *segs: where the self filter's segments go
VoxelK voxel_args(const cppf_robot* robot, const cppf_voxel_grid* grid, const VoxelLayout& lay, int n_self, int capacity, float* box_lo,
                  float* box_hi, int32_t* counts, void* workspace, float** segs) {
    char* const base = static_cast<char*>(workspace);
    VoxelK g;
    for (int k = 0; k < 3; ++k) g.origin[k] = grid->origin[k];
    g.voxel = grid->voxel_m;
    g.inv_voxel = 1.0f / grid->voxel_m;
    g.nx = grid->dims[0], g.ny = grid->dims[1], g.nz = grid->dims[2];
    g.wpr = lay.wpr, g.rows = lay.rows;
    g.bits = reinterpret_cast<unsigned long long*>(base);
    g.row_heads = reinterpret_cast<int32_t*>(base + lay.bits);
    g.row_cells = reinterpret_cast<int32_t*>(base + lay.bits + lay.row);
    g.row_offset = reinterpret_cast<int32_t*>(base + lay.bits + 2 * lay.row);
    *segs = reinterpret_cast<float*>(base + lay.bits + 3 * lay.row);
    g.segs = *segs;
    g.n_self = n_self;
    g.ncaps = n_self > 0 ? robot->coll.ncaps : 0;
    g.capacity = capacity;
    g.counts = counts;
    g.box_lo = box_lo, g.box_hi = box_hi;
    return g;
}

// a frame's occupancy into the workspace bitset: clear, the self filter's segments, the points
int voxel_launch_frame(const cppf_robot* robot, const VoxelSource& src, const VoxelK& g, const VoxelLayout& lay, const float* q_self,
                       float self_margin_m, float* segs, hipStream_t st) {
    const size_t n16 = (lay.bits + 3 * lay.row) / 16;
    hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)((std::max<size_t>(n16, 8) + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<uint4*>(g.bits), n16, g.counts);
    if (g.n_self > 0 && g.ncaps > 0) {
        VoxelSelfK sk;
        sk.q = q_self, sk.segs = segs, sk.n_self = g.n_self;
        for (int c = 0; c < CPPF_MAX_CAPSULES; ++c) {
            const double s = c < g.ncaps ? (double)robot->desc.cap_r[c] + (double)self_margin_m : 0.0;
            sk.thr2[c] = (float)(s * s);
        }
        // the generic capsule FK serves every robot: a generated table gives the same bits
        const int rc = for_dyn_robot(robot, [&](auto tag) {
            using RB = typename decltype(tag)::type;
            hipLaunchKernelGGL(voxel_self_kernel<RB>, dim3(1), dim3(64), 0, st, robot->chain, robot->coll, sk);
            return CPPF_OK;
        });
        if (rc) return rc;
    }
    if (src.n > 0) {
        const dim3 pgrid((unsigned)((src.n + 255) / 256));
        // (the depth form reads src.cam and is handed src.points = NULL)
        const auto points_kernel = src.points ? voxel_points_kernel<false> : voxel_points_kernel<true>;
        hipLaunchKernelGGL(points_kernel, pgrid, dim3(256), 0, st, g, src.points, src.cam, src.n);
    }
    return CPPF_OK;
}

// the bitset's box list: rows -> scan -> emit, merged along x and y or along z as well
void voxel_launch_boxes(const VoxelK& g, int merge, hipStream_t st) {
    const dim3 rgrid((unsigned)((g.rows + 255) / 256));
    hipLaunchKernelGGL(merge == CPPF_VOXEL_MERGE_XYZ ? voxel_rows_z_kernel : voxel_rows_kernel, rgrid, dim3(256), 0, st, g);
    hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(1024), 0, st, g);
    hipLaunchKernelGGL(merge == CPPF_VOXEL_MERGE_XYZ ? voxel_emit_z_kernel : voxel_emit_kernel, rgrid, dim3(256), 0, st, g);
}

// everything behind the source's own checks: the shared refusals, then the launches
int voxel_scene_run(const cppf_robot* robot, const VoxelSource& src, const cppf_voxel_grid* grid, const float* q_self, int n_self,
                    float self_margin_m, int capacity, float* box_lo, float* box_hi, int32_t* counts, void* workspace,
                    size_t workspace_bytes, void* stream) {
    VoxelLayout lay;
    if (int rc = voxel_check_frame(robot, grid, q_self, n_self, self_margin_m, &lay)) return rc;
    if (int rc = voxel_check_boxes(capacity, box_lo, box_hi)) return rc;
    if (int rc = voxel_check_scratch(counts, workspace, workspace_bytes, lay)) return rc;
    if (n_self > 0 && robot->desc.ndof < 3) return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: kernels are built for ndof in 3..12");

    int device = -1;
    if (int rc = voxel_device(robot, n_self, &device)) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess)
        return fail(CPPF_ERR_HIP, std::string("cppflow_hip: selecting the robot's device failed: ") + hipGetErrorString(guard.err));
    hipStream_t st = (hipStream_t)stream;
    float* segs = nullptr;
    const VoxelK g = voxel_args(robot, grid, lay, n_self, capacity, box_lo, box_hi, counts, workspace, &segs);
    if (int rc = voxel_launch_frame(robot, src, g, lay, q_self, self_margin_m, segs, st)) return rc;
    voxel_launch_boxes(g, CPPF_VOXEL_MERGE_XY, st);
    return check_launch();
}

// a frame into the map: the frame's bitset as voxel_scene_run builds it, then the integration
int voxel_map_add(const cppf_robot* robot, const VoxelSource& src, const cppf_voxel_grid* grid, const float* q_self, int n_self,
                  float self_margin_m, void* map, size_t map_bytes, int32_t* counts, void* workspace, size_t workspace_bytes,
                  void* stream) {
    VoxelLayout lay;
    if (int rc = voxel_check_frame(robot, grid, q_self, n_self, self_margin_m, &lay)) return rc;
    if (int rc = voxel_check_map(map, map_bytes, lay)) return rc;
    if (int rc = voxel_check_scratch(counts, workspace, workspace_bytes, lay)) return rc;
    if (n_self > 0 && robot->desc.ndof < 3) return fail(CPPF_ERR_UNSUPPORTED, "cppflow_hip: kernels are built for ndof in 3..12");

    int device = -1;
    if (int rc = voxel_device(robot, n_self, &device)) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess)
        return fail(CPPF_ERR_HIP, std::string("cppflow_hip: selecting the robot's device failed: ") + hipGetErrorString(guard.err));
    hipStream_t st = (hipStream_t)stream;
    float* segs = nullptr;
    const VoxelK g = voxel_args(robot, grid, lay, n_self, 0, nullptr, nullptr, counts, workspace, &segs);
    if (int rc = voxel_launch_frame(robot, src, g, lay, q_self, self_margin_m, segs, st)) return rc;
    VoxelMapK m;
    m.header = static_cast<int32_t*>(map);
    m.counters = reinterpret_cast<unsigned long long*>(static_cast<char*>(map) + 16);
    m.n_bytes = (size_t)lay.rows * lay.wpr * 8;
    hipLaunchKernelGGL(voxel_integrate_kernel, dim3((unsigned)((m.n_bytes + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const unsigned char*>(g.bits), m, counts);
    return check_launch();
}
}  // namespace

int cppf_voxel_scene_workspace_bytes(const cppf_voxel_grid* grid, int n_self, size_t* bytes) {
    CPPF_REQUIRE(bytes, "bytes is NULL");
    VoxelLayout lay;
    if (int rc = voxel_check_grid(grid, n_self, &lay)) return rc;
    *bytes = lay.total;
    return CPPF_OK;
}

int cppf_scene_from_points(const cppf_robot* robot, const float* points, int n_points, const cppf_voxel_grid* grid, const float* q_self,
                           int n_self, float self_margin_m, int capacity, float* box_lo, float* box_hi, int32_t* counts,
                           void* workspace, size_t workspace_bytes, void* stream) {
    VoxelSource src{};
    if (int rc = voxel_points_source(points, n_points, &src)) return rc;
    return voxel_scene_run(robot, src, grid, q_self, n_self, self_margin_m, capacity, box_lo, box_hi, counts, workspace, workspace_bytes,
                           stream);
}

int cppf_scene_from_depth(const cppf_robot* robot, const float* depth, int height, int width, const float intrinsics[4],
                          const float cam_to_world[12], float z_min, float z_max, const cppf_voxel_grid* grid, const float* q_self,
                          int n_self, float self_margin_m, int capacity, float* box_lo, float* box_hi, int32_t* counts,
                          void* workspace, size_t workspace_bytes, void* stream) {
    VoxelSource src{};
    if (int rc = voxel_depth_source(depth, height, width, intrinsics, cam_to_world, z_min, z_max, &src)) return rc;
    return voxel_scene_run(robot, src, grid, q_self, n_self, self_margin_m, capacity, box_lo, box_hi, counts, workspace, workspace_bytes,
                           stream);
}

// ---- scenes fused over frames (kernels_voxel.h) -----------------------------------------------------------------------------------------
int cppf_voxel_map_bytes(const cppf_voxel_grid* grid, size_t* bytes) {
    CPPF_REQUIRE(bytes, "bytes is NULL");
    VoxelLayout lay;
    if (int rc = voxel_check_grid(grid, 0, &lay)) return rc;
    *bytes = voxel_map_size(lay);
    return CPPF_OK;
}

int cppf_voxel_map_clear(void* map, size_t map_bytes, const cppf_voxel_grid* grid, void* stream) {
    VoxelLayout lay;
    if (int rc = voxel_check_grid(grid, 0, &lay)) return rc;
    if (int rc = voxel_check_map(map, map_bytes, lay)) return rc;
    const size_t n16 = map_bytes / 16;
    hipLaunchKernelGGL(voxel_map_clear_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<uint4*>(map), n16);
    return check_launch();
}

int cppf_voxel_map_add_points(const cppf_robot* robot, const float* points, int n_points, const cppf_voxel_grid* grid,
                              const float* q_self, int n_self, float self_margin_m, void* map, size_t map_bytes, int32_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream) {
    VoxelSource src{};
    if (int rc = voxel_points_source(points, n_points, &src)) return rc;
    return voxel_map_add(robot, src, grid, q_self, n_self, self_margin_m, map, map_bytes, counts, workspace, workspace_bytes, stream);
}

int cppf_voxel_map_add_depth(const cppf_robot* robot, const float* depth, int height, int width, const float intrinsics[4],
                             const float cam_to_world[12], float z_min, float z_max, const cppf_voxel_grid* grid, const float* q_self,
                             int n_self, float self_margin_m, void* map, size_t map_bytes, int32_t* counts, void* workspace,
                             size_t workspace_bytes, void* stream) {
    VoxelSource src{};
    if (int rc = voxel_depth_source(depth, height, width, intrinsics, cam_to_world, z_min, z_max, &src)) return rc;
    return voxel_map_add(robot, src, grid, q_self, n_self, self_margin_m, map, map_bytes, counts, workspace, workspace_bytes, stream);
}

int cppf_scene_from_map(const void* map, size_t map_bytes, const cppf_voxel_grid* grid, int min_frames, int merge, int capacity,
                        float* box_lo, float* box_hi, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    VoxelLayout lay;
    if (int rc = voxel_check_grid(grid, 0, &lay)) return rc;
    if (int rc = voxel_check_map(map, map_bytes, lay)) return rc;
    CPPF_REQUIRE(min_frames >= 1 && min_frames <= 255, "min_frames out of range (1 .. 255)");
    CPPF_REQUIRE(merge == CPPF_VOXEL_MERGE_XY || merge == CPPF_VOXEL_MERGE_XYZ, "merge is neither CPPF_VOXEL_MERGE_XY nor CPPF_VOXEL_MERGE_XYZ");
    if (int rc = voxel_check_boxes(capacity, box_lo, box_hi)) return rc;
    if (int rc = voxel_check_scratch(counts, workspace, workspace_bytes, lay)) return rc;

    // (no handle: the launches go to the calling thread's current device, where the caller's pointers live)
    hipStream_t st = (hipStream_t)stream;
    float* segs = nullptr;
    const VoxelK g = voxel_args(nullptr, grid, lay, 0, capacity, box_lo, box_hi, counts, workspace, &segs);
    // the threshold pass stores every word of the bitset: what is left to clear are the per-row arrays and counts
    const size_t n16 = 3 * lay.row / 16;
    hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)((std::max<size_t>(n16, 8) + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<uint4*>(g.row_heads), n16, counts);
    const size_t n_words = (size_t)lay.rows * lay.wpr;
    hipLaunchKernelGGL(voxel_threshold_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, g,
                       reinterpret_cast<const uint4*>(static_cast<const char*>(map) + 16), static_cast<const int32_t*>(map), min_frames);
    voxel_launch_boxes(g, merge, st);
    return check_launch();
}

// ---- motion between the waypoints (kernels_motion.h) ------------------------------------------------------------------------------
int cppf_motion_rho(const cppf_robot* robot, float* rho) {
    CPPF_ROBOT_ALIVE(robot);
    CPPF_REQUIRE(rho, "rho is NULL");
    std::memcpy(rho, robot->rho, sizeof(robot->rho));
    return CPPF_OK;
}

int cppf_motion_workspace_bytes(int S, int W, size_t* bytes) {
    CPPF_REQUIRE(bytes, "bytes is NULL");
    CPPF_REQUIRE(S >= 0, "S < 0");
    CPPF_REQUIRE(W >= 2, "W < 2: a motion needs two waypoints");
    // three 32-bit words per transition (kernels_motion.h); never 0, so that "workspace is NULL" stays a refusal
    *bytes = up16((size_t)S * (size_t)(W - 1) * 3 * sizeof(uint32_t)) + 16;
    return CPPF_OK;
}

int cppf_motion_clearance(const cppf_robot* robot, const float* q, int S, int W, int level, const float* box_lo, const float* box_hi,
                          int n_obs, float reach_m, uint8_t* status, float* min_clear, int32_t* hit_node, float* nodes, void* workspace,
                          size_t workspace_bytes, void* stream) {
    size_t n_nodes = 0;  // per path
    const auto shape = [&]() -> int {
        CPPF_REQUIRE(S >= 0, "S < 0");
        CPPF_REQUIRE(W >= 2, "W < 2: a motion needs two waypoints");
        CPPF_REQUIRE(level >= 0 && level <= CPPF_MOTION_MAX_LEVEL, "level out of range (0 .. CPPF_MOTION_MAX_LEVEL)");
        n_nodes = ((size_t)(W - 1) << level) + 1;
        CPPF_REQUIRE((size_t)S * (n_nodes + 64) <= 0x7fffffffu, "S * ((W-1) * 2^level + 1) exceeds 2^31-1 nodes");
        return CPPF_OK;
    };
    size_t lds = 0;
    if (int rc = check_scene_call(robot, shape, n_obs, reach_m, S == 0 || (q && status), "q / status is NULL", box_lo, box_hi, workspace,
                                  workspace_bytes, [&](size_t* bytes) { return cppf_motion_workspace_bytes(S, W, bytes); },
                                  "workspace is smaller than cppf_motion_workspace_bytes(S, W)", "motion", &lds))
        return rc;
    CPPF_ENTER(robot);
    hipStream_t st = (hipStream_t)stream;
    if (S == 0) return CPPF_OK;
    CPPF_REQUIRE(robot->d_quad != nullptr, "the handle has no device tables");

    const size_t n_tr = (size_t)S * (size_t)(W - 1);
    MotionK mk;
    mk.cull = scene_cull_setup(robot, box_lo, box_hi, n_obs, reach_m);
    mk.rho = reinterpret_cast<const float*>(static_cast<const uint4*>(robot->d_quad) + kQuadTableRecs);
    mk.fail = static_cast<uint32_t*>(workspace);
    mk.clear_key = mk.fail + n_tr;
    mk.hit = reinterpret_cast<int32_t*>(mk.clear_key + n_tr);
    mk.nodes = nodes;
    mk.S = S, mk.W = W, mk.level = level;
    mk.n_nodes = (int)n_nodes;
    mk.waves_per_path = (int)((n_nodes - 1 + 62) / 63);
    mk.inv_m = 1.f / (float)(1 << level);
    const size_t waves = (size_t)S * (size_t)mk.waves_per_path;
    const unsigned wave_blocks = (unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64));
    const CuboidChunks cut = cut_cuboid_chunks(robot, wave_blocks, n_obs);
    mk.chunk = cut.chunk;

    const unsigned tr_blocks = (unsigned)((n_tr + 255) / 256);
    hipLaunchKernelGGL(motion_init_kernel, dim3(tr_blocks), dim3(256), 0, st, mk.fail, mk.clear_key, mk.hit, n_tr);
    const int rc = for_robot(robot, [&](auto tag) {
        using RB = typename decltype(tag)::type;
        return launch(motion_kernel<RB>, dim3(wave_blocks, (unsigned)cut.n_chunks), dim3(kBlock), lds, st, robot->chain, robot->coll, mk, q);
    });
    if (rc) return rc;
    if (int rc2 = check_launch()) return rc2;
    hipLaunchKernelGGL(motion_finish_kernel, dim3(tr_blocks), dim3(256), 0, st, mk.fail, mk.clear_key, mk.hit, n_tr, status, min_clear,
                       hit_node);
    return check_launch();
}

// ---- adaptive bisection of the same test (kernels_motion_resolve.h) -----------------------------------------------------------------
int cppf_motion_resolve_workspace_bytes(int S, int W, int max_frontier, size_t* bytes) {
    CPPF_REQUIRE(bytes, "bytes is NULL");
    CPPF_REQUIRE(S >= 0, "S < 0");
    CPPF_REQUIRE(W >= 2, "W < 2: a motion needs two waypoints");
    CPPF_REQUIRE(max_frontier >= 1 && max_frontier <= CPPF_MOTION_RESOLVE_MAX_FRONTIER,
                 "max_frontier out of range (1 .. CPPF_MOTION_RESOLVE_MAX_FRONTIER)");
    // two lists of max_frontier 32-bit interval indices per transition; never 0, so that "workspace is NULL" stays a refusal
    *bytes = up16((size_t)S * (size_t)(W - 1) * 2 * (size_t)max_frontier * sizeof(uint32_t)) + 16;
    return CPPF_OK;
}

int cppf_motion_resolve(const cppf_robot* robot, const float* q, int S, int W, int start_level, int max_depth, int max_frontier,
                        const float* box_lo, const float* box_hi, int n_obs, float reach_m, const uint8_t* decided, uint8_t* status,
                        int32_t* depth, int32_t* hit_num, float* min_clear, int32_t* n_tested, void* workspace, size_t workspace_bytes,
                        void* stream) {
    const auto shape = [&]() -> int {
        CPPF_REQUIRE(S >= 0, "S < 0");
        CPPF_REQUIRE(W >= 2, "W < 2: a motion needs two waypoints");
        CPPF_REQUIRE(start_level >= 0 && start_level <= CPPF_MOTION_MAX_LEVEL, "start_level out of range (0 .. CPPF_MOTION_MAX_LEVEL)");
        CPPF_REQUIRE(max_depth >= start_level && max_depth <= CPPF_MOTION_RESOLVE_MAX_DEPTH,
                     "max_depth out of range (start_level .. CPPF_MOTION_RESOLVE_MAX_DEPTH)");
        CPPF_REQUIRE(max_frontier >= (1 << start_level) && max_frontier <= CPPF_MOTION_RESOLVE_MAX_FRONTIER,
                     "max_frontier out of range (2^start_level .. CPPF_MOTION_RESOLVE_MAX_FRONTIER)");
        CPPF_REQUIRE((size_t)S * (size_t)(W - 1) <= 0x7fffffffu, "S * (W-1) exceeds 2^31-1 transitions");
        return CPPF_OK;
    };
    size_t lds = 0;
    if (int rc = check_scene_call(robot, shape, n_obs, reach_m, S == 0 || (q && status), "q / status is NULL", box_lo, box_hi, workspace,
                                  workspace_bytes,
                                  [&](size_t* bytes) { return cppf_motion_resolve_workspace_bytes(S, W, max_frontier, bytes); },
                                  "workspace is smaller than cppf_motion_resolve_workspace_bytes(S, W, max_frontier)", "motion", &lds))
        return rc;
    CPPF_ENTER(robot);
    hipStream_t st = (hipStream_t)stream;
    if (S == 0) return CPPF_OK;
    CPPF_REQUIRE(robot->d_quad != nullptr, "the handle has no device tables");

    const size_t n_tr = (size_t)S * (size_t)(W - 1);
    ResolveK rk;
    rk.cull = scene_cull_setup(robot, box_lo, box_hi, n_obs, reach_m);
    rk.rho = reinterpret_cast<const float*>(static_cast<const uint4*>(robot->d_quad) + kQuadTableRecs);
    rk.decided = decided;
    rk.status = status;
    rk.depth = depth;
    rk.hit_num = hit_num;
    rk.min_clear = min_clear;
    rk.n_tested = n_tested;
    rk.frontier = static_cast<uint32_t*>(workspace);
    rk.S = S, rk.W = W, rk.start_level = start_level, rk.max_depth = max_depth, rk.max_frontier = max_frontier;
    const unsigned blocks = (unsigned)((n_tr + kBlock / 64 - 1) / (kBlock / 64));  // one wavefront per transition
    const int rc = for_robot(robot, [&](auto tag) {
        using RB = typename decltype(tag)::type;
        return launch(motion_resolve_kernel<RB>, dim3(blocks), dim3(kBlock), lds, st, robot->chain, robot->coll, rk, q);
    });
    if (rc) return rc;
    return check_launch();
}

// ---- RCCL behind the C ABI ------------------------------------------------------------------------------------------------------
// Declared here instead of including <rccl/rccl.h>: the library is loaded with dlopen so that libcppflow_hip.so has no link-time
// dependency on it (a process that already holds PyTorch's copy must not get a second one).
namespace {
struct RcclUid {
    char bytes[CPPF_COMM_ID_BYTES];
};
typedef void* RcclComm;
struct RcclApi {
    void* handle = nullptr;
    int (*GetUniqueId)(RcclUid*) = nullptr;
    int (*CommInitRank)(RcclComm*, int, RcclUid, int) = nullptr;
    int (*CommInitAll)(RcclComm*, int, const int*) = nullptr;
    int (*CommDestroy)(RcclComm) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, RcclComm, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;      // (the communicator's side of the library: the one piece of process-wide state)
std::mutex g_rccl_mu;  // two threads may create their communicators at the same time

int load_rccl() {
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    if (g_rccl.handle) return CPPF_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) {
        h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) return fail(CPPF_ERR_UNSUPPORTED, std::string("cppflow_hip: cannot load RCCL (librccl.so.1): ") + dlerror());
    RcclApi api;
    api.handle = h;
#define CPPF_SYM(field, name)                                                                        \
    api.field = reinterpret_cast<decltype(api.field)>(dlsym(h, name));                               \
    if (!api.field) return fail(CPPF_ERR_UNSUPPORTED, std::string("cppflow_hip: RCCL lacks ") + name)
    CPPF_SYM(GetUniqueId, "ncclGetUniqueId");
    CPPF_SYM(CommInitRank, "ncclCommInitRank");
    CPPF_SYM(CommInitAll, "ncclCommInitAll");
    CPPF_SYM(CommDestroy, "ncclCommDestroy");
    CPPF_SYM(AllGather, "ncclAllGather");
    CPPF_SYM(GroupStart, "ncclGroupStart");
    CPPF_SYM(GroupEnd, "ncclGroupEnd");
    CPPF_SYM(GetErrorString, "ncclGetErrorString");
#undef CPPF_SYM
    g_rccl = api;
    return CPPF_OK;
}

#define CPPF_RCCL(call)                                                                                          \
    do {                                                                                                         \
        int r__ = (call);                                                                                        \
        if (r__ != 0)                                                                                            \
            return fail(CPPF_ERR_HIP, std::string("cppflow_hip: " #call " failed: ") + g_rccl.GetErrorString(r__)); \
    } while (0)
}  // namespace

struct cppf_comm {
    RcclComm comm;
    int rank, world, device;
};

int cppf_comm_available(void) { return load_rccl(); }

int cppf_comm_unique_id(void* id_out) {
    CPPF_REQUIRE(id_out, "id_out is NULL");
    if (int rc = load_rccl()) return rc;
    RcclUid id;
    CPPF_RCCL(g_rccl.GetUniqueId(&id));
    std::memcpy(id_out, id.bytes, CPPF_COMM_ID_BYTES);
    return CPPF_OK;
}

int cppf_comm_init_rank(const void* id, int rank, int world, int device, cppf_comm** out) {
    CPPF_REQUIRE(id && out, "id / out is NULL");
    CPPF_REQUIRE(world >= 1 && rank >= 0 && rank < world, "rank / world out of range");
    *out = nullptr;
    if (int rc = load_rccl()) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail(CPPF_ERR_HIP, std::string("cppflow_hip: selecting the device failed: ") + hipGetErrorString(guard.err));
    RcclUid uid;
    std::memcpy(uid.bytes, id, CPPF_COMM_ID_BYTES);
    RcclComm c = nullptr;
    CPPF_RCCL(g_rccl.CommInitRank(&c, world, uid, rank));
    *out = new cppf_comm{c, rank, world, device};
    return CPPF_OK;
}

int cppf_comm_init_all(int n_devices, const int* devices, cppf_comm** out) {
    CPPF_REQUIRE(n_devices >= 1 && devices && out, "n_devices < 1 or NULL pointer");
    if (int rc = load_rccl()) return rc;
    std::vector<RcclComm> comms((size_t)n_devices, nullptr);
    CPPF_RCCL(g_rccl.CommInitAll(comms.data(), n_devices, devices));
    for (int i = 0; i < n_devices; ++i) out[i] = new cppf_comm{comms[(size_t)i], i, n_devices, devices[i]};
    return CPPF_OK;
}

int cppf_comm_rank(const cppf_comm* comm) { return comm ? comm->rank : CPPF_ERR_INVALID; }

int cppf_comm_world(const cppf_comm* comm) { return comm ? comm->world : CPPF_ERR_INVALID; }

int cppf_allgather_bytes(cppf_comm* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream) {
    CPPF_REQUIRE(comm, "comm is NULL");
    if (bytes_per_rank == 0) return CPPF_OK;
    CPPF_REQUIRE(send && recv, "send / recv is NULL");
    DeviceGuard guard(comm->device);
    if (guard.err != hipSuccess) return fail(CPPF_ERR_HIP, std::string("cppflow_hip: selecting the device failed: ") + hipGetErrorString(guard.err));
    CPPF_RCCL(g_rccl.AllGather(send, recv, bytes_per_rank, /* ncclUint8 */ 1, comm->comm, (hipStream_t)stream));
    return CPPF_OK;
}

int cppf_comm_group_begin(void) {
    if (int rc = load_rccl()) return rc;
    CPPF_RCCL(g_rccl.GroupStart());
    return CPPF_OK;
}

int cppf_comm_group_end(void) {
    if (int rc = load_rccl()) return rc;
    CPPF_RCCL(g_rccl.GroupEnd());
    return CPPF_OK;
}

void cppf_comm_destroy(cppf_comm* comm) {
    if (!comm) return;
    if (g_rccl.handle && comm->comm) (void)g_rccl.CommDestroy(comm->comm);
    delete comm;
}

}  // extern "C"
