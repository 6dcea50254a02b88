/*
 * cppflow_hip.h -- C ABI of libcppflow_hip.so: the MI355X (gfx950) implementation of jstmn/cppflow's batched LM-IK
 * refinement hot path (pose-only Levenberg-Marquardt step + batched self / environment collision masks).
 *
 * The reference has no FFI for this path (it is pure Python over torch + the un-vendored `jrl` package); the drop-in
 * boundary is therefore a set of Python call signatures, mirrored by the modules of cppflow_amd/, each of which lands on exactly
 * one entry point below.  Every entry point cites the reference interface it replaces (paths under /root/reference).
 *
 * Conventions
 *   - plain C, no torch types; all `x`, `target`, output pointers are DEVICE pointers to contiguous row-major fp32
 *     (masks: uint8) on the robot's device; robot / obstacle descriptions are HOST pointers, copied at call time.
 *   - the library never allocates or frees caller buffers; every launch is asynchronous on `stream` (a hipStream_t
 *     passed as void*, NULL = the default stream); no host synchronisation inside any compute entry point.
 *   - rows are (seed, waypoint) pairs: row r = s * W + w; `target` is [W, 7] and is indexed by r % W, which replaces the
 *     reference's `torch.vstack([target_path] * parallel_count)` (cppflow/optimization.py:399-401).  Pass W = n for an
 *     already-stacked [n, 7] target.
 *   - return value 0 on success; CPPF_ERR_INVALID (contract / shape violation -> the Python shim raises AssertionError,
 *     mirroring the reference's asserts), CPPF_ERR_HIP (runtime failure -> RuntimeError), CPPF_ERR_UNSUPPORTED.
 *     cppf_last_error() returns a thread-local message for the last failure.
 *
 * Ownership and lifetimes (the caller owns all tensors)
 *   - caller buffers: never allocated, freed or retained by the library beyond the launches that were handed them -- except by a
 *     cppf_lm_batch, which records its items' pointers: they must stay valid while the batch is launched.
 *   - cppf_robot: created / destroyed by the caller.  A cppf_lm_batch is bound to the robot it was created from and keeps that
 *     handle ALLOCATED: cppf_robot_destroy on a robot with live batches marks it destroyed and returns; from then on every entry
 *     point given the handle or one of its batches (cppf_lm_batch_launch included) returns CPPF_ERR_INVALID without launching
 *     anything, and the memory is released by the cppf_lm_batch_destroy of its last batch.  So "robot first, then its batches" is
 *     a legal order of destruction; using a robot handle after cppf_robot_destroy when it has NO live batch is a use after free,
 *     as for any C handle.  cppf_lm_batch_destroy needs nothing but the batch.
 *   - cppf_comm: independent of robots and batches.
 *   - one host thread per handle at a time; handles on different threads are independent (no process-wide mutable state besides
 *     the RCCL function table).
 */
#ifndef CPPFLOW_HIP_H
#define CPPFLOW_HIP_H

#ifndef __HIPCC_RTC__
#include <stddef.h>
#include <stdint.h>
#else /* hipRTC (cppf_robot_specialize compiles this header too) has no <stdint.h>: the compiler's own fixed-width types */
typedef __INT8_TYPE__ int8_t;
typedef __UINT8_TYPE__ uint8_t;
typedef __INT32_TYPE__ int32_t;
typedef __UINT32_TYPE__ uint32_t;
typedef __UINT64_TYPE__ uint64_t;
typedef __SIZE_TYPE__ size_t;
typedef __UINTPTR_TYPE__ uintptr_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define CPPF_ABI_VERSION 6

#define CPPF_MAX_DOF 12 /* every ndof in 3..12 is built (the reference's robots have 7 and 8) */
#define CPPF_MAX_CAPSULES 24
#define CPPF_MAX_PAIRS 128
#define CPPF_MAX_OBSTACLES 8
#define CPPF_MAX_BATCH 16 /* independent problems one batched fused launch can carry (cppf_lm_batch_create) */

#define CPPF_OK 0
#define CPPF_ERR_INVALID (-1)
#define CPPF_ERR_HIP (-2)
#define CPPF_ERR_UNSUPPORTED (-3)

#define CPPF_JOINT_REVOLUTE 0
#define CPPF_JOINT_PRISMATIC 1

/* Canonical serial chain (cppflow_amd/robot_model.py): world_T_link_j = prod_{i<=j} F_i * M_z(q_i), ee = link_{d-1} * F_ee.
 * Stands in for the `jrl.robot.Robot` object the reference passes around (cppflow/data_types.py:383). */
typedef struct cppf_robot_desc {
    int32_t ndof;
    float F[CPPF_MAX_DOF][12]; /* per joint: rotation row-major (9) then translation (3) */
    float F_ee[12];
    int32_t jtype[CPPF_MAX_DOF]; /* CPPF_JOINT_* : motion about / along the local z axis */
    float lo[CPPF_MAX_DOF];     /* robot.actuated_joints_limits (cppflow/optimization_utils.py:825-832) */
    float hi[CPPF_MAX_DOF];
    int32_t n_capsules;
    int32_t cap_link[CPPF_MAX_CAPSULES]; /* moving link the capsule rides on, -1 = base; must be non-decreasing */
    float cap_p0[CPPF_MAX_CAPSULES][3]; /* axis end points in the link frame; p0 == p1 exactly makes the capsule a sphere */
    float cap_p1[CPPF_MAX_CAPSULES][3]; /* |p1 - p0| = 0 (sphere) or > 1e-6 */
    float cap_r[CPPF_MAX_CAPSULES];
    int32_t n_pairs;
    int32_t pairs[CPPF_MAX_PAIRS][2]; /* capsule index pairs checked by self_collision_distances */
} cppf_robot_desc;

/* cppflow/lm_hyper_parameters.py:14-81 (fields the pose-only step reads) + fused-loop controls */
typedef struct cppf_lm_params {
    float lm_lambda;      /* OptimizationParameters.lm_lambda      (ALT_LOSS_V2_1_POSE: 1e-6, :123) */
    float alpha_position; /* OptimizationParameters.alpha_position (3.5,  :125) */
    float alpha_rotation; /* OptimizationParameters.alpha_rotation (0.35, :126) */
    int32_t n_steps;      /* K >= 1 fused { step ; clamp } iterations (cppflow/optimization.py:258-259 per iteration).  The LAST
                           * iteration of a launch -- the one that produces x_out -- is evaluated in the canonical arithmetic (the
                           * sine / cosine the bit-exact FK uses); the K - 1 iterations before it, whose iterates are not outputs,
                           * use cheaper elementary functions in the row shape: for the residual's roll / pitch / yaw shorter polynomials
                           * behind ONE shared reciprocal (4e-7 absolute), the 6x6 solve as a block L D L^T with 2x2 pivots (three
                           * reciprocals for six reciprocal square roots; 1.2 - 1.8x the Cholesky form's fp32 rounding error), and a
                           * cheaper sine / cosine (polynomials on [-pi, pi], 5e-7 absolute; the first
                           * iteration behind a reduction by whole turns -- the input need not lie inside the joint limits --
                           * the others directly: their iterates have been through the clamp).  A K = 1 launch (the reference's
                           * cadence) and every iteration of an early-out launch are canonical throughout.
                           * What K fused steps are worth against K steps of the reference (cppflow/optimization.py:61-92, 258-259),
                           * measured at K = 2, 3, 5 against the fp64 reference-order oracle on the four shipped robots and on the C4
                           * planner inputs (tests/test_gpu_lean_parity.py, profiles/r5_lean_parity.txt), in the scaled task space of
                           * the residual, ts = |J_s (x_K - x_K^oracle)|: median 2e-7, 90th percentile <= 1.5e-6 (the reference's own
                           * fp32 arithmetic: median 8e-6 .. 2e-4), and ROW BY ROW
                           *     ts <= K * eps * (1 + 2 |largest step| / sigma_min(J_s)),  eps = 1e-4 (CPPF_SOLVER_AUTO), 2e-5 (CPPF_SOLVER_F64)
                           * -- K per-step errors of the K = 1 bar grown by the row's own conditioning; pose error after K steps within
                           * 1e-5 + 2 K |step| |dx| of the oracle's.  The polynomials and the relative gate by themselves (K launches of
                           * one step against one launch of K): median 2.5e-7, 90th percentile <= 1.6e-6. */
    int32_t clamp;        /* 1: clamp_to_joint_limits after every step (the reference loop); 0: bare step (K must be 1) */
    /* Early-out (0 = off): a row whose residual at the start of an iteration has ||t_target - t|| < tol_pos_m and
     * ||(roll, pitch, yaw)|| < tol_rot_rad is left untouched from then on, and a wavefront whose rows are all below
     * tolerance leaves the loop -- the in-launch counterpart of the reference loop stopping once the pose is valid
     * (cppflow/optimization.py:251-258, 326-358).  Not combinable with J_out / e_out. */
    float tol_pos_m;
    float tol_rot_rad;
    /* Kernel shape: CPPF_SHAPE_AUTO picks by batch size; CPPF_SHAPE_ROW = one (seed, waypoint) row per lane (throughput
     * shape); CPPF_SHAPE_QUAD = four lanes cooperate on one row (latency shape for batches that cannot fill the chip). */
    int32_t shape;
    /* Precision of the damped solve (ndof >= 6; below that the primal fp32 solve).
     *   CPPF_SOLVER_AUTO (0, the default): the reference's dtype, conditioning-gated -- every row is solved in fp32; a row whose
     *     a-posteriori error estimate  eps * a_max * max diag(A) * max |y|  (the task-space size of the rounding error of forming
     *     and factoring A = J J^T + lambda S^-2, known once y = A^-1 e is) exceeds `solver_gate` redoes the solve in double
     *     precision.  The step is then never farther from the exactly solved one than the reference's own fp32 arithmetic
     *     (torch.linalg.solve on the primal system, cppflow/optimization.py:85-88) gets -- near-singular rows included.
     *     Two exceptions, both inside a clamped launch (clamp = 1): a flagged row whose fp32 step leaves the joint limits keeps the
     *     fp32 step -- where it lands is decided by the clamp, not by the last digits of the solve; and in the K - 1 iterations in
     *     front of the LAST one (whose iterates are intermediates; both kernel shapes) a flagged row is re-solved only when the estimate also
     *     exceeds a thousandth of the residual norm the step reduces -- an intermediate step has to be accurate relative to its
     *     residual; the last iteration, a K = 1 launch and every iteration of an early-out launch keep the absolute bar.  Measured
     *     (tests/test_gpu_lean_parity.py): the relative gate declines the re-solve on 0.3 % of a planner's rows (7 - 15 % of independent
     *     random 7-joint configurations) and moves the K-step iterate by <= K (1e-3 |e_s| + 1e-4) (1 + 2 |step| / sigma_min) in scaled
     *     task space; a row that is never flagged is not moved at all.
     *   CPPF_SOLVER_F64: every row in double precision (J J^T, its factorisation, the substitutions and J^T y): the exactly
     *     solved step of the fp32 Jacobian on every row, clamped or not (task-space difference to the fp64 oracle <= 6e-7).  A verification mode: every
     *     wavefront runs eight re-solve rounds per iteration (~10x the iteration time).
     *   CPPF_SOLVER_F32: fp32 only, no gate (the round-2 behaviour; up to 6e-2 off in task space on near-singular rows). */
    int32_t solver;
    /* Tolerance of CPPF_SOLVER_AUTO's gate in the scaled task-space units of the residual (rad * alpha_rotation, m *
     * alpha_position); 0 = CPPF_SOLVER_GATE_DEFAULT. */
    float solver_gate;
} cppf_lm_params;

#define CPPF_SOLVER_AUTO 0
#define CPPF_SOLVER_F64 1
#define CPPF_SOLVER_F32 2
#define CPPF_SOLVER_GATE_DEFAULT 1e-5f

#define CPPF_SHAPE_AUTO 0
#define CPPF_SHAPE_ROW 1
#define CPPF_SHAPE_QUAD 2

/* Optional outputs of the fused launch; any pointer may be NULL. */
typedef struct cppf_lm_outputs {
    float* x_out;         /* [n, d]    x after K steps (may alias x_in) */
    float* J_out;         /* [n, 6, d] SCALED Jacobian at the last linearisation point (optimization.py:77-80, 90-92) */
    float* e_out;         /* [n, 6]    SCALED pose error there, rows [roll pitch yaw x y z] (optimization_utils.py:806) */
    float* pos_err_m;     /* [n]  ||t_target - t(x_out)||_2            (evaluation_utils.py:134-136) */
    float* rot_err_rad;   /* [n]  geodesic quaternion distance at x_out (evaluation_utils.py:139-141) */
    uint8_t* self_mask;   /* [n]  min self distance < 0 at x_out        (collision_detection.py:52-69) */
    uint8_t* env_mask;    /* [n]  OR over obstacles of min dist < 0     (collision_detection.py:27-49) */
    uint8_t* jlim_mask;   /* [n]  joint within padding of a limit       (search.py:25-52) */
    float* ext_cost;      /* [n]  100*jlim + 1000*env + 1000*self        (search.py:14-15, 146-150) */
    float* min_self;      /* [n]  min over pairs of the signed distance (+inf when no pairs) */
    float* min_env;       /* [n]  min over obstacles and capsules       (+inf when no obstacles) */
    float* seed_summary;  /* [S,8] the reduction of cppf_seed_summary over each seed's W rows, produced by the same launch
                           * when W is 64, 128 or 256 (a 256-row workgroup then holds whole seeds); for any other W the entry point runs the
                           * separate reduction kernel afterwards, which needs x_out, pos_err_m, rot_err_rad, the three masks
                           * and ext_cost to be non-NULL.  Implies the collision stage. */
    int32_t* n_iters;     /* [n]  LM steps actually applied to the row (< n_steps only with the early-out tolerances) */
} cppf_lm_outputs;

typedef struct cppf_robot cppf_robot; /* opaque: host copy of the description + launch state for one device */

int cppf_abi_version(void);
/* sha256 prefix of the sources this binary was compiled from (cppflow_amd/build.py:source_hash); the Python binding refuses a
 * library whose id differs from the sources next to it. */
const char* cppf_build_id(void);
const char* cppf_last_error(void);

/* Replaces jrl.robots.get_robot(name) (cppflow/data_type_utils.py:197): validates and binds a description to `device`. */
int cppf_robot_create(const cppf_robot_desc* desc, int device, cppf_robot** out);
void cppf_robot_destroy(cppf_robot* robot);
int cppf_robot_ndof(const cppf_robot* robot);
/* >= 0: index of the robot-specialised kernel set (generated tables, csrc/robots_gen.h) this handle runs; -1: the generic
 * kernels, driven by the description in the kernel-argument segment. */
int cppf_robot_specialization(const cppf_robot* robot);
/* Compile-time tables for a description that matches none of the generated ones (any real robot a caller brings): the fused,
 * collision and quad kernels are compiled for THIS robot with hipRTC -- chain constants become literals, capsule end points
 * stay in registers, exactly as for the shipped robots -- and cached on disk under `cache_dir` (NULL: $CPPF_CACHE_DIR, else
 * $HOME/.cache/cppflow_amd) keyed by a hash of the description and of the kernel sources, so that later processes load the code
 * object without compiling.  Results are bit-identical to the generic kernels.  (The generic fused kernel stages capsule end
 * points in LDS, 6 KB per capsule: at 12 joints x 24 capsules that no longer fits a compute unit and the fused launch with
 * collision outputs returns CPPF_ERR_UNSUPPORTED -- such a robot must be specialised.)  After success cppf_robot_specialization()
 * returns CPPF_SPECIALIZATION_RTC.  Stands in for jrl.robots.get_robot returning a robot class with baked-in kinematics
 * (cppflow/data_type_utils.py:197).  A no-op (CPPF_OK) for a handle that already runs a generated table. */
#define CPPF_SPECIALIZATION_RTC 1000
int cppf_robot_specialize(cppf_robot* robot, const char* cache_dir);
/* (Test and tuning hooks live in cppflow_hip_debug.h; none of them is process-wide.) */

/* Replaces Problem.obstacles_cuboids / obstacles_Tcuboids (cppflow/data_type_utils.py:87-145).
 * cuboids [O,6] = (-sx/2,-sy/2,-sz/2, sx/2,sy/2,sz/2); Rt [O,12] = rotation row-major (9) then translation (3), HOST
 * pointers.  Only axis-aligned cuboids are accepted (R = I), as the reference asserts at data_type_utils.py:108. */
int cppf_set_obstacles(cppf_robot* robot, int n_obs, const float* cuboids, const float* Rt);

/* Padded joint limits l + eps / u - eps of joint_limit_almost_violations_3d (cppflow/search.py:46-51), HOST [d] each. */
int cppf_set_joint_limit_padding(cppf_robot* robot, const float* lo_padded, const float* hi_padded);

/* Robot.forward_kinematics(x) -> [n,7] = [x y z qw qx qy qz] (call sites cppflow/optimization_utils.py:811,
 * cppflow/evaluation_utils.py:115) */
int cppf_forward_kinematics(const cppf_robot* robot, const float* x, int n, float* poses, void* stream);

/* Robot.jacobian(x) -> [n,6,d], rows 0:3 angular, 3:6 linear, world frame (call site cppflow/optimization.py:74) */
int cppf_jacobian(const cppf_robot* robot, const float* x, int n, float* J, void* stream);

/* get_6d_pose_errors(robot, x, target_poses) -> (e [n,6], current_poses [n,7]); cppflow/optimization_utils.py:802-820 */
int cppf_pose_errors(const cppf_robot* robot, const float* x, const float* target, int S, int W, float* e,
                     float* current_poses, void* stream);

/* clamp_to_joint_limits(robot, x): in place; cppflow/optimization_utils.py:823-833 */
int cppf_clamp_to_joint_limits(const cppf_robot* robot, float* x, int n, void* stream);

/* levenberg_marquardt_only_pose (cppflow/optimization.py:61-92) followed by clamp_to_joint_limits (:259), K times in one
 * launch, with the pose-error metrics of x_is_valid (cppflow/optimization_utils.py:847) and the collision masks / search
 * cost (cppflow/collision_detection.py:27-69, cppflow/search.py:146-150) of the result evaluated in the same launch. */
int cppf_lm_pose_steps(const cppf_robot* robot, const float* x_in, const float* target, int S, int W,
                       const cppf_lm_params* params, const cppf_lm_outputs* out, void* stream);

/* Several INDEPENDENT problems of the same robot in ONE launch of the same kernel (row shape).  The reference's entry point takes one
 * problem per call (run_lm_optimization, cppflow/optimization.py:376-426; its parallel_count replicates ONE target path); a planner
 * that serves several requests at once, or a GPU that holds only a shard of the candidate seeds (cppflow/planners.py:231-251 split
 * over 8 GPUs leaves 128 seeds = half a wavefront per SIMD on each), cannot fill the MI355X with one such launch: four small
 * launches in flight is all the hardware overlaps, and each costs one wavefront's full latency however few rows it has.  A batch
 * lays up to CPPF_MAX_BATCH problems end to end in one grid -- every workgroup belongs to exactly one problem, so each problem's
 * results are bit for bit those of cppf_lm_pose_steps on it alone -- and the launch is full width again.
 * Each item is what cppf_lm_pose_steps takes: x_in [S*W, d], target [W, 7] (items may have different targets, S and W), and its own
 * outputs (J_out / e_out / min_self / min_env are not available in a batch; seed_summary as in cppf_lm_pose_steps: in the launch
 * for W in {64, 128, 256}, else by one reduction launch per such item behind it, which needs the per-row outputs).
 * cppf_lm_batch_create copies the item descriptors to a device table owned by the batch object (the only allocation; the caller's
 * buffers stay the caller's, and must stay valid while the batch is used); cppf_lm_batch_launch is then one asynchronous launch on
 * `stream`, hipGraph-capturable, reading the robot's obstacles / joint-limit padding as they are at launch time.
 * cppf_lm_params.shape must be CPPF_SHAPE_AUTO or CPPF_SHAPE_ROW (a batch is the throughput shape by construction). */
typedef struct cppf_lm_batch_item {
    const float* x_in;   /* [S*W, d] */
    const float* target; /* [W, 7] */
    int32_t S, W;
    cppf_lm_outputs out;
} cppf_lm_batch_item;
typedef struct cppf_lm_batch cppf_lm_batch; /* opaque: device table of the items + the marshalled parameters */
int cppf_lm_batch_create(const cppf_robot* robot, int n_items, const cppf_lm_batch_item* items /* HOST */,
                         const cppf_lm_params* params, cppf_lm_batch** out);
int cppf_lm_batch_launch(const cppf_lm_batch* batch, void* stream); /* CPPF_ERR_INVALID once its robot has been destroyed */
void cppf_lm_batch_destroy(cppf_lm_batch* batch);                   /* also releases a robot that was destroyed before it (see "Ownership") */

/* qpaths_batched_self_collisions / qpaths_batched_env_collisions (cppflow/collision_detection.py:27-69) +
 * joint_limit_almost_violations_3d + q_costs_external (cppflow/search.py:25-52, 146-150) for q [S,W,d]. Outputs [S*W]. */
int cppf_collision_masks(const cppf_robot* robot, const float* q, int S, int W, uint8_t* self_mask, uint8_t* env_mask,
                         uint8_t* jlim_mask, float* ext_cost, float* min_self, float* min_env, void* stream);

/* Obstacle scenes: q [S*W, d] against n_obs <= CPPF_MAX_SCENE_OBSTACLES axis-aligned cuboids held in DEVICE memory (box_lo / box_hi
 * [n_obs, 3], world-frame corners, formed as cppf_set_obstacles forms them: translation + local corner in fp32), in one call.  The
 * handle's own <= CPPF_MAX_OBSTACLES cuboids are neither read nor changed.  With d(r,c,o) = sqrt(seg_box_dist2) - radius of capsule c
 * -- bit for bit the value cppf_collision_masks' min_env is the minimum of -- and D(r,o) = min_c d(r,c,o):
 *   env_mask[r]    = any_o D(r,o) < 0                                         (exact whatever reach_m is)
 *   min_env[r]     = min_o D(r,o) if that is < reach_m, else +inf              (n_obs = 0: +inf, mask 0)
 *   nearest_obs[r] = the lowest o attaining a finite min_env[r], else -1
 *   obs_min[o]     = min_r D(r,o) if that is < reach_m, else +inf              (what a planner picks its active cuboids by)
 * reach_m in [0, +inf]: distances are truncated there, which lets the kernel skip cuboids no row of a wavefront comes near; every
 * output is bit-identical to the unculled definition and the same on every run.  min_env / nearest_obs / obs_min may be NULL (all
 * three NULL: the mask-only form, no square roots).  workspace: cppf_scene_workspace_bytes(S*W, n_obs) bytes, 16-byte aligned,
 * device; its contents on return are scratch.  Three launches on `stream` (keys to all-ones, the scene kernel, the decode), asynchronous, no host synchronisation, capturable
 * in a graph.  CPPF_ERR_INVALID, before the device is selected: a NULL / destroyed handle, NULL pointers, n_obs out of range, a NaN or
 * negative reach_m, a short or misaligned workspace.  n_obs = 0 is valid. */
#define CPPF_MAX_SCENE_OBSTACLES 4096
int cppf_scene_workspace_bytes(int n_rows, int n_obs, size_t* bytes);
int cppf_scene_env_collisions(const cppf_robot* robot, const float* q, int S, int W, const float* box_lo, const float* box_hi, int n_obs,
                              float reach_m, uint8_t* env_mask, float* min_env, int32_t* nearest_obs, float* obs_min, void* workspace,
                              size_t workspace_bytes, void* stream);

/* The MOTION between the waypoints of q [S, W, d] (W >= 2), certified collision-free or not: the adaptive-clearance test (Schwarzer,
 * Saha, Latombe) on M = 2^level equal intervals per transition, level in 0 .. CPPF_MOTION_MAX_LEVEL, against the robot's self pairs and
 * a scene box_lo / box_hi [n_obs, 3] exactly as cppf_scene_env_collisions takes it (DEVICE memory, 0 <= n_obs <=
 * CPPF_MAX_SCENE_OBSTACLES; the handle's own cuboids are neither read nor changed; n_obs = 0: self only).  The reference has no
 * counterpart: everything it calls collision-free is decided at the waypoints (cppflow/collision_detection.py:27-69).
 *   Nodes.  Transition t of path s goes from a = q[s,t] to b = q[s,t+1] on the straight line in the STORED joint values -- there is no
 *   wrapping: a caller with continuous joints unwraps first.  Node 0 is a itself, node M is b itself, node i in between is
 *   fmaf(i / M, b - a, a) per joint (the subtraction in fp32; i / M is exact).  `nodes` [S, W-1, M+1, d] (may be NULL) returns them.
 *   Clearances at a node.  For a self pair: the value cppf_self_collision_distances gives.  For (capsule c, cuboid o):
 *   min(sqrt_rn(seg_box_dist2) - cap_r[c], reach_m), reach_m in [0, +inf]: the truncation keeps the scene kernel's culling legal and can
 *   only make a certificate harder.
 *   Travel bound.  A table built by cppf_robot_create in double precision and rounded UP to fp32 (cppf_motion_rho reads it):
 *   with l = cap_link[c], for a revolute joint j <= l
 *       rho[j][c] = sum_{i=j+1..l} |t_i| + sum_{prismatic i in (j, l]} max(|lo_i|, |hi_i|) + max(|p0_c|, |p1_c|) + r_c
 *   (t_i the translation of F_i: the distance of any point of the capsule from joint j's origin, hence from its axis); 1 for a prismatic
 *   joint j <= l; 0 for j > l.  Against a cuboid lambda_c = sum_j |b_j - a_j| rho[j][c]; for a self pair (c1, c2) on links l1 <= l2 only
 *   the joints in between count, lambda_p = sum_{l1 < j <= l2} |b_j - a_j| rho[j][c2] (0 for a pair on one link); fp32, joints
 *   ascending, one fmaf each.  One interval's bound is lambda / M.
 *   Verdict per transition, status [S, W-1]:
 *     CPPF_MOTION_CERTIFIED  every interval (i, i+1), every self pair and every (capsule, cuboid) has
 *                            (clear_i + clear_{i+1}) - lambda / M > 1e-6 (the micrometre covers the fp32 accumulation of lambda), both
 *                            waypoints lie inside the joint limits (outside them the prismatic term is no bound) and no node is hit;
 *     CPPF_MOTION_HIT        some node has a clearance < 0;
 *     neither bit            undecided.  The two bits are never set together.
 *   min_clear [S, W-1] (may be NULL): the minimum over the transition's nodes of min(min_self, min_env) as cppf_collision_masks and
 *   cppf_scene_env_collisions (at the same reach_m: +inf beyond it) report them for the node, bit for bit.  hit_node [S, W-1] (may be
 *   NULL): the lowest node index with a negative clearance, else -1.
 * workspace: cppf_motion_workspace_bytes(S, W) bytes, 16-byte aligned, device; scratch on return.  Three launches on `stream`,
 * asynchronous, no host synchronisation, capturable in a graph; no output depends on the order in which anything arrives.
 * CPPF_ERR_INVALID, before the device is selected: a NULL / destroyed handle, NULL q / status / corners, level out of range, W < 2,
 * n_obs out of range, a NaN or negative reach_m, a short or misaligned workspace.  A handle specialised at run time is served by the
 * generic kernel. */
#define CPPF_MOTION_MAX_LEVEL 6
#define CPPF_MOTION_CERTIFIED 1
#define CPPF_MOTION_HIT 2
int cppf_motion_workspace_bytes(int S, int W, size_t* bytes);
int cppf_motion_clearance(const cppf_robot* robot, const float* q, int S, int W, int level, const float* box_lo, const float* box_hi,
                          int n_obs, float reach_m, uint8_t* status, float* min_clear, int32_t* hit_node, float* nodes, void* workspace,
                          size_t workspace_bytes, void* stream);
/* the travel-bound table of the handle, HOST rho[CPPF_MAX_DOF][CPPF_MAX_CAPSULES] (needs no device) */
int cppf_motion_rho(const cppf_robot* robot, float* rho);

/* The same test made ADAPTIVE, as Schwarzer, Saha and Latombe state it: only the intervals whose test fails are bisected, until they
 * pass, a node penetrates, or a resolution floor is reached.  q, the scene, reach_m, the clearances and their truncation at reach_m,
 * rho, lambda_c, lambda_p, the 1e-6 slack, the joint-limit rule and "no wrapping" are those of cppf_motion_clearance.
 *   Nodes and intervals.  Node (L, i), 0 <= i <= 2^L, is a itself for i = 0, b itself for i = 2^L, otherwise fmaf(i 2^-L, b - a, a) per
 *   joint (the subtraction in fp32): (L, i) and (L+1, 2i) are the same bits.  Interval (L, i) lies between the nodes (L, i) and
 *   (L, i+1).  It PASSES when every self pair and every (capsule, cuboid) has (clear_i + clear_{i+1}) - lambda 2^-L > 1e-6 (fp32, in
 *   that order); a cuboid beyond reach_m at both ends counts with reach_m at both ends, whatever the kernel's culling skips.
 *   Per transition tr of [S, W-1], breadth first -- no output depends on any order of arrival:
 *     0. decided != NULL and decided[tr] != 0: the transition is not examined and none of its outputs is written (decided may
 *        alias status: resolve what an earlier call left undecided, in place).
 *     1. L = start_level, F = all 2^L intervals, n_tested = 0, min_clear = +inf.
 *     2. |F| > max_frontier: status = CPPF_MOTION_OVERFLOW, depth = L, stop.
 *     3. Both end nodes of every interval of F are evaluated.  n_tested += |F|; min_clear = min over every evaluated node of
 *        min(min_self, min_env), the per-node value behind cppf_motion_clearance's min_clear (+inf beyond reach_m).
 *     4. An evaluated node has a clearance < 0: status = CPPF_MOTION_HIT, depth = L, hit_num = the lowest such i (the hit sits at
 *        parameter hit_num / 2^depth), stop.
 *     5. A waypoint lies outside the joint limits: status = 0, depth = L, stop.
 *     6. F' = the children (L+1, 2i) and (L+1, 2i+1) of every interval of F that does not pass.  F' empty: status =
 *        CPPF_MOTION_CERTIFIED, depth = L, stop.
 *     7. L == max_depth: status = 0 (undecided), depth = L, stop.  Otherwise F = F', L = L + 1, back to 2.
 *   status u8 [S, W-1]; depth, hit_num (-1 unless HIT), n_tested int32 [S, W-1] and min_clear float [S, W-1] may each be NULL.
 *   CPPF_MOTION_OVERFLOW (bit 2) is never set together with bit 0 or 1.
 * With start_level == max_depth == L and decided == NULL, status and min_clear equal cppf_motion_clearance(level = L) bit for bit and
 * hit_num equals its hit_node.
 * start_level in 0 .. CPPF_MOTION_MAX_LEVEL, max_depth in start_level .. CPPF_MOTION_RESOLVE_MAX_DEPTH, max_frontier in
 * 2^start_level .. CPPF_MOTION_RESOLVE_MAX_FRONTIER, W >= 2, n_obs and reach_m as above.  workspace:
 * cppf_motion_resolve_workspace_bytes(S, W, max_frontier) bytes, 16-byte aligned, device; scratch on return.  One launch on `stream`,
 * asynchronous, no host synchronisation, capturable in a graph; two runs give the same bits.  CPPF_ERR_INVALID, before the device is
 * selected: a NULL / destroyed handle, NULL q / status / corners, start_level, max_depth or max_frontier out of range, W < 2, S < 0,
 * n_obs out of range, a NaN or negative reach_m, a short or misaligned workspace.  A handle specialised at run time is served by the
 * generic kernel. */
#define CPPF_MOTION_RESOLVE_MAX_DEPTH 16
#define CPPF_MOTION_RESOLVE_MAX_FRONTIER 4096
#define CPPF_MOTION_OVERFLOW 4 /* status bit: undecided because the frontier did not fit; never with bit 0 or 1 */
int cppf_motion_resolve_workspace_bytes(int S, int W, int max_frontier, size_t* bytes);
int cppf_motion_resolve(const cppf_robot* robot, const float* q, int S, int W, int start_level, int max_depth, int max_frontier,
                        const float* box_lo, const float* box_hi, int n_obs, float reach_m, const uint8_t* decided,
                        uint8_t* status, int32_t* depth, int32_t* hit_num, float* min_clear, int32_t* n_tested,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Scenes from sensor data: a point cloud (points [n, 3], world frame) or a depth image becomes the box_lo / box_hi list the four
 * scene readers above take, entirely on the device.  DEVICE pointers only; the library allocates nothing.
 *   Grid.  cppf_voxel_grid { origin[3], voxel_m, dims = (nx, ny, nz) }, each dim in 1 .. CPPF_VOXEL_MAX_DIM; nxp = 64 ceil(nx / 64) is
 *   the padded row length in bits, and nxp ny nz <= CPPF_VOXEL_MAX_CELLS.
 *   Planes.  Plane i of axis k is P_k(i) = fadd_rn(origin[k], fmul_rn((float)i, voxel_m)), i = 0 .. n_k: two separate roundings, on
 *   purpose not an fmaf, so that float32 arithmetic anywhere reproduces every corner bit for bit whatever voxel_m is.  The entry
 *   points check on the host that every P_k is finite and strictly increasing (CPPF_ERR_INVALID otherwise).
 *   Cell of a point.  The index of coordinate p_k is the unique i in [0, n_k) with P_k(i) <= p_k < P_k(i+1) -- decided against the
 *   planes themselves, exactly, for every fp32 input; a point with no such i on some axis is OUTSIDE.
 *   Classes.  Every input falls into exactly one class, tested in this order: INVALID (a non-finite coordinate, or an invalid pixel
 *   of the depth form), OUTSIDE, SELF (removed by the self filter), KEPT.  A cell is occupied if it holds at least one kept point.
 *   Self filter.  q_self [n_self, d], 0 <= n_self <= CPPF_VOXEL_MAX_SELF, and self_margin_m >= 0.  A point p is SELF if for some
 *   configuration and some capsule c of the robot dist2(p, segment_c) < thr2_c, thr2_c = fp32((r_c + self_margin_m)^2) formed on the
 *   host in fp64.  Centre C and half-axis H of the capsule are the canonical capsule FK's (the bits cppf_collision_masks works on);
 *   with D = p - C (fp32), u = clamp(fmaf-chain(D . H) * inv, -1, 1), inv = fp32 1 / (H . H) (0 where H . H = 0: a sphere),
 *   E = fmaf(-u, H, D) per axis, dist2 = E . E (fmaf chain, x first).  n_self = 0 switches the filter off; only then may robot and
 *   q_self be NULL.
 *   Boxes of an occupancy.  An x-RUN of row (y, z) is a maximal interval [x0, x1) of occupied cells.  A run is a HEAD if row
 *   (y-1, z) does not hold the identical maximal run [x0, x1).  A head's box spans y .. y1, y1 the first y' > y whose row (y', z)
 *   does not hold that identical maximal run.  The list is the heads ascending by (z, y, x0):
 *       box_lo = (P_x(x0), P_y(y), P_z(z)),  box_hi = (P_x(x1), P_y(y1), P_z(z+1)).
 *   The union of the boxes is the union of the occupied cells, exactly; their interiors are disjoint; the list depends on the
 *   occupancy alone.  Nothing is merged along z.
 *   Capacity.  0 <= capacity <= CPPF_MAX_SCENE_OBSTACLES: the first min(total, capacity) boxes of the list are written to box_lo /
 *   box_hi [capacity, 3]; nothing beyond is touched.  A scene with total > capacity is NOT a sound scene -- it has lost obstacles:
 *   read counts before using it.
 *   counts int32 [8]: 0 boxes in total, 1 boxes written, 2 occupied cells, 3 kept, 4 outside, 5 invalid, 6 self points, 7 zero.
 *   counts[3..6] sum to the number of inputs.
 *   Depth form.  depth [height, width] fp32 metres, intrinsics (fx, fy, cx, cy), cam_to_world[12] = R row-major, then t.  Pixel
 *   (row v, column u) of depth z is INVALID unless z > z_min && z < z_max (a NaN fails both).  Otherwise, with ifx = 1.0f / fx and
 *   ify = 1.0f / fy formed on the host in fp32, every operation rounded separately and in this order:
 *       xc = fmul(fsub((float)u, cx), fmul(z, ifx)),  yc likewise with v, cy, ify,  zc = z,
 *       w_k = fadd(fadd(fadd(fmul(R_k0, xc), fmul(R_k1, yc)), fmul(R_k2, zc)), t_k);
 *   from there on w takes the point form's path (a non-finite w_k is INVALID).
 * workspace: cppf_voxel_scene_workspace_bytes(grid, n_self) bytes, 16-byte aligned, device; it need not be initialised and is
 * scratch on return.  Up to six launches on `stream`, asynchronous, no host synchronisation, capturable in a graph; the only atomics
 * are integer OR and integer add, so two runs give identical bytes.  n_points = 0 (height width = 0) is valid: 0 boxes.
 * CPPF_ERR_INVALID, before a device is selected: a NULL or destroyed handle with n_self > 0, NULL pointers, dims / cells / n_self /
 * capacity out of range, a non-positive or non-finite voxel_m, planes that are not finite and strictly increasing, a negative or NaN
 * margin, z_min >= z_max, fx or fy zero or not finite, a short or misaligned workspace, n_points < 0, height width >= 2^31. */
#define CPPF_VOXEL_MAX_DIM 1024
#define CPPF_VOXEL_MAX_CELLS (1 << 24)
#define CPPF_VOXEL_MAX_SELF 16
typedef struct cppf_voxel_grid {
    float origin[3];
    float voxel_m;
    int32_t dims[3];
} cppf_voxel_grid;
int cppf_voxel_scene_workspace_bytes(const cppf_voxel_grid* grid, int n_self, size_t* bytes);
int cppf_scene_from_points(const cppf_robot* robot, const float* points, int n_points, const cppf_voxel_grid* grid, const float* q_self,
                           int n_self, float self_margin_m, int capacity, float* box_lo, float* box_hi, int32_t* counts,
                           void* workspace, size_t workspace_bytes, void* stream);
int cppf_scene_from_depth(const cppf_robot* robot, const float* depth, int height, int width, const float intrinsics[4],
                          const float cam_to_world[12], float z_min, float z_max, const cppf_voxel_grid* grid, const float* q_self,
                          int n_self, float self_margin_m, int capacity, float* box_lo, float* box_hi, int32_t* counts,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Scenes fused over frames: a persistent MAP of per-cell hit counts that frames are added to, and the scene of the cells seen in at
 * least min_frames of them.  Grid, planes, cell of a point, classes, self filter, the depth form's arithmetic, the boxes of an
 * occupancy and the capacity rule are the definitions above, word for word.  DEVICE pointers only; the library allocates nothing.
 *   Map.  cppf_voxel_map_bytes(grid) = 16 + nxp ny nz bytes of device memory, 16-byte aligned, the caller's: a 16-byte header --
 *   int32 frames, then three zero words -- and behind it one uint8 counter per cell of the padded grid, cell (x, y, z) at
 *   (z ny + y) nxp + x.  Counters at x >= nx stay 0 (and are not read as cells).  At CPPF_VOXEL_MAX_CELLS the map is 16 MB + 16 B.  cppf_voxel_map_clear zeroes
 *   all of it (header included) in one launch; a map must be cleared once before its first frame.
 *   Adding a frame.  The frame's occupancy is that of cppf_scene_from_points / cppf_scene_from_depth on the same arguments: a cell
 *   is occupied if it holds at least one KEPT input.  Then count = min(count + 1, 255) for every cell the frame occupies, every
 *   other counter unchanged, and frames = min(frames + 1, INT32_MAX).  A counter therefore counts the FRAMES in which its cell held
 *   a kept point, not points.  The map after a set of frames does not depend on their order.  n_points = 0 (height width = 0) is a
 *   valid frame: frames + 1 and no counter changes.
 *   counts int32 [8] of an add call: 0 and 1 zero, 2 the cells this frame occupies, 3 kept, 4 outside, 5 invalid, 6 self inputs of
 *   this frame (they sum to the number of inputs), 7 frames after the call.
 *   Map to scene.  1 <= min_frames <= 255.  A cell is occupied iff count >= min_frames.  merge = CPPF_VOXEL_MERGE_XY: the list is
 *   "Boxes of an occupancy" above -- for a map of one frame and min_frames = 1 byte for byte the list cppf_scene_from_points /
 *   _from_depth give for that frame.  merge = CPPF_VOXEL_MERGE_XYZ: "Boxes merged along z" below.  cppf_scene_from_map reads the
 *   map and does not change it; it takes no robot.
 *   counts int32 [8] of cppf_scene_from_map: 0 boxes in total, 1 boxes written, 2 occupied cells, 3 cells with count >= 1, 4..6 zero,
 *   7 frames.
 *   Boxes merged along z.  Let B(z) be the set of boxes (x0, x1, y, y1) of layer z under "Boxes of an occupancy": its heads, each
 *   with the y1 it reaches.  A box of B(z) is a Z-HEAD if B(z-1) does not contain the identical (x0, x1, y, y1); every box of layer
 *   0 is a z-head.  A z-head's cuboid spans z .. z1, z1 the first z' > z with (x0, x1, y, y1) not in B(z'), or nz.  The list is the
 *   z-heads ascending by (z, y, x0):
 *       box_lo = (P_x(x0), P_y(y), P_z(z)),  box_hi = (P_x(x1), P_y(y1), P_z(z1)).
 *   Each B(z') tiles its layer exactly, so the union of the cuboids is the union of the occupied cells, exactly; the interiors of
 *   the cuboids are disjoint; the list is a function of the occupancy alone.  (A box belongs to exactly one maximal chain of
 *   consecutive layers that hold it, and the chain's first member is its z-head.)
 * workspace: cppf_voxel_scene_workspace_bytes(grid, n_self) bytes for an add call, cppf_voxel_scene_workspace_bytes(grid, 0) for
 * cppf_scene_from_map, 16-byte aligned, device; it need not be initialised and is scratch on return.  Every call is asynchronous on
 * `stream`, makes no host synchronisation and can be captured in a graph: one launch for the clear, up to four for an add call (the
 * three that build the frame's bitset and the integration), five for cppf_scene_from_map.  The only atomics are the integer OR of
 * the point pass and integer adds of counts, so two runs give identical bytes, map included.
 * CPPF_ERR_INVALID, before a device is selected: every refusal of the entry points above (grid, handle with n_self > 0, q_self,
 * margin, the source's own, capacity and boxes, counts, workspace); a NULL or misaligned map; map_bytes other than
 * cppf_voxel_map_bytes(grid) (a short map among them); min_frames outside 1 .. 255; a merge other than the two constants.  robot and
 * q_self may be NULL only with n_self = 0. */
#define CPPF_VOXEL_MERGE_XY 0  /* the existing box list */
#define CPPF_VOXEL_MERGE_XYZ 1 /* merged along z as well */
int cppf_voxel_map_bytes(const cppf_voxel_grid* grid, size_t* bytes);
int cppf_voxel_map_clear(void* map, size_t map_bytes, const cppf_voxel_grid* grid, void* stream);
int cppf_voxel_map_add_points(const cppf_robot* robot, const float* points, int n_points, const cppf_voxel_grid* grid,
                              const float* q_self, int n_self, float self_margin_m, void* map, size_t map_bytes, int32_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream);
int cppf_voxel_map_add_depth(const cppf_robot* robot, const float* depth, int height, int width, const float intrinsics[4],
                             const float cam_to_world[12], float z_min, float z_max, const cppf_voxel_grid* grid, const float* q_self,
                             int n_self, float self_margin_m, void* map, size_t map_bytes, int32_t* counts, void* workspace,
                             size_t workspace_bytes, void* stream);
int cppf_scene_from_map(const void* map, size_t map_bytes, const cppf_voxel_grid* grid, int min_frames, int merge, int capacity,
                        float* box_lo, float* box_hi, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* Robot.self_collision_distances(x) -> [n, n_pairs] (call site cppflow/collision_detection.py:65) */
int cppf_self_collision_distances(const cppf_robot* robot, const float* x, int n, float* dists, void* stream);

/* Robot.env_collision_distances(x, cuboid, Tcuboid) -> [n, n_capsules] for ONE cuboid (HOST cuboid[6], Rt[12]);
 * call site cppflow/collision_detection.py:40 */
int cppf_env_collision_distances(const cppf_robot* robot, const float* x, int n, const float* cuboid, const float* Rt,
                                 float* dists, void* stream);

/* Robot.self_collision_distances_jacobian(x) -> [n, n_pairs, d] and Robot.env_collision_distances_jacobian(x, cuboid,
 * Tcuboid) -> [n, n_capsules, d] (jrl; call sites cppflow/optimization_utils.py:670, 710): d(distance)/dq with the
 * closest points held fixed on their links.  `dists` (same leading shape, may be NULL) receives the distances the
 * gradients belong to, so that a caller needs one launch for both. */
int cppf_self_collision_distances_jacobian(const cppf_robot* robot, const float* x, int n, float* jac, float* dists,
                                           void* stream);
int cppf_env_collision_distances_jacobian(const cppf_robot* robot, const float* x, int n, const float* cuboid,
                                          const float* Rt, float* jac, float* dists, void* stream);

/* calculate_pose_error_cm_deg's two per-row terms (cppflow/evaluation_utils.py:113-116) in metres / radians */
int cppf_pose_error_metrics(const cppf_robot* robot, const float* x, const float* target, int S, int W, float* pos_err_m,
                            float* rot_err_rad, void* stream);

/* Tracking IK in one launch: k candidate joint-space paths along ONE target path (the seed stage of a planner).
 * The path [0, T) is split into S contiguous segments (1 <= S <= T); one lane runs candidate i on segment s and walks the segment's
 * waypoints in order, keeping q in registers:
 *   - first waypoint of a segment: start from q0[i*S + s] (q0 [k*S, d], may be NULL) or, without q0, from a uniform draw in
 *     lo + (hi - lo) * [0.1, 0.9]; n_restart LM iterations;
 *   - every later waypoint: warm start from the previous waypoint's q; n_track LM iterations.
 * An LM block of n iterations is exactly a cppf_lm_pose_steps launch of n_steps = n with clamp = 1 and the same tolerances (row shape):
 * with S = 1, n_random_restarts = 0, no jump bar and the same starts, the result is the chain of per-waypoint launches, in one launch.
 * Recovery ladder: a row that is not converged (tolerances set; the early-out criterion of cppf_lm_params.tol_*) or whose change from
 * the previous row exceeds max_jump_rad on a revolute / max_jump_m on a prismatic joint (0 = that bar off) first continues its warm start
 * up to n_restart iterations in total, then tries up to n_random_restarts fresh random starts of n_restart iterations each, and stops at
 * the first attempt that is converged (when tolerances are set) and within the jump bars; failing that it keeps the attempt with the lowest
 * scaled pose error a_pos^2 |e_pos|^2 + a_rot^2 |e_rot|^2.
 * Outputs (all required): q_out [k, T, d]; pos_err_m / rot_err_rad [k, T] (the definitions of cppf_pose_error_metrics at q_out);
 * status [k, T], bits CPPF_TRACK_*.  Random draws hash (seed, call_index, candidate, segment, waypoint, attempt): the same arguments give
 * bit-identical outputs, another call_index other candidates.  A non-finite q0 row poisons every row of its lane (NaN, status 0); a
 * non-finite target waypoint is written NaN / status 0 by every lane, which carries its q on unchanged. */
typedef struct cppf_track_params {
    float lm_lambda;           /* damping, as cppf_lm_params */
    float alpha_position;      /* as cppf_lm_params */
    float alpha_rotation;      /* as cppf_lm_params */
    int32_t n_restart;         /* >= 1: LM iterations from a fresh start (and the warm continuation's total) */
    int32_t n_track;           /* >= 1: LM iterations from the warm start */
    int32_t n_random_restarts; /* >= 0: R, random restarts of the recovery ladder */
    float tol_pos_m;           /* early-out / convergence tolerances: both or neither (0 = off: no convergence test, no early-out) */
    float tol_rot_rad;
    float max_jump_rad;        /* >= 0: joint-change bar of revolute joints between consecutive rows (0 = off) */
    float max_jump_m;          /* >= 0: the same for prismatic joints (0 = off) */
    uint32_t seed;
    uint32_t call_index;       /* a planner's rerun counter: another value, other candidates */
} cppf_track_params;

#define CPPF_TRACK_CONVERGED 1 /* the row meets tol_pos_m / tol_rot_rad */
#define CPPF_TRACK_RESTARTED 2 /* the row's q comes from a fresh start: the first row of a segment or a random restart */
#define CPPF_TRACK_JUMP 4      /* the row's change from the previous row exceeds a jump bar */
#define CPPF_TRACK_RECOVERED 8 /* the row's q comes from the continued warm start of the ladder */

int cppf_track_paths(const cppf_robot* robot, const float* target, int T, int k, int S, const cppf_track_params* params,
                     const float* q0, float* q_out, float* pos_err_m, float* rot_err_rad, uint8_t* status, void* stream);

/* Validity half of x_is_valid for every seed (cppflow/optimization_utils.py:845-884, evaluation_utils.py:29-75):
 * out [S,4] = max position error (cm), max rotation error (deg), max |revolute joint change| (deg),
 * max |prismatic joint change| (cm) over the seed's W waypoints. */
int cppf_seed_validity(const cppf_robot* robot, const float* x, const float* target, int S, int W, float* out,
                       void* stream);

/* Plan metrics of S joint-space paths at once -- the properties of `Plan` (cppflow/data_types.py:140-264), which the
 * reference evaluates one path at a time on the host: x [S*W,d], target [W,7] -> out [S,16] =
 *   [0] max, [1] mean positional error (cm)            (data_types.py:166-186, evaluation_utils.py:134-136)
 *   [2] max, [3] mean rotational error (deg)           (data_types.py:156-164, evaluation_utils.py:139-141)
 *   [4] mjac of the revolute joints (deg), [5] of the prismatic joints (cm)  (data_types.py:189-210, evaluation_utils.py:83-99)
 *   [6] path length of the revolute joints (rad), [7] of the prismatic joints (m)      (data_types.py:141-149)
 *   [8] number of (waypoint, joint) entries outside the joint limits       (evaluation_utils.py:16-27)
 *   [9] number of self-colliding, [10] of environment-colliding waypoints (sums of the given masks; 0 for a NULL mask)
 *   [11] ||q_init - q_path[0]||_2, 0 when q_init (DEVICE [d]) is NULL       (data_types.py:217-221)   [12..15] 0
 * self_mask / env_mask [S*W] are the outputs of cppf_collision_masks / cppf_lm_pose_steps for the same x (may be NULL). */
int cppf_plan_metrics(const cppf_robot* robot, const float* x, const float* target, int S, int W, const uint8_t* self_mask,
                      const uint8_t* env_mask, const float* q_init, float* out, void* stream);

/* Per-seed reduction of the per-row outputs of cppf_lm_pose_steps (no FK is repeated): out [S,8] =
 *   max position error (cm), max rotation error (deg), max |revolute joint change| (deg), max |prismatic joint change| (cm)
 *   -- the four quantities x_is_valid thresholds (cppflow/optimization_utils.py:861-884, evaluation_utils.py:29-75) --
 *   then # self-colliding, # env-colliding, # joint-limit-padding waypoints and the summed external cost (search.py:146-150).
 * 32 bytes per seed: the payload a multi-GPU run all-gathers every step (the per-row buffer is 15 B per row). */
int cppf_seed_summary(const cppf_robot* robot, const float* x, int S, int W, const float* ext_cost, const float* pos_err_m,
                      const float* rot_err_rad, const uint8_t* self_mask, const uint8_t* env_mask,
                      const uint8_t* jlim_mask, float* out, void* stream);

/* Constraints (cppflow/data_types.py:53-62; CLI values scripts/evaluate.py:51-56: 0.01 cm, 0.1 deg, 7 deg, 2 cm) and the two
 * collision switches of cppflow/config.py:23-24 that x_is_valid reads (cppflow/optimization_utils.py:889, 896). */
typedef struct cppf_constraints {
    float max_allowed_position_error_cm;
    float max_allowed_rotation_error_deg;
    float max_allowed_mjac_deg;
    float max_allowed_mjac_cm;
    int32_t self_collisions_ignored;
    int32_t env_collisions_ignored;
} cppf_constraints;

/* The seed selection of x_is_valid (cppflow/optimization_utils.py:856-909) over the per-seed summaries [S,8] of
 * cppf_seed_summary / cppf_lm_outputs.seed_summary -- of one GPU, or of every rank after the all-gather: a seed is valid
 * when its four maxima are strictly below the constraints (cppflow/evaluation_utils.py:29-75) and it has no self- /
 * environment-colliding waypoint.  out (DEVICE int32 [4]) = { first valid seed in order or -1, number of valid seeds,
 * seed of smallest summed external cost (first on ties), 0 }.  One small launch. */
int cppf_select_valid_seed(const cppf_robot* robot, const float* seed_summary, int S, const cppf_constraints* constraints,
                           int32_t* out, void* stream);
/* The same over what ONE all-gather of [n_groups, S_chunk, 8] buffers from n_chunks ranks leaves behind
 * (gathered [n_chunks, n_groups, S_chunk, 8]: the summaries of n_groups consecutive steps travel in one collective): group g
 * is the n_chunks * S_chunk seeds of step g in rank order, seed index = rank * S_chunk + s.  out: DEVICE int32 [n_groups, 4]. */
int cppf_select_valid_seed_gathered(const cppf_robot* robot, const float* gathered, int n_chunks, int n_groups, int S_chunk,
                                    const cppf_constraints* constraints, int32_t* out, void* stream);

/* cppflow/lm_hyper_parameters.py:14-56: the fields the coupled step reads (values of ALT_LOSS_V2_1_DIFF at :86-118) */
typedef struct cppf_full_params {
    float lm_lambda;
    float alpha_position, alpha_rotation;        /* pose block (only when use_pose) */
    float alpha_differencing;                    /* 0.00375 */
    float alpha_differencing_prismatic_scaling;  /* 1.0 */
    float alpha_virtual_configs;                 /* multiplies alpha_differencing */
    float alpha_self_collision, alpha_env_collision; /* 0.01, 0.01 */
    int32_t use_pose, use_differencing, use_virtual_configs, n_virtual_configs, use_self_collisions, use_env_collisions;
    /* The "satisfied" row options of LmResidualFns.get_r_and_J (off in both presets; all zero = off).
     *   pose_do_scale_down_satisfied (cppflow/optimization_utils.py:514-533, :288-333): a pose row whose unscaled |error| is below
     *     pose_threshold_rad (rotation rows) / pose_threshold_m (position rows) is multiplied by pose_scale_down, r and J alike.
     *     The caller forms the thresholds (the reference: pose_ignore_satisfied_threshold_scale x the constraint).
     *   differencing_mode (:548-606): 1 = differencing_do_ignore_satisfied -- rows with |joint change| <= threshold leave the system,
     *     the others are shifted towards zero by the threshold (filter_rows_from_r_J_differencing, :736-768; no prismatic scaling
     *     in this mode, :601); 2 = differencing_do_scale_satisfied -- rows below the threshold are multiplied by
     *     differencing_scale_down, the others optionally shifted (:352-398).  Thresholds: rad for revolute, m for prismatic
     *     joints (the reference: max_allowed_mjac - margin).  A step with differencing_mode != 0 is eliminated by the
     *     one-lane-per-trajectory kernel (the couplings between consecutive waypoints differ from row to row). */
    int32_t pose_do_scale_down_satisfied;
    float pose_threshold_m, pose_threshold_rad, pose_scale_down;
    int32_t differencing_mode;
    float differencing_threshold_rad, differencing_threshold_m, differencing_scale_down;
    int32_t differencing_shift_invalid_to_threshold;
} cppf_full_params;

/* levenberg_marquardt_full (cppflow/optimization.py:95-144) with the residual / Jacobian of LmResidualFns.get_r_and_J
 * (cppflow/optimization_utils.py:486-731, the "satisfied" scaling / filtering options included): one coupled LM step for each
 * of S trajectories x_in [S*W, d] (the reference: one trajectory, :128).
 * target [W,7]; virtual_configs [S*W, d] or NULL (= x_in, which is what the loop sets at optimization.py:253).
 * Obstacles are those of cppf_set_obstacles.  The normal matrix is never formed densely: it is block-tridiagonal and is
 * eliminated per trajectory.  Workspace (device): work_blocks [S*W * (d(d+1)/2 + d)], work_G [S*W * d*d],
 * work_y [S*W * d] floats.  x_out [S*W, d] must not alias x_in.  CPPF_ERR_INVALID, before a device is selected or anything
 * launched: a NULL / destroyed handle, NULL params, S < 0, W < 1 or S*W beyond 2^31-1, lm_lambda <= 0, 2 * n_virtual_configs >= W,
 * a differencing_mode outside 0 .. 2, a scale-down in use outside [0, 1), x_out == x_in, and (S > 0) a NULL pointer other than
 * virtual_configs. */
int cppf_lm_full_step(const cppf_robot* robot, const float* x_in, const float* target, const float* virtual_configs, int S,
                      int W, const cppf_full_params* params, float* work_blocks, float* work_G, float* work_y,
                      float* x_out, void* stream);

/* The same step with the start and / or the goal configuration held fixed.  pin_mask = CPPF_PIN_FIRST | CPPF_PIN_LAST (any
 * combination; 0 is cppf_lm_full_step bit for bit, anything else CPPF_ERR_INVALID): waypoint 0 and / or W-1 of EVERY trajectory
 * is a constant of the optimisation, its value whatever x_in holds in that row.  Its columns leave the system: its pose,
 * collision and virtual-config rows vanish, the differencing row to its free neighbour n keeps n's column only (a_j^2 on the
 * diagonal of n's block, -+ a_j^2 wrap(x_n - x_p) on its right-hand side, as for any other neighbour), and the coupling between
 * the two is gone -- a boundary condition of the block elimination.  Virtual-config membership (t < n or t >= W - n) stays indexed
 * on the full path.  x_out of a pinned row is a copy of x_in (no arithmetic touches it); with no free waypoint (W = 1, or W = 2
 * with both ends pinned) x_out == x_in.  Same workspaces as cppf_lm_full_step.  Served by the parallel-in-time, the row-per-lane
 * and the one-lane elimination; CPPF_ERR_UNSUPPORTED -- before anything is launched or a device selected -- together with the
 * "satisfied" row options (differencing_mode != 0, pose_do_scale_down_satisfied) and for the one-wavefront-per-trajectory
 * cross-check kernel (CPPF_TUNE_FULL_ROWS = 0 beyond the parallel-in-time form's sizes).  CPPF_ERR_INVALID, before a device is
 * selected: everything cppf_lm_full_step refuses, and a pin_mask outside CPPF_PIN_FIRST | CPPF_PIN_LAST. */
#define CPPF_PIN_FIRST 1
#define CPPF_PIN_LAST 2
int cppf_lm_full_step_pinned(const cppf_robot* robot, const float* x_in, const float* target, const float* virtual_configs, int S,
                             int W, const cppf_full_params* params, int pin_mask, float* work_blocks, float* work_G,
                             float* work_y, float* x_out, void* stream);

/* The same step with its environment rows taken from a whole obstacle scene: n_obs <= CPPF_MAX_SCENE_OBSTACLES axis-aligned cuboids
 * in DEVICE memory (box_lo / box_hi [n_obs, 3], world-frame corners formed as for cppf_scene_env_collisions), instead of the handle's
 * <= CPPF_MAX_OBSTACLES; the handle's own cuboids are neither read nor changed.  Environment rows of a row r: for o = 0 .. n_obs-1
 * ascending and every capsule c ascending, the (capsule, cuboid) pair contributes its row -- the same closest points, distance,
 * gradient and accumulation as in cppf_lm_full_step_pinned -- exactly when it penetrates (distance < 0); a pair that does not
 * contributes nothing.  Hence the contract: whenever the cuboids that penetrate some row of the call can be bound to a handle (at
 * most 8 of them, in ascending index order), x_out equals cppf_lm_full_step_pinned on that handle BIT FOR BIT, whatever else the
 * scene holds; and trajectories whose penetrating cuboids differ each equal the step with their own set bound.  In front of the
 * exact test the kernel culls 64 cuboids at a time against the bounding box of a wavefront's capsules (threshold: largest capsule
 * radius + 1 cm); a culled cuboid cannot penetrate, so the culling changes no bit, and two runs are bit-identical.
 * Workspaces, aliasing rule, pin_mask and the CPPF_ERR_UNSUPPORTED cases are those of cppf_lm_full_step_pinned.  Asynchronous on
 * `stream`, no host synchronisation, capturable in a graph.  n_obs = 0 is valid (the step on a handle without obstacles), and so is
 * params->use_env_collisions = 0 (the scene is then not read).  A handle specialised at run time (cppf_robot_specialize) is served
 * by the generic kernels, as for every coupled step: same bits.  CPPF_ERR_INVALID, before a device is selected: a NULL / destroyed
 * handle, NULL pointers (box_lo / box_hi may be NULL only with n_obs = 0), n_obs out of range, a pin_mask outside
 * CPPF_PIN_FIRST | CPPF_PIN_LAST, and every value cppf_lm_full_step refuses.  The device-side optimiser loop (cppf_lm_optimize_enqueue) does not take a scene. */
int cppf_lm_full_step_scene(const cppf_robot* robot, const float* x_in, const float* target, const float* virtual_configs, int S,
                            int W, const cppf_full_params* params, int pin_mask, const float* box_lo, const float* box_hi,
                            int n_obs, float* work_blocks, float* work_G, float* work_y, float* x_out, void* stream);

/* ---- the alternating LM optimiser loop on the device (run_lm_alternating_loss, cppflow/optimization.py:147-373) -------------------
 * cppf_lm_optimize_enqueue() enqueues `n_iterations` iterations of  { pose step | coupled step ; clamp ; capsule masks ; plan
 * metrics ; decide }  on `stream` and returns without synchronising.  Which step an iteration takes, whether the trajectory is
 * valid, converged or finished is decided ON THE DEVICE by the last kernel of the iteration, from the [S,16] metrics the one before
 * it wrote, with the rules of the reference's loop; the decision lives in a loop-control block in device memory, and every kernel
 * of an iteration returns at once for a trajectory whose record does not ask for it (an iteration enqueued after `done` costs its
 * launches and nothing else).  The caller copies the control block back ONCE, whenever it wants to know.
 *
 * Control block (device, int32 words; the caller initialises it, see below):
 *     cppf_optloop_record  record[C]                   C = S if per_trajectory else 1
 *     cppf_optloop_trace   trace[C][trace_capacity]    one row per iteration the record has decided (those beyond the capacity
 *                                                      are not recorded)
 * per_trajectory = 0: ONE record speaks for all S trajectories, as the reference's loop does (TL = the sum over the trajectories,
 * flags of the last trajectory x_is_valid examined, the snapshot is the whole x).  per_trajectory = 1: every trajectory alternates
 * and terminates on its own.
 * Initial record: mode = CPPF_OPT_MODE_POSE, pose_pos_valid = 1, pose_rot_valid = 0 (the reference leads with a pose step,
 * optimization.py:218-219), last_valid_idx = -1, everything else 0.  A record with mode = CPPF_OPT_MODE_DONE is never touched again. */
#define CPPF_OPT_MODE_POSE 0 /* the next step is the pose-only step (K = 1, no clamp inside) */
#define CPPF_OPT_MODE_DIFF 1 /* the next step is the coupled differencing step (virtual configs := current x) */
#define CPPF_OPT_MODE_DONE 2 /* finished: is_valid, valid_seed_idx, i_final hold the result */

#define CPPF_OPT_ON_POSE_VALID_DIFFERENCING 0
#define CPPF_OPT_ON_POSE_VALID_STOP 1
#define CPPF_OPT_ON_POSE_VALID_CONTINUE 2

typedef struct cppf_optloop_record { /* 16 words */
    int32_t mode;                           /* CPPF_OPT_MODE_*: the step the NEXT iteration takes */
    int32_t pose_pos_valid, pose_rot_valid; /* of the last trajectory x_is_valid examined */
    int32_t converged;                      /* TL change between two consecutive differencing steps fell below the threshold */
    int32_t last_valid_idx;                 /* iteration of the last snapshot, -1 = none */
    int32_t n_steps;                        /* iterations decided so far */
    int32_t has_tl;                         /* last_tl holds the TL after the last differencing step */
    float last_tl;
    int32_t is_valid;       /* a snapshot exists (workspace, see below) */
    int32_t valid_seed_idx; /* first valid trajectory at the last snapshot (0 with per_trajectory) */
    int32_t i_final;        /* valid once mode = DONE: the loop index the reference's loop ends with (its n_steps_taken) */
    int32_t reserved[5];
} cppf_optloop_record;

/* flags: bit 0 pose_pos_valid, 1 pose_rot_valid, 2 mjac_rev_valid, 3 mjac_pris_valid; bits 4-5 is_a_self_collision and bits 6-7
 * is_a_env_collision as 0 = not looked at (the reference's None), 1 = no, 2 = yes.  flags = valid = -1: the iteration ended on the
 * TL rule before validity was evaluated (optimization.py:294-297). */
typedef struct cppf_optloop_trace {
    int32_t mode; /* the step this iteration took */
    float tl;
    int32_t flags;
    int32_t valid;
} cppf_optloop_trace;

typedef struct cppf_optloop_params {
    float pose_lm_lambda, pose_alpha_position, pose_alpha_rotation; /* ALT_LOSS_V2_1_POSE: 1e-6, 3.5, 0.35 */
    cppf_full_params diff;                                          /* ALT_LOSS_V2_1_DIFF (use_pose = 0, differencing_mode = 0) */
    cppf_constraints constraints;                                   /* thresholds (strict <, fp32) and the two collisions-ignored switches */
    int32_t max_n_steps;                   /* >= 1 */
    int32_t return_if_valid_after_n_steps; /* -1 = no such rule */
    int32_t on_pose_valid;                 /* CPPF_OPT_ON_POSE_VALID_* */
    int32_t per_trajectory;
    int32_t trace_capacity; /* >= 0 */
    int32_t reserved;
    double convergence_threshold; /* |TL - previous TL| is formed and compared in double, as the Python loop does */
} cppf_optloop_params;

/* Workspace (device, 16-byte aligned) for S trajectories of W waypoints.  Its first S*W*d floats are the SNAPSHOT: the x of the
 * last valid iteration (per record), what the caller returns when is_valid; the rest is scratch. */
int cppf_lm_optimize_workspace_bytes(const cppf_robot* robot, int S, int W, size_t* bytes);
int cppf_lm_optimize_control_bytes(int S, const cppf_optloop_params* params, size_t* bytes);
/* x [S*W, d] is read and written in place; target [W,7].  Obstacles / limits: those of the handle.  CPPF_ERR_UNSUPPORTED where a
 * step has no gated kernel: fewer than 6 joints or more rows than the quad-shape pose kernel serves, a handle specialised at run
 * time, a coupled step that is not eliminated by the parallel-in-time or the row-per-lane kernels. */
int cppf_lm_optimize_enqueue(const cppf_robot* robot, float* x, const float* target, int S, int W,
                             const cppf_optloop_params* params, void* workspace, int32_t* control, int n_iterations,
                             void* stream);
/* The loop with pinned end waypoints (pin_mask as for cppf_lm_full_step_pinned; 0 is cppf_lm_optimize_enqueue bit for bit): the rows
 * of x that the mask names are never written -- the pose step and the coupled step both write the workspace, and the clamp, the
 * loop's only writer of x, skips them.  Masks, metrics and the decision see the whole path, pinned rows included.  Same workspace
 * and control block. */
int cppf_lm_optimize_enqueue_pinned(const cppf_robot* robot, float* x, const float* target, int S, int W,
                                    const cppf_optloop_params* params, int pin_mask, void* workspace, int32_t* control,
                                    int n_iterations, void* stream);

/* _get_mjacs (cppflow/search.py:100-125): q [k,T,d] -> mjacs [k,k,T-1], mjacs[i,j,t] = max over joints of
 * |wrap(s (q[i,t+1] - q[j,t]))| with s = prismatic_scaling on prismatic joints.  cppf_dp_search does not need it (it never
 * materialises the tensor); provided for callers of the reference helper. */
int cppf_mjacs(const cppf_robot* robot, const float* q, int k, int T, float prismatic_scaling, float* mjacs, void* stream);

/* dp_search(robot, q, ...) of cppflow/search.py:128-191 given the external cost matrix q_costs_external [k,T]
 * (search.py:146-150, the `ext_cost` output of cppf_collision_masks / cppf_lm_pose_steps): the min-max dynamic programme
 * over the k candidate paths q [k,T,d] with mjacs as in search.py:100-125 (prismatic deltas scaled by `prismatic_scaling`,
 * 5.0 in the reference), then the back-trace.  Outputs best_path [T,d] and best_idx [T] (which candidate each waypoint
 * came from).  The caller supplies the workspace (device): work_qT [T*k*d] floats, work_costsT [T*k] floats (on return:
 * the cost table, time-major), work_memoT [T*k] int32.
 * mode = CPPF_DP_AUTO: for k <= 1024 (the reference plans with k = 175 and re-plans with 300, cppflow/planners.py:47, 253-258; eight
 *   ranks gather 1024) the whole recurrence runs in ONE resident launch -- one destination per wavefront (k <= 64) or four per
 *   workgroup, at most 256 workgroups; the cost row of step t-1 is handed from workgroup to workgroup as write-through words that are
 *   their own flags, no grid barrier -- else one small launch per waypoint; no host synchronisation either way.
 * mode = CPPF_DP_RESIDENT / CPPF_DP_LAUNCHES force one form for THIS call (no handle state involved).
 * The resident form needs its <= 256 workgroups on the device together.  The entry point holds the grid against what the device can
 * hold of that kernel (occupancy x compute units) BEFORE launching: a device that cannot (partitioned, CU-masked, smaller) gets one
 * launch per waypoint under CPPF_DP_AUTO and CPPF_ERR_UNSUPPORTED for a forced CPPF_DP_RESIDENT.  Work already on the device can
 * still delay workgroups (another resident search on a second stream, a full-width fused launch): the waits are bounded, and if one
 * expires the call has still returned CPPF_OK -- it is asynchronous -- but best_idx[*] = -1 and best_path is NaN: repeat the call
 * with CPPF_DP_LAUNCHES (cppflow_amd.search.dp_search does).  Do not run two resident searches of > 512 candidates concurrently. */
#define CPPF_DP_AUTO 0
#define CPPF_DP_RESIDENT 1
#define CPPF_DP_LAUNCHES 2
int cppf_dp_search(const cppf_robot* robot, const float* q, const float* ext_cost, int k, int T, float prismatic_scaling,
                   float* work_qT, float* work_costsT, int32_t* work_memoT, float* best_path, int32_t* best_idx, int mode,
                   void* stream);

/* The same dynamic programme for k <= 256 from a precomputed transition table (the mjacs tensor of search.py:100-125, which
 * the reference materialises as well): the table is filled by the whole chip, the recurrence then runs on ONE compute unit
 * (no hand-off between workgroups: one workgroup barrier per waypoint, the table streamed through registers two steps ahead)
 * and the argmins are recovered in a third, parallel launch.  Same outputs, bit for bit, as cppf_dp_search.  Measured at
 * T = 256: 560 vs 720 us at the reference's k = 175, 378 vs 734 us at k = 128, 168 vs 422 us at k = 64; slower at k = 256
 * (one compute unit streams ~80-90 GB/s).  Extra workspace: work_table, cppf_dp_table_floats(k, T) = ((T-1) * k + 32) *
 * roundup(k, 64) floats (34 MB at k = 175, T = 256).  T <= 65536. */
int cppf_dp_table_floats(int k, int T, size_t* n_floats);
int cppf_dp_search_tabled(const cppf_robot* robot, const float* q, const float* ext_cost, int k, int T, float prismatic_scaling,
                          float* work_qT, float* work_costsT, int32_t* work_memoT, float* work_table, float* best_path,
                          int32_t* best_idx, void* stream);

/* The N lowest-cost paths of a finished search that are actually different from each other.  Inputs: the candidates q [k,T,d] and
 * the tables a completed cppf_dp_search / cppf_dp_search_tabled has left -- costsT = work_costsT [T,k], memoT = work_memoT [T,k];
 * they are read, never written.  Every terminal j has a complete best path behind it (idx_j[T-1] = j, idx_j[t-1] =
 * memoT[t][idx_j[t]]).  The terminals are ordered by (costsT[T-1][j], j) ascending -- a cost that is not below +inf counts as +inf --
 * and accepted greedily in that order: a terminal is accepted when its path is at least `min_separation` away from every path
 * accepted before it, where sep(a, b) = max over waypoints and joints of |wrap(s (q[idx_a[t],t] - q[idx_b[t],t]))|, s =
 * prismatic_scaling on prismatic joints (as in cppf_mjacs), 1 otherwise; until n_paths are accepted or the terminals run out.
 * min_separation = 0 gives the plain n_paths lowest-cost terminals.  Slot 0 is the search's own best_path / best_idx, bit for bit.
 * Outputs (device): paths [n_paths,T,d], path_idx [n_paths,T] (the candidate each waypoint came from), path_cost [n_paths] (the
 * terminal's cost), n_found [1].  Slots at or beyond n_found hold NaN paths, -1 indices and +inf cost; n_paths > k is allowed.  If
 * memoT[0] carries the timed-out flag of the resident search (best_idx = -1 there), n_found = -1 and every slot is empty: repeat
 * the search with CPPF_DP_LAUNCHES.  workspace: cppf_dp_nbest_workspace_bytes(k, T, n_paths) bytes, 16-byte aligned, device.
 * Three launches on `stream` (trace of all terminals, selection in one workgroup, gather), asynchronous, no host synchronisation.
 * CPPF_ERR_INVALID, before the device is selected: a NULL / destroyed handle, NULL pointers, k / T / n_paths < 1, a negative or
 * non-finite min_separation, a misaligned workspace, k*T*d or n_paths*T*d beyond 2^31-1. */
int cppf_dp_nbest_workspace_bytes(int k, int T, int n_paths, size_t* bytes);
int cppf_dp_nbest(const cppf_robot* robot, const float* q, const float* costsT, const int32_t* memoT, int k, int T, int n_paths,
                  float min_separation, float prismatic_scaling, void* workspace, float* paths /*[n_paths,T,d]*/,
                  int32_t* path_idx /*[n_paths,T]*/, float* path_cost /*[n_paths]*/, int32_t* n_found /*[1]*/, void* stream);

/* ---- seed sharding across the GPUs of one node: RCCL behind the C ABI ---------------------------------------
 * The reference is one process on one device (no collective anywhere in its tree); the MI355X build shards the candidate seeds
 * of cppflow/planners.py:231-251 over the GPUs and needs ONE collective: an all-gather of each rank's packed per-row / per-seed
 * outputs, so that every rank holds what cppflow/search.py:146-151 consumes.  The library loads RCCL lazily (dlopen of
 * librccl.so.1: the copy already in the process -- e.g. PyTorch's -- or the ROCm one), so a caller that never shards needs no
 * RCCL at all.  Two process models:
 *   - one process (or thread) per GPU: rank 0 calls cppf_comm_unique_id, ships the 128 bytes to the other ranks by any means,
 *     every rank calls cppf_comm_init_rank;
 *   - one process, all GPUs: cppf_comm_init_all creates one communicator per listed device.
 * cppf_allgather_bytes is asynchronous on `stream` (the stream of the communicator's device); with cppf_comm_init_all, issue
 * the calls for all communicators between cppf_comm_group_begin / cppf_comm_group_end. */
typedef struct cppf_comm cppf_comm;
#define CPPF_COMM_ID_BYTES 128

/* CPPF_OK when RCCL can be loaded into this process (dlopen + every symbol the library uses), else CPPF_ERR_UNSUPPORTED with
 * the reason in cppf_last_error(): lets every rank of a job agree on a transport BEFORE anyone enters a collective. */
int cppf_comm_available(void);
int cppf_comm_unique_id(void* id_out /* CPPF_COMM_ID_BYTES */);
int cppf_comm_init_rank(const void* id, int rank, int world, int device, cppf_comm** out);
int cppf_comm_init_all(int n_devices, const int* devices, cppf_comm** out /* [n_devices] */);
int cppf_comm_rank(const cppf_comm* comm);
int cppf_comm_world(const cppf_comm* comm);
/* recv [world * bytes_per_rank] <- every rank's send [bytes_per_rank] in rank order (DEVICE pointers; the packed buffer of
 * cppf_lm_outputs: ext_cost | pos_err_m | rot_err_rad | the three masks, or the [S,8] per-seed summaries). */
int cppf_allgather_bytes(cppf_comm* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int cppf_comm_group_begin(void);
int cppf_comm_group_end(void);
void cppf_comm_destroy(cppf_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* CPPFLOW_HIP_H */
