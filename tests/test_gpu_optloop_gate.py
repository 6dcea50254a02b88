"""The launch gates of the device-side optimiser loop (StepGateK, csrc/lmik_device.h; cppf_lm_optimize_enqueue,
csrc/kernels_optloop.h), ONE gated iteration at a time with the mode pattern chosen by the test, on the MI355X.

The gate is a pure selection, so it has an exact reference: the ungated public entry points (lm_pose_steps, lm_full_step,
clamp_to_joint_limits, collision_masks, plan_metrics) on the same handle under the same `debug_set` tuning and on the whole
[S*W, d] batch -- same kernel, same grid.  Every comparison of the matrix is therefore EQUALITY of bits (tensors are compared as
int32 / uint8 words): x, every section of the sentinel-filled workspace, and the loop-control block, whose expected records and
trace rows come from the host-compiled `optloop_decide` (tests/optloop_shim.py) applied to the preset record and the device's own
metrics row.  Only the anchor against the fp64 oracle (one trajectory per robot) has tolerances, and those are the ones the
project already holds the ungated calls to.

Workspace layout (optloop_layout, restated in `layout`): snapshot | x_new | blocks | G | y | metrics [S,16] | self mask | env mask.
`blocks`, `G` and `y` are row-major per trajectory in every elimination form (the parallel-in-time form with its state in LDS does
not write G at all), so for every trajectory NOT in differencing mode all three must keep the sentinel; for trajectories in
differencing mode their content is the elimination's scratch and is not asserted.

The module checks about itself (from W, S and the pattern, on the host) that the lane patterns it is for do occur: a quad
wavefront (16 rows) / a row wavefront (64 rows) / a row-per-lane wavefront (8 or 4 trajectories) that holds open and closed
trajectories side by side, a partly filled last row-per-lane wavefront whose last trajectory is closed, and every outcome of the
decision.  Nothing is retried; S*W <= 16 384 rows, one enqueued iteration per case."""

import ctypes
import os
import time

import numpy as np
import pytest
import torch

from cppflow_amd import _hip
from cppflow_amd.data_types import Constraints
from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF, ALT_LOSS_V2_1_POSE
from tests import helpers as H
from tests.optloop_shim import build_shim

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7FC0BEEF  # (a NaN pattern, should anything compute on it)
P, D, X = _hip.OPT_MODE_POSE, _hip.OPT_MODE_DIFF, _hip.OPT_MODE_DONE
LETTER = {P: "P", D: "D", X: "X"}
WIDTHS = (0.0, 1e-3, 3e-2, 0.5)
N0, MAX_N_STEPS, RETURN_IF_VALID_AFTER, CONVERGENCE_THRESHOLD = 3, 20, 15, 0.3  # every preset record has taken N0 iterations
PROBLEMS = ("panda__2cubes", "fetch_arm__s__truncated", "fetch__hello")
GENERIC = "generic11"
GENERIC_W = 90
CONSTRAINTS = Constraints(max_allowed_position_error_cm=0.01, max_allowed_rotation_error_deg=0.1, max_allowed_mjac_deg=7.0,
                          max_allowed_mjac_cm=2.0)  # fmt: skip

# what the matrix reached, per robot: filled by test_gate_matrix, held against the conditions by the module's last test
REACHED = {}
WIDTHS_ON_PAPER = {}  # waypoints per problem as counted from the path files by the first test


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("optloop_gate"))


# ---- the cases: patterns, elimination forms, and what they make of a wavefront (host arithmetic only) ------------------------------
def patterns(S):
    """name -> mode per trajectory"""
    rng = np.random.RandomState(1000 + S)
    out = {
        "all_pose": [P] * S,
        "all_diff": [D] * S,
        "alternating": [(P, D, X)[s % 3] for s in range(S)],
        "last_done": [(D, P)[s % 2] for s in range(S - 1)] + [X],
        "random_a": [int(m) for m in rng.choice([P, D, X], size=S)],
        "random_b": [int(m) for m in rng.choice([P, D, D, X], size=S)],
    }
    for where, idx in (("first", 0), ("middle", S // 2), ("last", S - 1)):
        for open_mode in (P, D):
            m = [X] * S
            m[idx] = open_mode
            out[f"one_{LETTER[open_mode]}_{where}"] = m
    return out


def forms(W, ndof):
    """name -> debug_set switches; the parallel-in-time (PCR) forms exist up to 8 joints and 512 waypoints"""
    out = {"default": {}}
    if ndof <= 8:
        out["rows"] = {"pcr_max_rows": 0}
    if ndof <= 8 and W <= 256:
        for v in (0, 1, 2):
            out[f"pcr_lds{v}"] = {"pcr_lds": v}
    return out


def is_row_per_lane(form, W, ndof):
    return ndof > 8 or W > 512 or "pcr_max_rows" in forms(W, ndof)[form]


def mixed_wavefronts(modes, W, rows_per_wave, open_modes):
    """wavefronts of `rows_per_wave` consecutive rows that hold rows of an open and of a closed trajectory"""
    S = len(modes)
    is_open = np.repeat(np.array([m in open_modes for m in modes]), W)
    n, count = S * W, 0
    for r0 in range(0, n, rows_per_wave):
        part = is_open[r0 : r0 + rows_per_wave]
        count += bool(part.any() and not part.all())
    return count


def mixed_trajectory_wavefronts(modes, tpw):
    """row-per-lane elimination, `tpw` trajectories per wavefront: (wavefronts that hold an open (differencing) and a closed
    trajectory, whether the last wavefront is partly filled with its last trajectory closed and an earlier one open)"""
    S = len(modes)
    mixed = 0
    for s0 in range(0, S, tpw):
        part = [m == D for m in modes[s0 : s0 + tpw]]
        mixed += bool(any(part) and not all(part))
    last = modes[(S - 1) // tpw * tpw :]
    partial = S % tpw != 0 and last[-1] != D and any(m == D for m in last[:-1])
    return mixed, partial


# ---- robots, targets and start paths ---------------------------------------------------------------------------------------------
_setups = {}


class Setup:
    """robot, target [W,7], a path worth starting from [W,d], the constraints, the obstacles (cuboids, Tcuboids), the oracle"""

    def __init__(self, name, rb, target, x_base, constraints, cuboids, Tcuboids, oracle):
        self.name, self.rb, self.target, self.x_base, self.constraints = name, rb, target, x_base, constraints
        self.cuboids, self.Tcuboids, self.oracle = cuboids, Tcuboids, oracle
        self.W, self.d = target.shape[0], rb.ndof

    def bind(self):
        self.rb.set_obstacles(self.cuboids, self.Tcuboids)
        self.rb.set_joint_limit_padding(None, None)

    def release(self):
        self.rb.set_obstacles([], [])


def _generic_setup():
    """an 11-joint chain that matches no generated table (generic kernels; sixteen lanes per trajectory in the row-per-lane
    elimination, one quad wavefront per SIMD): the target is FK of a smooth joint path that keeps clear of itself and of one cuboid,
    so that the path itself is a valid trajectory"""
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robots import Robot
    from oracle.oracle import Oracle

    spec = H.random_chain_spec(11, seed=41)
    ch = canonicalize(spec)
    o64, o32 = Oracle(ch, f32=False, threads=8), Oracle(ch, f32=True, threads=8)
    obs = [H.cuboid_obstacle(0.9, 0.9, 0.2, 0.2, 0.2, 0.2)]
    lo, hi = H.box_corners([c for c, _ in obs], [T for _, T in obs])
    rng = np.random.RandomState(41)
    path = None
    for _ in range(200):  # (host only: draw until a whole smooth path is collision-free)
        q0 = rng.uniform(ch.lo + 0.3 * (ch.hi - ch.lo), ch.hi - 0.3 * (ch.hi - ch.lo))
        step = 0.004 * rng.randn(GENERIC_W, ch.ndof)
        step[:, ch.jtype == 1] *= 0.1
        cand = H.f32(np.clip(q0[None] + np.cumsum(step, axis=0), ch.lo + 0.01, ch.hi - 0.01))
        m = o32.masks(cand, lo, hi, None, None)
        if not m["self_mask"].any() and not m["env_mask"].any():
            path = cand
            break
    assert path is not None, "no collision-free smooth path of the generic chain found"
    target = H.f32(o64.fk(path))
    rb = Robot(spec, specialize=False)
    return Setup(GENERIC, rb, torch.tensor(target, dtype=torch.float32, device=DEV), torch.tensor(path, dtype=torch.float32),
                 CONSTRAINTS, [c for c, _ in obs], [T for _, T in obs], o64)  # fmt: skip


def setup(name):
    if name not in _setups:
        if name == GENERIC:
            _setups[name] = _generic_setup()
        else:
            from tests.test_gpu_optloop import _base

            problem, x_base = _base(name)
            _setups[name] = Setup(name, problem.robot, problem.target_path, x_base.cpu(), problem.constraints,
                                  problem.obstacles_cuboids or [], problem.obstacles_Tcuboids or [], H.oracle64(problem.robot.name))  # fmt: skip
    return _setups[name]


def starts(su, S, seed):
    """S copies of the base path, trajectory s perturbed with width WIDTHS[s % 4]"""
    g = torch.Generator().manual_seed(seed)
    out = [su.x_base + WIDTHS[s % 4] * torch.randn(su.x_base.shape, generator=g) for s in range(S)]
    return torch.cat(out, dim=0).to(DEV).contiguous()


def params(su, per_trajectory=1, self_ignored=0, env_ignored=0):
    prm = _hip.OptloopParams()
    prm.pose_lm_lambda, prm.pose_alpha_position = float(ALT_LOSS_V2_1_POSE.lm_lambda), float(ALT_LOSS_V2_1_POSE.alpha_position)
    prm.pose_alpha_rotation = float(ALT_LOSS_V2_1_POSE.alpha_rotation)
    prm.diff = su.rb.full_params(ALT_LOSS_V2_1_DIFF)
    c = su.constraints
    prm.constraints = _hip.Constraints(c.max_allowed_position_error_cm, c.max_allowed_rotation_error_deg, c.max_allowed_mjac_deg,
                                       c.max_allowed_mjac_cm, int(self_ignored), int(env_ignored))  # fmt: skip
    prm.max_n_steps, prm.return_if_valid_after_n_steps, prm.trace_capacity = MAX_N_STEPS, RETURN_IF_VALID_AFTER, MAX_N_STEPS
    prm.on_pose_valid, prm.per_trajectory, prm.convergence_threshold = _hip.OPT_ON_POSE_VALID["differencing"], per_trajectory, CONVERGENCE_THRESHOLD
    return prm


def layout(d, S, W):
    """optloop_layout (csrc/cppflow_hip.hip), in floats: every section a multiple of 4 floats"""

    def up(v):
        return (v + 3) // 4 * 4

    n, nt = S * W, d * (d + 1) // 2
    L, at = {}, 0
    for key, size in (("snapshot", n * d), ("x_new", n * d), ("blocks", n * (nt + d)), ("G", n * d * d), ("y", n * d), ("metrics", S * 16),
                      ("self_mask", (n + 3) // 4), ("env_mask", (n + 3) // 4)):  # fmt: skip
        L[key] = (at, size)
        at += up(size)
    L["total"] = at
    return L


def i32(t):
    return t.contiguous().view(torch.int32)


def differing(got, want, S):
    """trajectories (rows of the [S, -1] view) in which two word tensors differ"""
    return torch.nonzero((got.reshape(S, -1) != want.reshape(S, -1)).any(dim=1)).flatten().tolist()


# ---- one gated iteration against the ungated composition ------------------------------------------------------------------------------
def gated_iteration(su, decide, x0, S, modes, prm, kind_shift=0):
    """Preset the control block to `modes` (record c: per trajectory, or record 0 for all), enqueue ONE iteration on a sentinel
    workspace, and hold x, the workspace and the control block against the ungated calls.  Returns what the decision did."""
    rb, W, d, target = su.rb, su.W, su.d, su.target
    n, per_traj = S * W, bool(prm.per_trajectory)
    C, G = (S, 1) if per_traj else (1, S)
    traj_modes = list(modes) if per_traj else [modes[0]] * S
    self_ign, env_ign = bool(prm.constraints.self_collisions_ignored), bool(prm.constraints.env_collisions_ignored)
    # -- the reference: ungated launches over the whole batch
    x_pose = rb.lm_pose_steps(x0, target, prm.pose_lm_lambda, prm.pose_alpha_position, prm.pose_alpha_rotation, n_steps=1, clamp=False)["x"]
    x_diff = rb.lm_full_step(x0, target, ALT_LOSS_V2_1_DIFF, virtual_configs=x0)
    tm = torch.tensor(traj_modes, device=DEV)
    row_mode = tm.repeat_interleave(W).unsqueeze(1)
    x_step = torch.where(row_mode == D, x_diff, x_pose)  # (rows of a finished trajectory: not used below)
    x_after = torch.where(row_mode == X, x0, rb.clamp_to_joint_limits(x_step.clone()))
    self_m = env_m = None
    if not (self_ign and env_ign):
        masks = rb.collision_masks(x_after.view(S, W, d), only=("self", "env"))
        self_m, env_m = masks["self_mask"].view(-1), masks["env_mask"].view(-1)
    metrics = rb.plan_metrics(x_after, target, None if self_ign else self_m, None if env_ign else env_m)
    # -- the preset control block: every record has taken N0 iterations; four kinds of history, so that the decision has work to do
    workspace, control = rb.lm_optimize_buffers(S, W, prm, DEV)
    words = control.cpu().numpy().copy()
    recs = words[: C * 16].reshape(C, 16)
    tl = metrics.cpu().numpy()[:, 6].reshape(C, G).sum(axis=1)
    for c in range(C):
        r = _hip.OptloopRecord.from_buffer_copy(recs[c].tobytes())
        r.mode, r.n_steps = modes[c], N0
        r.pose_pos_valid, r.pose_rot_valid = 1, int(modes[c] == D)
        kind = (c + kind_shift) % 4
        if kind == 1:  # a valid previous iteration and a TL close by: a differencing step converges and stops at once
            r.has_tl, r.last_tl, r.last_valid_idx, r.is_valid = 1, float(tl[c]) + 0.125, N0 - 1, 1
        elif kind == 2:  # a TL close by, nothing valid yet: a differencing step converges and goes on to the validity check
            r.has_tl, r.last_tl = 1, float(tl[c]) + 0.125
        elif kind == 3:  # converged earlier: ends as soon as the trajectory is valid, whatever the step
            r.has_tl, r.last_tl, r.converged = 1, float(tl[c]) + 5.0, 1
        recs[c] = np.frombuffer(bytes(r), dtype=np.int32)
    control.copy_(torch.from_numpy(words))
    control_before = words.copy()
    sentinel = torch.full_like(i32(workspace), SENTINEL)
    i32(workspace).copy_(sentinel)
    x = x0.clone()
    # -- the gated iteration
    rb.lm_optimize_enqueue(x, target, prm, workspace, control, 1)
    torch.cuda.synchronize()
    ws = i32(workspace)
    L = layout(d, S, W)
    assert ws.numel() == L["total"]

    def section(t, key):
        return t[L[key][0] : L[key][0] + L[key][1]]

    live = [m != X for m in traj_modes]
    live_t, diff_t = torch.tensor(live, device=DEV), tm == D
    what = f"{su.name} S={S} modes={''.join(LETTER[m] for m in modes)} per_trajectory={int(per_traj)}"
    # x
    assert torch.equal(i32(x), i32(x_after)), f"{what}: x differs in trajectories {differing(i32(x), i32(x_after), S)}"
    # the workspace, section by section (what is not named keeps the sentinel, the padding between sections included)
    want = sentinel.clone()
    rows_live, rows_diff = live_t.repeat_interleave(W).unsqueeze(1), diff_t.repeat_interleave(W).unsqueeze(1)
    section(want, "x_new").copy_(torch.where(rows_live, i32(x_step), section(sentinel, "x_new").view(n, d)).view(-1))
    for key, per_row in (("blocks", d * (d + 1) // 2 + d), ("G", d * d), ("y", d)):
        section(want, key).copy_(torch.where(rows_diff, section(ws, key).view(n, per_row), section(sentinel, key).view(n, per_row)).view(-1))
    section(want, "metrics").copy_(torch.where(live_t.unsqueeze(1), i32(metrics), section(sentinel, "metrics").view(S, 16)).view(-1))
    if not (self_ign and env_ign):
        for key, m in (("self_mask", self_m), ("env_mask", env_m)):
            sec = section(want, key).view(torch.uint8)
            sec[:n].copy_(torch.where(rows_live.view(-1), m.view(torch.uint8), sec[:n]))
    # the decision: the host-compiled function on the preset record and the device's own metrics rows
    got_metrics = section(ws, "metrics").view(torch.float32).cpu().numpy().reshape(S, 16)
    want_control = control_before.copy()
    want_recs, want_trace = want_control[: C * 16].reshape(C, 16), want_control[C * 16 :].reshape(C, prm.trace_capacity, 4)
    snaps, outcomes = [], []
    for c in range(C):
        if modes[c] == X:
            continue
        r, tr = _hip.OptloopRecord.from_buffer_copy(want_recs[c].tobytes()), _hip.OptloopTrace()
        m = np.ascontiguousarray(got_metrics[c * G : (c + 1) * G], dtype=np.float32)
        snap = decide.shim_decide(ctypes.byref(prm), ctypes.byref(r), m.ctypes.data, G, ctypes.byref(tr))
        want_recs[c] = np.frombuffer(bytes(r), dtype=np.int32)
        want_trace[c, N0] = np.frombuffer(bytes(tr), dtype=np.int32)
        snaps.append(snap)
        if r.mode == X:
            outcomes.append("stop_now" if (modes[c] == D and tr.flags == -1 and not snap) else
                            "valid_and_converged" if (snap and r.converged) else "done_otherwise")  # fmt: skip
        else:
            outcomes.append("live_pose" if r.mode == P else "live_diff")
        if snap:
            rows = slice(c * G * W, (c + 1) * G * W)
            section(want, "snapshot").view(n, d)[rows] = i32(x_after)[rows]
    for key in ("snapshot", "x_new", "blocks", "G", "y", "metrics", "self_mask", "env_mask"):
        a, b = section(ws, key), section(want, key)
        if not torch.equal(a, b):
            per = S if key != "metrics" and not key.endswith("mask") else 1
            where = differing(a, b, per) if a.numel() % per == 0 else "?"
            raise AssertionError(f"{what}: workspace section '{key}' differs (trajectories {where}; {int((a != b).sum())} words)")
    assert torch.equal(ws, want), f"{what}: the padding between workspace sections was written"
    got_control = control.cpu().numpy()
    assert np.array_equal(got_control, want_control), (
        f"{what}: control block differs in words {np.flatnonzero(got_control != want_control)[:16].tolist()} (records are 16 words)")  # fmt: skip
    return dict(snaps=snaps, outcomes=outcomes)


def run_with(rb, switches, fn):
    try:
        for k, v in switches.items():
            rb.debug_set(k, v)
        return fn()
    finally:
        for k in switches:
            rb.debug_set(k, None)


def note(reached, res):
    reached["outcomes"].update(res["outcomes"])
    reached["mixed_snapshot_launch"] |= (0 in res["snaps"]) and (1 in res["snaps"])


def test_widths_and_patterns_reach_the_lane_mixes_on_paper():
    """no launch: each W splits a wavefront between two trajectories, and the patterns contain the mixes the matrix is for"""
    import csv

    ref = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_files", "paths")
    widths = {}
    for name, path in (("panda__2cubes", "2cubes.csv"), ("fetch_arm__s__truncated", "s_truncated.csv"), ("fetch__hello", "hello.csv")):
        with open(os.path.join(ref, path)) as f:
            widths[name] = sum(1 for row in csv.reader(f) if row) - 1  # (one header line)
    widths[GENERIC] = GENERIC_W
    assert widths == {"panda__2cubes": 200, "fetch_arm__s__truncated": 59, "fetch__hello": 553, GENERIC: GENERIC_W}
    WIDTHS_ON_PAPER.update(widths)
    for name, W in widths.items():
        assert W % 16 != 0, (name, W)
        tpw = 4 if name == GENERIC else 8
        quad = rows = traj = partial = 0
        for S in (2, 3, 9, 11):
            assert S * W <= 16384
            for modes in patterns(S).values():
                quad += mixed_wavefronts(modes, W, 16, (P,))
                rows += mixed_wavefronts(modes, W, 64, (D,)) + mixed_wavefronts(modes, W, 64, (P, D))
                m, p = mixed_trajectory_wavefronts(modes, tpw)
                traj, partial = traj + m, partial + p
        assert quad > 0 and rows > 0 and traj > 0 and partial > 0, (name, quad, rows, traj, partial)


@pytest.mark.parametrize("name", PROBLEMS + (GENERIC,))
def test_gate_matrix(name, decide):
    """S x pattern x elimination form, per_trajectory = 1: see the module docstring for what is compared.  The conditions at the
    end are about the matrix itself (computed from W, S and the pattern): it did contain the wavefronts it is for."""
    su = setup(name)
    su.bind()
    W, d = su.W, su.d
    assert W % 16 != 0 and WIDTHS_ON_PAPER.get(name, W) == W
    tpw = 8 if d <= 8 else 4  # trajectories per wavefront of the row-per-lane elimination
    reached = REACHED.setdefault(name, dict(outcomes=set(), mixed_snapshot_launch=False))
    quad_mixed = rows_mixed = traj_mixed = traj_partial = n_cases = 0
    t0 = time.time()
    try:
        for S in (2, 3, 9, 11):
            assert S * W <= 16384
            x0 = starts(su, S, seed=S)
            for k, (pname, modes) in enumerate(patterns(S).items()):
                for form, switches in forms(W, d).items():
                    prm = params(su)
                    res = run_with(su.rb, switches, lambda: gated_iteration(su, decide, x0, S, modes, prm, kind_shift=k))
                    note(reached, res)
                    q = mixed_wavefronts(modes, W, 16, (P,))
                    r = mixed_wavefronts(modes, W, 64, (D,)) + mixed_wavefronts(modes, W, 64, (P, D))
                    t, p = mixed_trajectory_wavefronts(modes, tpw) if is_row_per_lane(form, W, d) else (0, False)
                    print(f"{name} W={W} S={S} {pname}={''.join(LETTER[m] for m in modes)} form={form} mixed wavefronts: quad {q}, "
                          f"row {r}, row-per-lane {t}{' (+ partly filled, last closed)' if p else ''}; outcomes {sorted(set(res['outcomes']))}")
                    quad_mixed, rows_mixed, traj_mixed, traj_partial = quad_mixed + q, rows_mixed + r, traj_mixed + t, traj_partial + int(p)
                    n_cases += 1
    finally:
        su.release()
    print(f"{name}: {n_cases} cases in {time.time() - t0:.1f} s")
    assert quad_mixed > 0, "no quad wavefront held an open and a closed trajectory"
    assert rows_mixed > 0, "no 64-row wavefront (full_blocks_kernel / capsule masks) held an open and a closed trajectory"
    assert traj_mixed > 0, "no row-per-lane wavefront held an open and a closed trajectory"
    assert traj_partial > 0, "no partly filled last row-per-lane wavefront with its last trajectory closed and an earlier one open"


@pytest.mark.parametrize("ignored", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_collision_flags_choose_the_launches_and_the_mask_pointers(ignored, decide):
    """self / env collisions ignored: the masks are skipped only when both are, the metrics take NULL for an ignored mask"""
    su = setup("panda__2cubes")
    su.bind()
    reached = REACHED.setdefault(su.name, dict(outcomes=set(), mixed_snapshot_launch=False))
    try:
        for S in (3, 9):
            x0 = starts(su, S, seed=20 + S)
            for k, modes in enumerate((patterns(S)["alternating"], patterns(S)["last_done"])):
                note(reached, gated_iteration(su, decide, x0, S, modes, params(su, self_ignored=ignored[0], env_ignored=ignored[1]), kind_shift=k))
    finally:
        su.release()


@pytest.mark.parametrize("mode", [P, D, X])
@pytest.mark.parametrize("name", ["panda__2cubes", "fetch__hello"])
def test_one_record_for_all_trajectories(name, mode, decide):
    """per_trajectory = 0, S = 3: every trajectory follows record 0 (the other modes in `modes` are never read: there is one record)"""
    su = setup(name)
    su.bind()
    try:
        x0 = starts(su, 3, seed=31)
        for kind_shift in range(4):
            gated_iteration(su, decide, x0, 3, [mode], params(su, per_trajectory=0), kind_shift=kind_shift)
    finally:
        su.release()


# ---- an anchor outside the project's own kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS + (GENERIC,))
def test_gated_iterations_against_the_fp64_oracle(name, decide):
    """S = 1: one gated pose iteration and one gated differencing iteration against the fp64 oracle, at the tolerances the ungated
    calls are held to:
      pose step + clamp       tests/test_gpu_parity.py::test_single_lm_step_matches_reference_order_oracle: |dx| < 5e-3 on the rows
                              whose scaled Jacobian has sigma_min >= 2e-2 (below that the reference's own fp32 result is noise)
      coupled step + clamp    tests/test_gpu_api.py::test_coupled_lm_step_matches_dense_reference_order_oracle: |dx| < 2e-4 + 2e-3 * step
                              (the oracle's banded solve beyond 256 waypoints: the same rows, identical in exact arithmetic)
      plan metrics            tests/test_gpu_api.py::test_plan_metrics_match_oracle, column by column"""
    su = setup(name)
    su.bind()
    rb, W, d, orc = su.rb, su.W, su.d, su.oracle
    lm = dict(lm_lambda=float(ALT_LOSS_V2_1_POSE.lm_lambda), alpha_position=float(ALT_LOSS_V2_1_POSE.alpha_position),
              alpha_rotation=float(ALT_LOSS_V2_1_POSE.alpha_rotation))  # fmt: skip
    lo, hi = H.box_corners(su.cuboids, su.Tcuboids) if len(su.cuboids) else (None, None)
    try:
        g = torch.Generator().manual_seed(77)
        x0 = (su.x_base + 3e-2 * torch.randn(su.x_base.shape, generator=g)).to(DEV).contiguous()
        x0_64 = x0.cpu().numpy().astype(np.float64)
        target_64 = su.target.cpu().numpy().astype(np.float64)
        for mode in (P, D):
            prm = params(su)
            workspace, control = rb.lm_optimize_buffers(1, W, prm, DEV)
            i32(workspace).fill_(SENTINEL)
            control[0] = mode
            control[2] = int(mode == D)
            x = x0.clone()
            rb.lm_optimize_enqueue(x, su.target, prm, workspace, control, 1)
            torch.cuda.synchronize()
            got = x.cpu().numpy().astype(np.float64)
            if mode == P:
                xo, Jo, _, fails = orc.lm_step(x0_64, target_64, solver=0, **lm)
                assert fails == 0
                ok = np.linalg.svd(Jo, compute_uv=False)[:, -1] >= 2e-2
                diff = np.abs(got - orc.clamp(xo))
                print(f"{name} pose: {ok.mean():.3f} of the rows well conditioned, max |dx| there {diff[ok].max() if ok.any() else float('nan'):.3g}")
                assert ok.any(), "no well-conditioned row: nothing was compared"
                assert diff[ok].max() < 5e-3, diff[ok].max()
            else:
                pm = ALT_LOSS_V2_1_DIFF
                want = orc.lm_full_step(x0_64, target_64, pm, 1, W, virtual_configs=x0_64, boxes_lo=lo, boxes_hi=hi, banded=W > 256)
                step = np.abs(want - x0_64).max()
                diff = np.abs(got - orc.clamp(want)).max()
                print(f"{name} differencing: step {step:.3g}, max |dx| {diff:.3g}")
                assert step > 1e-4
                assert diff < 2e-4 + 2e-3 * step, (diff, step)
            assert np.isfinite(got).all()
            L = layout(d, 1, W)
            m = workspace[L["metrics"][0] : L["metrics"][0] + 16].cpu().numpy().astype(np.float64).reshape(1, 16)
            sm = workspace.view(torch.uint8)[4 * L["self_mask"][0] :][:W].cpu().numpy()
            em = workspace.view(torch.uint8)[4 * L["env_mask"][0] :][:W].cpu().numpy()
            want_m = orc.plan_metrics(got, target_64, 1, W, sm, em)
            np.testing.assert_allclose(m[:, [0, 1]], want_m[:, [0, 1]], rtol=2e-3, atol=2e-4)
            np.testing.assert_allclose(m[:, [2, 3]], want_m[:, [2, 3]], rtol=2e-3, atol=2.6e-2)
            np.testing.assert_allclose(m[:, 4:8], want_m[:, 4:8], rtol=1e-5, atol=1e-5)
            assert np.array_equal(m[:, 8:11], want_m[:, 8:11])
            np.testing.assert_allclose(m[:, 11], want_m[:, 11], rtol=1e-6)
            assert np.all(m[:, 12:] == 0)
    finally:
        su.release()


# ---- the refusal that must come before the first launch --------------------------------------------------------------------------------
def test_unsupported_elimination_is_refused_before_anything_is_written():
    """full_rows = 0 beyond the parallel-in-time limit (pcr_max_rows = 0 puts every size beyond it): CPPF_ERR_UNSUPPORTED, and x, the
    sentinel workspace and the control block are bit for bit what they were"""
    su = setup("panda__2cubes")
    su.bind()
    rb, W = su.rb, su.W
    try:
        for S, per_traj in ((1, 0), (3, 1)):
            prm = params(su, per_trajectory=per_traj)
            x = starts(su, S, seed=5)
            x_before = x.clone()
            workspace, control = rb.lm_optimize_buffers(S, W, prm, DEV)
            i32(workspace).fill_(SENTINEL)
            control_before = control.clone()

            def refused():
                h = rb._handle(torch.device(DEV))
                rc = _hip.lib().cppf_lm_optimize_enqueue(h, x.data_ptr(), su.target.data_ptr(), S, W, ctypes.byref(prm), workspace.data_ptr(),
                                                         control.data_ptr(), 1, None)  # fmt: skip
                torch.cuda.synchronize()
                return rc

            assert run_with(rb, {"pcr_max_rows": 0, "full_rows": 0}, refused) == _hip.CPPF_ERR_UNSUPPORTED
            assert "elimination" in _hip.lib().cppf_last_error().decode()
            assert torch.equal(i32(x), i32(x_before))
            assert bool((i32(workspace) == SENTINEL).all())
            assert torch.equal(control, control_before)
    finally:
        su.release()


# ---- what the matrix reached (keep this test last) -------------------------------------------------------------------------------------
def test_the_matrix_reached_every_outcome_of_the_decision():
    """Over the module: some launch took a snapshot for one trajectory and none for another; a record ended through `stop_now`, one
    through validity + convergence, one stayed live in each of pose and differencing mode.  (Filled by the tests above: run the module
    as a whole.)"""
    assert REACHED, "the matrix tests above fill this: run the whole module"
    outcomes = set().union(*(r["outcomes"] for r in REACHED.values()))
    print({k: (sorted(v["outcomes"]), v["mixed_snapshot_launch"]) for k, v in REACHED.items()})
    assert any(r["mixed_snapshot_launch"] for r in REACHED.values()), "no launch with a snapshot for one trajectory and none for another"
    for need in ("stop_now", "valid_and_converged", "live_pose", "live_diff"):
        assert need in outcomes, (need, outcomes)
