#!/usr/bin/env python3
"""Bit identity of the coupled step across builds of the library on one box (developer tool; profiles/coupled_fold_bits.txt):

    python scripts/coupled_bits_ab.py build_var/lib_parent.so [--out profiles/coupled_fold_bits.txt]

The in-tree library and the given one each run the same case matrix on the same seeded inputs, one fresh child process per
(library, robot) under its own time limit; a child binds its library with ctypes and calls only entry points both builds have.  A child
prints one SHA-256 per case: of x_out's bytes, or of the return code and message where the step is refused.  The parent compares
case by case, stops at the first failing child and exits non-zero on any difference.

Cases (every elimination form, small shapes): Panda, Fetch (prismatic joint), a generic 3-joint chain and chain12; S in {1, 9} x
W in {1, 2, 3, 25, 59, 257}; pin 0 .. 3; tuning default, pcr_lds 0 .. 3, pcr_max_rows = 0 (rows), pcr_max_rows = 0 with full_rows = 0
(one wavefront per trajectory up to 8 joints, which refuses a pin; one lane at chain12), pose block on (one lane), differencing_mode
1 and 2 (individually weighted rows, pin 0); virtual configurations off / given / on with a NULL pointer (W >= 3).  Self- and
environment-collision rows are on with a cuboid 2 cm from the tool of the path's middle waypoint; one revolute joint jumps from +3.1 to
-3.1 rad between two waypoints (the wrap).  Then one gated iteration of cppf_lm_optimize_enqueue in the differencing mode, x digested.
The table has one line per (robot, form, S, W): the number of (pin, virtual-config) cases, how many were refused, how many differ,
and the first 64 bits of one SHA-256 over their digests."""

import argparse
import ctypes
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROBOTS = ("panda", "fetch", "generic3", "chain12")
SHAPES = [(S, W) for S in (1, 9) for W in (1, 2, 3, 25, 59, 257)]
# name -> (tuning, parameter overrides, pins)
FORMS = {
    "default": ({}, {}, (0, 1, 2, 3)),
    "pcr_lds0": ({"pcr_lds": 0}, {}, (0, 1, 2, 3)),
    "pcr_lds1": ({"pcr_lds": 1}, {}, (0, 1, 2, 3)),
    "pcr_lds2": ({"pcr_lds": 2}, {}, (0, 1, 2, 3)),
    "pcr_lds3": ({"pcr_lds": 3}, {}, (0, 1, 2, 3)),
    "rows": ({"pcr_max_rows": 0}, {}, (0, 1, 2, 3)),
    "wave_or_lane": ({"pcr_max_rows": 0, "full_rows": 0}, {}, (0, 1, 2, 3)),
    "pose": ({}, {"use_pose": 1}, (0, 1, 2, 3)),
    "diff_mode1": ({}, {"differencing_mode": 1}, (0,)),
    "diff_mode2": ({}, {"differencing_mode": 2, "differencing_shift_invalid_to_threshold": 1}, (0,)),
}
VQ = ("off", "given", "null")


def child(lib_path: str, name: str) -> None:
    import numpy as np
    import torch

    from cppflow_amd import _hip
    from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot
    from tests import helpers as H

    L = ctypes.CDLL(lib_path)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    fpp = ctypes.POINTER(ctypes.c_float)
    L.cppf_robot_create.argtypes = [ctypes.POINTER(_hip.RobotDesc), ci, ctypes.POINTER(vp)]
    L.cppf_debug_set.argtypes = [vp, ci, ci]
    L.cppf_set_obstacles.argtypes = [vp, ci, fpp, fpp]
    L.cppf_forward_kinematics.argtypes = [vp, vp, ci, vp, vp]
    L.cppf_collision_masks.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    L.cppf_lm_full_step_pinned.argtypes = [vp, vp, vp, vp, ci, ci, ctypes.POINTER(_hip.FullParams), ci, vp, vp, vp, vp, vp]
    L.cppf_lm_optimize_workspace_bytes.argtypes = [vp, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    L.cppf_lm_optimize_enqueue.argtypes = [vp, vp, vp, ci, ci, ctypes.POINTER(_hip.OptloopParams), vp, vp, ci, vp]
    L.cppf_last_error.restype = ctypes.c_char_p
    spec = H.random_chain_spec(3, seed=11, n_prismatic=0) if name == "generic3" else ROBOT_SPECS[name]()
    ch = canonicalize(spec)
    desc = _hip.chain_to_desc(ch)
    h = vp()
    assert L.cppf_robot_create(ctypes.byref(desc), 0, ctypes.byref(h)) == 0, L.cppf_last_error()
    dev = torch.device("cuda:0")
    d = ch.ndof
    stream = torch.cuda.current_stream().cuda_stream
    wrap_joint = max(j for j in range(d) if ch.jtype[j] == 0)  # the last revolute joint

    def inputs(S, W):
        rng = np.random.RandomState(1000 * S + W)
        base = np.clip(0.5 * rng.uniform(ch.lo, ch.hi)[None] + np.cumsum(0.01 * rng.randn(W, d), axis=0), ch.lo + 0.05, ch.hi - 0.05)
        x = np.clip(base[None] + 0.003 * rng.randn(S, W, d), ch.lo, ch.hi)
        if W >= 2:  # the wrap: +3.1 -> -3.1 is a joint change of 2 pi - 6.2 = +0.083 rad
            tw = (W - 1) // 2
            x[:, tw, wrap_joint] = 3.1 + 0.003 * rng.randn(S)
            x[:, tw + 1, wrap_joint] = -3.1 + 0.003 * rng.randn(S)
        xv = x + 0.02 * rng.randn(S, W, d)
        xb = torch.tensor(base, dtype=torch.float32, device=dev)
        target = torch.empty((W, 7), dtype=torch.float32, device=dev)
        assert L.cppf_forward_kinematics(h, xb.data_ptr(), W, target.data_ptr(), None) == 0, L.cppf_last_error()
        x = torch.tensor(x.reshape(S * W, d), dtype=torch.float32, device=dev)
        return x, torch.tensor(xv.reshape(S * W, d), dtype=torch.float32, device=dev), target

    def obstacle_at(target):
        """one 0.3 m cube with a face 2 cm from the tool position of the path's middle waypoint, bound to the handle: along the path
        the tool's capsules graze it, enter it and leave it"""
        p = target[target.shape[0] // 2, :3].cpu().numpy().astype(np.float32) + np.array([0.17, 0.0, 0.0], dtype=np.float32)
        cub = np.array([[-0.15, -0.15, -0.15, 0.15, 0.15, 0.15]], dtype=np.float32)
        rt = np.zeros((1, 12), dtype=np.float32)
        rt[0, :9] = np.eye(3, dtype=np.float32).reshape(9)
        rt[0, 9:] = p
        assert L.cppf_set_obstacles(h, 1, _hip.fptr(cub), _hip.fptr(rt)) == 0, L.cppf_last_error()

    def tune(settings):
        for key in ("pcr_max_rows", "full_rows", "pcr_lds"):
            assert L.cppf_debug_set(h, _hip.TUNE_KEYS[key], settings.get(key, _hip.TUNE_DEFAULT)) == 0, L.cppf_last_error()

    def sha(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    colliding = 0
    for S, W in SHAPES:
        x, xv, target = inputs(S, W)
        obstacle_at(target)
        n = S * W
        sm, em = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        assert L.cppf_collision_masks(h, x.data_ptr(), S, W, sm.data_ptr(), em.data_ptr(), None, None, None, None, stream) == 0, L.cppf_last_error()  # fmt: skip
        colliding += int((sm | em).sum())
        blocks = torch.zeros(n * (d * (d + 1) // 2 + d), dtype=torch.float32, device=dev)
        G, y = torch.zeros(n * d * d, dtype=torch.float32, device=dev), torch.zeros(n * d, dtype=torch.float32, device=dev)
        for form, (settings, over, pins) in FORMS.items():
            tune(settings)
            for vq in VQ if W >= 3 else VQ[:1]:
                fp = Robot.full_params(ALT_LOSS_V2_1_DIFF)
                fp.use_self_collisions = fp.use_env_collisions = 1
                fp.alpha_differencing_prismatic_scaling = 3.0  # (1 in the preset: Fetch's torso joint would not show it)
                fp.alpha_position, fp.alpha_rotation = fp.alpha_position or 3.5, fp.alpha_rotation or 0.35
                fp.differencing_threshold_rad, fp.differencing_threshold_m, fp.differencing_scale_down = 0.01, 0.005, 0.1
                fp.use_virtual_configs = int(vq != "off")
                fp.n_virtual_configs = min(max(fp.n_virtual_configs, 1), (W - 1) // 2) if vq != "off" else 0
                for k, v in over.items():
                    setattr(fp, k, v)
                for pin in pins:
                    out = torch.full_like(x, float("nan"))
                    rc = L.cppf_lm_full_step_pinned(h, x.data_ptr(), target.data_ptr(), xv.data_ptr() if vq == "given" else None, S, W,
                                                    ctypes.byref(fp), pin, blocks.data_ptr(), G.data_ptr(), y.data_ptr(),
                                                    out.data_ptr(), stream)  # fmt: skip
                    dig = sha(out) if rc == 0 else "refused:" + hashlib.sha256(b"%d " % rc + L.cppf_last_error()).hexdigest()
                    print(f"CASE {name} {form} {S} {W} pin={pin} vq={vq} {dig}", flush=True)
    tune({})
    print(f"COLLIDING {name} {colliding}", flush=True)
    if d < 6:  # the device loop's pose step needs 6 joints
        return
    # one gated iteration of the device loop in the differencing mode
    for S, W in ((1, 59), (9, 25), (1, 256)):
        x, _, target = inputs(S, W)
        obstacle_at(target)
        prm = _hip.OptloopParams()
        prm.pose_lm_lambda, prm.pose_alpha_position, prm.pose_alpha_rotation = 1e-6, 3.5, 0.35
        prm.diff = Robot.full_params(ALT_LOSS_V2_1_DIFF)
        prm.constraints = _hip.Constraints(0.01, 0.1, 7.0, 2.0, 0, 0)
        prm.max_n_steps, prm.return_if_valid_after_n_steps, prm.trace_capacity, prm.convergence_threshold = 1000000, -1, 0, 0.0
        nb = ctypes.c_size_t(0)
        assert L.cppf_lm_optimize_workspace_bytes(h, S, W, ctypes.byref(nb)) == 0, L.cppf_last_error()
        workspace = torch.zeros(nb.value // 4, dtype=torch.float32, device=dev)
        words = _hip.optloop_initial_control(1, 0)
        words[0], words[2] = _hip.OPT_MODE_DIFF, 1
        control = torch.from_numpy(words).to(dev)
        x0 = x.clone()
        rc = L.cppf_lm_optimize_enqueue(h, x.data_ptr(), target.data_ptr(), S, W, ctypes.byref(prm), workspace.data_ptr(),
                                        control.data_ptr(), 1, stream)  # fmt: skip
        assert rc == 0, L.cppf_last_error()
        dig = sha(x)
        assert float((x - x0).abs().max()) > 0.0, "the gated iteration did not step"
        print(f"CASE {name} optloop {S} {W} pin=0 vq=preset {dig}", flush=True)


def run_child(lib: str, name: str) -> dict:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--robot", name], capture_output=True, text=True, timeout=300)
    cases = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("CASE "):
            key, dig = ln[5:].rsplit(" ", 1)
            cases[key] = dig
        elif ln.startswith("COLLIDING "):
            cases["colliding rows " + name] = ln.split()[2]
    if r.returncode != 0 or not cases:
        print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
        raise SystemExit(f"the child for {lib} / {name} failed (exit {r.returncode}): stopping")
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coupled_fold_bits.txt"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--robot", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.robot)
    libs = [os.path.join(ROOT, "cppflow_amd", "csrc", "libcppflow_hip.so"), os.path.abspath(a.lib)]
    lines = [f"# scripts/coupled_bits_ab.py: SHA-256 over the per-case digests of x_out, {os.path.relpath(libs[0], ROOT)} against "
             f"{os.path.relpath(libs[1], ROOT)}",
             "# virtual configurations need 2 n_virtual_configs < W: the W = 1 and W = 2 shapes run with them off only",
             f"{'robot':9s} {'form':13s} {'S':>2s} {'W':>4s} {'cases':>5s} {'refused':>7s} {'differ':>6s}  digest of the in-tree build (first 64 bits)"]  # fmt: skip
    differ = []
    for name in ROBOTS:
        new, old = run_child(libs[0], name), run_child(libs[1], name)
        if new.keys() != old.keys():
            raise SystemExit(f"{name}: the two builds ran different cases")
        n_coll = new.pop("colliding rows " + name)
        assert old.pop("colliding rows " + name) == n_coll and int(n_coll) > 0, f"{name}: no colliding row in the inputs"
        groups = {}
        for key in new:
            groups.setdefault(tuple(key.split()[:4]), []).append(key)
        for (rb, form, S, W), keys in groups.items():
            bad = [k for k in keys if new[k] != old[k]]
            differ += bad
            dig = hashlib.sha256(" ".join(new[k] for k in keys).encode()).hexdigest()
            n_ref = sum(new[k].startswith("refused:") for k in keys)
            lines.append(f"{rb:9s} {form:13s} {S:>2s} {W:>4s} {len(keys):5d} {n_ref:7d} {len(bad):6d}  {dig[:16]}")
        lines.append(f"# {name}: {len(new)} cases, {n_coll} input rows with a colliding pair or capsule (summed over the shapes)")
        print("\n".join(lines[-len(groups) - 1:]), flush=True)
    lines.append(f"# {len(differ)} cases differ" + "".join("\n#   " + k for k in differ))
    print(lines[-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
