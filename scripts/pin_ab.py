#!/usr/bin/env python3
"""A/B of the UNPINNED coupled step across builds of the library on one box (developer tool; profiles/pin_ab.txt):

    python scripts/pin_ab.py build_var/lib_parent_a.so build_var/lib_parent_b.so [--rounds 3] [--out profiles/pin_ab.txt]

The in-tree library and the given ones alternate `--rounds` times over, each in a fresh child process.  Timed with device events,
median of 7 batches of 20 calls after a warm-up: `cppf_lm_full_step` for Panda at 1 x 256 and 1024 x 256 (smooth paths, self-collision
rows on, no obstacles), and ONE gated iteration of `cppf_lm_optimize_enqueue` at 1 x 256 with the record preset to the differencing
mode (x and the control block restored by two device copies before every iteration, inside the timed region, the same for every
build).  Only entry points every build has are called (a child binds the library itself), so a build from before the pinned entry
points runs unchanged.  Two builds of the same parent commit give the run-to-run spread the new build is held against."""

import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(lib_path: str) -> None:
    import numpy as np
    import torch

    from cppflow_amd import _hip
    from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot

    L = ctypes.CDLL(lib_path)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.cppf_robot_create.argtypes = [ctypes.POINTER(_hip.RobotDesc), ci, ctypes.POINTER(vp)]
    L.cppf_lm_full_step.argtypes = [vp, vp, vp, vp, ci, ci, ctypes.POINTER(_hip.FullParams), vp, vp, vp, vp, vp]
    L.cppf_lm_optimize_workspace_bytes.argtypes = [vp, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    L.cppf_lm_optimize_enqueue.argtypes = [vp, vp, vp, ci, ci, ctypes.POINTER(_hip.OptloopParams), vp, vp, ci, vp]
    L.cppf_forward_kinematics.argtypes = [vp, vp, ci, vp, vp]
    L.cppf_last_error.restype = ctypes.c_char_p
    ch = canonicalize(ROBOT_SPECS["panda"]())
    desc = _hip.chain_to_desc(ch)
    h = vp()
    assert L.cppf_robot_create(ctypes.byref(desc), 0, ctypes.byref(h)) == 0, L.cppf_last_error()
    dev = torch.device("cuda:0")
    d, W = ch.ndof, 256
    fp = Robot.full_params(ALT_LOSS_V2_1_DIFF)

    def inputs(S):
        rng = np.random.RandomState(S)
        base = np.clip(0.5 * rng.uniform(ch.lo, ch.hi)[None] + np.cumsum(0.01 * rng.randn(W, d), axis=0), ch.lo + 0.05, ch.hi - 0.05)
        x = np.clip(base[None] + 0.003 * rng.randn(S, W, d), ch.lo, ch.hi).reshape(S * W, d)
        xb = torch.tensor(base, dtype=torch.float32, device=dev)
        target = torch.empty((W, 7), dtype=torch.float32, device=dev)
        assert L.cppf_forward_kinematics(h, xb.data_ptr(), W, target.data_ptr(), None) == 0, L.cppf_last_error()
        return torch.tensor(x, dtype=torch.float32, device=dev), target

    def timed(fn, reps=20, batches=7):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(batches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) / reps * 1e3)
        return statistics.median(out)

    res = []
    stream = torch.cuda.current_stream().cuda_stream
    for S in (1, 1024):
        x, target = inputs(S)
        n = S * W
        blocks = torch.empty(n * (d * (d + 1) // 2 + d), dtype=torch.float32, device=dev)
        G, y, out = torch.empty(n * d * d, dtype=torch.float32, device=dev), torch.empty(n * d, dtype=torch.float32, device=dev), torch.empty_like(x)

        def step():
            rc = L.cppf_lm_full_step(h, x.data_ptr(), target.data_ptr(), None, S, W, ctypes.byref(fp), blocks.data_ptr(), G.data_ptr(),
                                     y.data_ptr(), out.data_ptr(), stream)  # fmt: skip
            assert rc == 0, L.cppf_last_error()

        res.append(timed(step))
    # one gated iteration in differencing mode
    x, target = inputs(1)
    prm = _hip.OptloopParams()
    prm.pose_lm_lambda, prm.pose_alpha_position, prm.pose_alpha_rotation = 1e-6, 3.5, 0.35
    prm.diff = fp
    prm.constraints = _hip.Constraints(0.01, 0.1, 7.0, 2.0, 0, 0)
    prm.max_n_steps, prm.return_if_valid_after_n_steps, prm.trace_capacity, prm.convergence_threshold = 1000000, -1, 0, 0.0
    nb = ctypes.c_size_t(0)
    assert L.cppf_lm_optimize_workspace_bytes(h, 1, W, ctypes.byref(nb)) == 0
    workspace = torch.empty(nb.value // 4, dtype=torch.float32, device=dev)
    words = _hip.optloop_initial_control(1, 0)
    words[0], words[2] = _hip.OPT_MODE_DIFF, 1
    control0 = torch.from_numpy(words).to(dev)
    control, x0 = control0.clone(), x.clone()

    def iteration():
        x.copy_(x0)
        control.copy_(control0)
        rc = L.cppf_lm_optimize_enqueue(h, x.data_ptr(), target.data_ptr(), 1, W, ctypes.byref(prm), workspace.data_ptr(),
                                        control.data_ptr(), 1, stream)  # fmt: skip
        assert rc == 0, L.cppf_last_error()

    res.append(timed(iteration))
    assert float((x - x0).abs().max()) > 0.0, "the gated iteration did not step"
    print("RESULT %.2f %.2f %.2f" % tuple(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pin_ab.txt"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    libs = [os.path.join(ROOT, "cppflow_amd", "csrc", "libcppflow_hip.so")] + [os.path.abspath(p) for p in a.libs]
    lines = ["# scripts/pin_ab.py: us per call, device events, median of 7 x 20 calls; builds alternate, one fresh process each",
             f"{'build':44s} {'step 1x256':>11s} {'step 1024x256':>14s} {'gated iteration 1x256':>22s}"]  # fmt: skip
    print("\n".join(lines), flush=True)
    for _ in range(a.rounds):
        for lib in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib], capture_output=True, text=True, timeout=300)
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
            if r.returncode != 0 or not got:
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"the child for {lib} failed (exit {r.returncode}): stopping")
            v = [float(t) for t in got[0].split()[1:]]
            ln = f"{os.path.relpath(lib, ROOT):44s} {v[0]:11.2f} {v[1]:14.2f} {v[2]:22.2f}"
            print(ln, flush=True)
            lines.append(ln)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
