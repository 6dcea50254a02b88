#!/usr/bin/env python3
"""The coupled LM step on a whole obstacle scene (cppf_lm_full_step_scene): what it costs, and what the planner does with it
(developer tool; profiles/scene_step.txt):

    python scripts/scene_step_bench.py build_var/lib_parent_a.so build_var/lib_parent_b.so [--rounds 3] [--out profiles/scene_step.txt]

Every number is us per call from device events: median of 7 batches of 200 calls after a warm-up, one fresh child process per
measurement set, the median over `--rounds` such processes.  Panda, 1 x 256 and 8 x 256 rows (smooth paths with 0.003 rad of noise,
ALT_LOSS_V2_1_DIFF, virtual_configs = x).
  (a) the scene step on a scene of the 8 cuboids the handle holds, beside the existing step on that handle: the cost of the form.
  (b) the scene step on 64 and 1024 cuboids, "near" clutter (centres 0.30 .. 0.95 m from the base axis, the robot's workspace) and
      "far" clutter (1.5 .. 2.5 m: every tile is culled).
  (c) the plain cppf_lm_full_step (no obstacles) of this build against the given builds of the parent commit, alternating, each in a
      fresh process (as scripts/pin_ab.py does): two builds of the same parent give the run-to-run spread the new build is held against.
  (d) CppFlowPlanner with scene_optimizer off / on on the cube of panda__1cube_mini cut into 3 x 3 x 3 and 5 x 5 x 5 pieces: validity,
      LM steps, selection rounds, env-colliding waypoints."""

import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = 256
SIZES = (1, 8)


def _inputs(ch, S, dev):
    import numpy as np
    import torch

    d = ch.ndof
    rng = np.random.RandomState(S)
    base = np.clip(0.5 * rng.uniform(ch.lo, ch.hi)[None] + np.cumsum(0.01 * rng.randn(W, d), axis=0), ch.lo + 0.05, ch.hi - 0.05)
    x = np.clip(base[None] + 0.003 * rng.randn(S, W, d), ch.lo, ch.hi).reshape(S * W, d)
    return torch.tensor(x, dtype=torch.float32, device=dev), torch.tensor(base, dtype=torch.float32, device=dev)


def _timed(fn, reps=200, batches=7):
    import torch

    for _ in range(20):
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


def child_ab(lib_path: str) -> None:
    """(c): cppf_lm_full_step of ANY build (the child binds the library itself; only entry points every build has)"""
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
    L.cppf_forward_kinematics.argtypes = [vp, vp, ci, vp, vp]
    L.cppf_last_error.restype = ctypes.c_char_p
    ch = canonicalize(ROBOT_SPECS["panda"]())
    desc = _hip.chain_to_desc(ch)
    h = vp()
    assert L.cppf_robot_create(ctypes.byref(desc), 0, ctypes.byref(h)) == 0, L.cppf_last_error()
    dev = torch.device("cuda:0")
    d = ch.ndof
    fp = Robot.full_params(ALT_LOSS_V2_1_DIFF)
    stream = torch.cuda.current_stream().cuda_stream
    res = []
    for S in SIZES:
        x, xb = _inputs(ch, S, dev)
        target = torch.empty((W, 7), dtype=torch.float32, device=dev)
        assert L.cppf_forward_kinematics(h, xb.data_ptr(), W, target.data_ptr(), None) == 0, L.cppf_last_error()
        n = S * W
        blocks = torch.empty(n * (d * (d + 1) // 2 + d), dtype=torch.float32, device=dev)
        G, y, out = torch.empty(n * d * d, dtype=torch.float32, device=dev), torch.empty(n * d, dtype=torch.float32, device=dev), torch.empty_like(x)

        def step():
            rc = L.cppf_lm_full_step(h, x.data_ptr(), target.data_ptr(), x.data_ptr(), S, W, ctypes.byref(fp), blocks.data_ptr(), G.data_ptr(),
                                     y.data_ptr(), out.data_ptr(), stream)  # fmt: skip
            assert rc == 0, L.cppf_last_error()

        res.append(_timed(step))
    print("RESULT " + " ".join(f"{v:.2f}" for v in res))


def _polar_corners(radii, n, seed):
    import numpy as np

    g = np.random.default_rng(seed)
    r, a, z = g.uniform(*radii, n), g.uniform(0, 2 * np.pi, n), g.uniform(0, 1.3, n)
    half = g.uniform(0.02, 0.06, (n, 3))
    c = np.stack([r * np.cos(a), r * np.sin(a), z], axis=1)
    return (c - half).astype(np.float32), (c + half).astype(np.float32)


def child_scene() -> None:
    """(a) and (b), on the in-tree library through the C ABI (buffers allocated once, outside the timed region)"""
    import numpy as np
    import torch

    from cppflow_amd import _hip
    from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF
    from cppflow_amd.robots import get_robot

    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    rb = get_robot("panda")
    ch = canonicalize(ROBOT_SPECS["panda"]())
    dev = torch.device("cuda:0")
    d, L = ch.ndof, _hip.lib()
    fp = rb.full_params(ALT_LOSS_V2_1_DIFF)
    stream = torch.cuda.current_stream().cuda_stream
    lo8, hi8 = _polar_corners((0.30, 0.95), 8, 0)
    cuboids = [np.concatenate([-(h - l) / 2, (h - l) / 2]).astype(np.float32) for l, h in zip(lo8, hi8)]
    Ts = []
    for l, h in zip(lo8, hi8):
        T = np.zeros((4, 4), dtype=np.float32)
        T[:3, :3] = np.eye(3)
        T[:3, 3] = (l + h) / 2
        Ts.append(T)
    rb.set_obstacles(cuboids, Ts)
    # the scene of "the same 8": the corners exactly as the handle forms them (translation + local corner in fp32)
    lo_same = np.stack([T[:3, 3] + c[:3] for c, T in zip(cuboids, Ts)]).astype(np.float32)
    hi_same = np.stack([T[:3, 3] + c[3:] for c, T in zip(cuboids, Ts)]).astype(np.float32)
    scenes = {"same8": (lo_same, hi_same)}
    for O in (64, 1024):
        scenes[f"near{O}"] = _polar_corners((0.30, 0.95), O, 1)
        scenes[f"far{O}"] = _polar_corners((1.5, 2.5), O, 2)
    res = {}
    for S in SIZES:
        x, xb = _inputs(ch, S, dev)
        target = rb.forward_kinematics(xb).contiguous()
        n = S * W
        blocks = torch.empty(n * (d * (d + 1) // 2 + d), dtype=torch.float32, device=dev)
        G, y = torch.empty(n * d * d, dtype=torch.float32, device=dev), torch.empty(n * d, dtype=torch.float32, device=dev)
        out, ref = torch.empty_like(x), torch.empty_like(x)
        h = rb._handle(dev)

        def handle_step(dst=out):
            _hip.check(L.cppf_lm_full_step_pinned(h, x.data_ptr(), target.data_ptr(), x.data_ptr(), S, W, ctypes.byref(fp), 0, blocks.data_ptr(),
                                                  G.data_ptr(), y.data_ptr(), dst.data_ptr(), stream))  # fmt: skip

        res[(S, "handle8")] = _timed(handle_step)
        handle_step(ref)
        for tag, (lo, hi) in scenes.items():
            lod, hid = torch.tensor(lo, device=dev), torch.tensor(hi, device=dev)

            def scene_step():
                _hip.check(L.cppf_lm_full_step_scene(h, x.data_ptr(), target.data_ptr(), x.data_ptr(), S, W, ctypes.byref(fp), 0, lod.data_ptr(),
                                                     hid.data_ptr(), lo.shape[0], blocks.data_ptr(), G.data_ptr(), y.data_ptr(), out.data_ptr(),
                                                     stream))  # fmt: skip

            res[(S, tag)] = _timed(scene_step)
            torch.cuda.synchronize()
            if tag == "same8":  # (what is timed is the same computation: the same bits)
                assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), "the scene step on the handle's cuboids differs from the handle's step"
    rb.set_obstacles([], [])
    tags = ["handle8"] + list(scenes)
    print("TAGS " + " ".join(tags))
    for S in SIZES:
        print(f"RESULT {S} " + " ".join(f"{res[(S, t)]:.2f}" for t in tags))


def child_planner() -> None:
    """(d)"""
    import dataclasses

    import numpy as np
    import torch

    from cppflow_amd.data_type_utils import problem_from_filename
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, TrackingSeedProvider

    ref = os.path.join(ROOT, "tests", "golden", "reference_files")
    base = problem_from_filename(None, "panda__1cube_mini", problems_dir=os.path.join(ref, "problems"), paths_dir=os.path.join(ref, "paths"),
                                 device="cuda:0")  # fmt: skip
    c, T = base.obstacles_cuboids[0].cpu().numpy().astype(np.float64), base.obstacles_Tcuboids[0].cpu().numpy().astype(np.float64)
    size = c[3:] - c[:3]
    for k in (3, 5):
        cub, Ts = [], []
        for i in range(k):
            for j in range(k):
                for l in range(k):
                    centre = T[:3, 3] + c[:3] + (np.array([i, j, l]) + 0.5) * size / k
                    s = (size / k).astype(np.float32)
                    cub.append(torch.tensor(np.concatenate([-s / 2, s / 2]).astype(np.float32)))
                    Tm = np.zeros((4, 4), dtype=np.float32)
                    Tm[:3, :3] = np.eye(3)
                    Tm[:3, 3] = centre
                    Ts.append(torch.tensor(Tm))
        for on in (False, True):
            problem = dataclasses.replace(base, obstacles_cuboids=cub, obstacles_Tcuboids=Ts, active_obstacles=None)
            settings = PlannerSettings(k=175, tmax_sec=60.0, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=False,
                                       do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip
            res = CppFlowPlanner(settings, problem.robot, seed_provider=TrackingSeedProvider(seed=0), scene_optimizer=on).generate_plan(problem)
            di = res.debug_info
            print(f"PLAN {k}x{k}x{k} ({k**3} cuboids) scene_optimizer={str(on):5s} is_valid={str(bool(res.plan.is_valid)):5s} "
                  f"LM steps={di.get('n_optimization_steps')} selection rounds={di.get('scene_selection_rounds')} "
                  f"active={di.get('active_obstacles')} env-colliding waypoints={int(res.plan.env_colliding_per_ts.sum())}")  # fmt: skip


def _run_child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
        raise SystemExit(f"the child {args} failed (exit {r.returncode}): stopping")
    return r.stdout.splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_step.txt"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.child == "ab":
        return child_ab(a.lib)
    if a.child == "scene":
        return child_scene()
    if a.child == "planner":
        return child_planner()
    lines = ["# scripts/scene_step_bench.py: Panda, us per call, device events, median of 7 x 200 calls per process; one fresh process per line"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# (a) / (b): the existing step on a handle of 8 cuboids | the scene step on the same 8 | on 64 / 1024 cuboids near and far")
    per = {}
    tags = None
    for _ in range(a.rounds):
        out = _run_child(["--child", "scene"])
        tags = [ln for ln in out if ln.startswith("TAGS")][0].split()[1:]
        for ln in out:
            if ln.startswith("RESULT"):
                t = ln.split()
                per.setdefault(int(t[1]), []).append([float(v) for v in t[2:]])
    say(f"{'rows':>8s} " + " ".join(f"{t:>9s}" for t in tags) + "    (median over processes; min .. max of the first two columns)")
    for S, runs in per.items():
        med = [statistics.median(col) for col in zip(*runs)]
        spread = " ".join(f"[{min(col):.2f} .. {max(col):.2f}]" for col in list(zip(*runs))[:2])
        say(f"{S:>3d}x{W:<4d} " + " ".join(f"{v:9.2f}" for v in med) + "    " + spread)

    say("# (c): plain cppf_lm_full_step, no obstacles: this build and builds of the parent commit, alternating")
    libs = [os.path.join(ROOT, "cppflow_amd", "csrc", "libcppflow_hip.so")] + [os.path.abspath(p) for p in a.libs]
    say(f"{'build':44s} " + " ".join(f"{f'step {S}x{W}':>12s}" for S in SIZES))
    ab = {lib: [] for lib in libs}
    for _ in range(a.rounds):
        for lib in libs:
            out = _run_child(["--child", "ab", "--lib", lib])
            v = [float(t) for t in [ln for ln in out if ln.startswith("RESULT")][0].split()[1:]]
            ab[lib].append(v)
            say(f"{os.path.relpath(lib, ROOT):44s} " + " ".join(f"{x:12.2f}" for x in v))
    for lib in libs:
        cols = list(zip(*ab[lib]))
        say(f"median {os.path.relpath(lib, ROOT):37s} " + " ".join(f"{statistics.median(c):12.2f}" for c in cols) +
            "   min .. max " + " ".join(f"[{min(c):.2f} .. {max(c):.2f}]" for c in cols))  # fmt: skip
    if len(libs) > 1:
        parent = [list(zip(*ab[lib])) for lib in libs[1:]]
        for i, S in enumerate(SIZES):
            pv = [v for p in parent for v in p[i]]
            new = statistics.median(list(zip(*ab[libs[0]]))[i])
            verdict = "within" if min(pv) <= new <= max(pv) else ("below" if new < min(pv) else "ABOVE")
            say(f"step {S}x{W}: this build's median {new:.2f} us is {verdict} the parent builds' own range [{min(pv):.2f} .. {max(pv):.2f}] us")

    say("# (d): CppFlowPlanner on the cube of panda__1cube_mini cut into pieces (k = 175 candidates, TrackingSeedProvider(seed=0))")
    for ln in _run_child(["--child", "planner"]):
        if ln.startswith("PLAN"):
            say(ln[5:])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
