"""bench.py --dump-outputs without a GPU: which ring slot holds the last timed step (`last_step_slot` against the walk
ShardedRefiner.run_steps really takes, eager and graph-replayed), and what `dump_outputs` writes from a refiner's buffers (CPU
tensors stand in for the device ones)."""

import contextlib
import os

import numpy as np
import pytest
import torch

import bench
from cppflow_amd import distributed as D


class _Launch:
    def __init__(self, log, first_slot, steps):
        self.log, self.first_slot, self.steps = log, first_slot, steps

    def launch_on(self, stream):
        self.log.append(self.first_slot + self.steps - 1)


class _Graph:
    def __init__(self, log, last_slot):
        self.log, self.last_slot = log, last_slot

    def replay(self):
        self.log.append(self.last_slot)


def _walker(B, G, n_streams, transport, graphs):
    r = object.__new__(D.ShardedRefiner)
    r.B, r.G, r.n_streams = B, G, n_streams
    r.buckets = transport or graphs
    r.transport = object() if transport else None
    r.NBUF = n_streams * G if r.buckets else max(4, n_streams) * B
    r.step_no, r.start_bucket = 0, None
    r._on = lambda stream: contextlib.nullcontext()
    r.streams = [f"s{i}" for i in range(n_streams)]
    r.log = []  # the last ring slot each launch / replay wrote
    r.launches = [[_Launch(r.log, g * B, c + 1) for c in range(B)] for g in range(r.NBUF // B)]
    r.graphs = [_Graph(r.log, (b + 1) * G - 1) for b in range(n_streams)] if graphs else None
    r.exchange = lambda bucket: None
    return r


@pytest.mark.parametrize("transport,graphs", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("B,G,n_streams", [(1, 1, 2), (1, 8, 4), (2, 8, 2), (8, 8, 2), (4, 32, 4)])
def test_last_step_slot_follows_the_ring_walk(B, G, n_streams, transport, graphs):
    if not (transport or graphs):
        G = B  # without buckets the ring has no bucket size of its own
    r = _walker(B, G, n_streams, transport, graphs)
    for steps in (1, 3, B, G, 2 * G + 1, 37, 200):
        for warm in (0, 5):
            r.run_steps(warm)  # the warm-up moves the ring before the region starts
            r.drain()
            start = r.step_no
            del r.log[:]
            r.run_steps(steps)
            r.drain()
            assert bench.last_step_slot(r, start, steps) == r.log[-1], (steps, warm, start)


def _refiner(S, W, d, collide=True, transport=False, G=1):
    n = S * W
    r = object.__new__(D.ShardedRefiner)
    r.n, r.S, r.W, r.G, r.collide = n, S, W, G, collide
    r.synchronize = lambda: None
    g = torch.Generator().manual_seed(0)
    r.x_outs = [torch.rand((n, d), generator=g) for _ in range(2)]
    if collide:
        packed = []
        for _ in range(2):
            f = torch.rand(3 * n, generator=g)
            m = (torch.rand(3 * n, generator=g) < 0.5).to(torch.uint8)
            packed.append(torch.cat([f.view(torch.uint8), m]))
        r.packeds, r.summ_all = packed, torch.rand((2, S, 8), generator=g)
    else:
        r.errs = [(torch.rand(n, generator=g), torch.rand(n, generator=g)) for _ in range(2)]
    r.selected = [torch.arange(4 * G, dtype=torch.int32).view(G, 4) + 100 * b for b in range(2)] if transport else None
    return r


def _load(dir_):
    return {f[:-4]: np.load(os.path.join(dir_, f)) for f in sorted(os.listdir(dir_))}


def test_dump_writes_the_slot_s_arrays_as_a_caller_receives_them(tmp_path):
    r = _refiner(S=4, W=6, d=7, transport=True, G=2)
    bench.dump_outputs(r, 1, str(tmp_path), rank=0, world=1)
    out = _load(tmp_path)
    assert sorted(out) == ["env_mask", "ext_cost", "jlim_mask", "pos_err_m", "rot_err_rad", "seed_summary", "selected_seed", "self_mask", "x"]
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    np.testing.assert_array_equal(out["x"], r.x_outs[1].numpy())
    cost, pe, re, sm, em, jm = D.unpack_rows(r.packeds[1], r.n)
    for name, t in (("ext_cost", cost), ("pos_err_m", pe), ("rot_err_rad", re), ("self_mask", sm), ("env_mask", em), ("jlim_mask", jm)):
        np.testing.assert_array_equal(out[name], t.numpy().astype(np.float32))
    np.testing.assert_array_equal(out["seed_summary"], r.summ_all[1].numpy())
    np.testing.assert_array_equal(out["selected_seed"], r.selected[0][1].numpy().astype(np.float64))  # slot 1 = bucket 0, row 1


def test_dump_without_collision_and_per_rank_names(tmp_path):
    r = _refiner(S=2, W=3, d=9, collide=False)
    bench.dump_outputs(r, 0, str(tmp_path), rank=3, world=4)
    out = _load(tmp_path)
    assert sorted(out) == ["pos_err_m_rank3", "rot_err_rad_rank3", "x_rank3"]
    np.testing.assert_array_equal(out["pos_err_m_rank3"], r.errs[0][0].numpy())


def test_dump_over_budget_keeps_a_fixed_sample_of_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    r = _refiner(S=16, W=32, d=7)
    for sub in ("a", "b"):
        bench.dump_outputs(r, 0, str(tmp_path / sub), rank=0, world=1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= 4096
    keep = a["sampled_rows"].astype(np.int64)
    assert 0 < len(keep) < r.n and np.all(np.diff(keep) > 0)
    np.testing.assert_array_equal(a["x"], r.x_outs[0].numpy()[keep])
    for k in a:  # the same rows every time
        np.testing.assert_array_equal(a[k], b[k])
