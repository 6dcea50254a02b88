"""What the Python binding checks and allocates in front of a C-ABI call, each rule in one place: the tensor contracts (device
tensors, output buffers, rows against a target path, paths, scene cuboids), the sizes the library is asked for, the optional outputs
of a call, and the outputs of a fused launch (`cppf_lm_outputs`).  Contract violations are AssertionErrors, CPU tensors RuntimeErrors.
"""

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from cppflow_amd import _hip
from cppflow_amd.packed_rows import packed_views


def _require_device_tensor(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on '{t.device}': cppflow_amd runs on MI355X only (no CPU fallback); move the tensor to cuda"
        )
    assert t.dtype == dtype, f"{name} must be {dtype}, is {t.dtype}"
    return t if t.is_contiguous() else t.contiguous()


def _require_output_tensor(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    """A caller-supplied OUTPUT buffer: the kernel writes through its data_ptr(), so a non-contiguous tensor cannot be
    silently replaced by a contiguous copy (the caller's buffer would never be written)."""
    t = _require_device_tensor(t, name, dtype) if t.is_contiguous() else None
    assert t is not None, f"{name} is an output buffer and must be contiguous"
    return t


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def rows_tensor(x: torch.Tensor, ndof: int, name: str = "x") -> torch.Tensor:
    x = _require_device_tensor(x, name)
    assert x.dim() == 2 and x.shape[1] == ndof, f"{name} must be [n, {ndof}], is {tuple(x.shape)}"
    return x


def rows_and_target(x: torch.Tensor, target: torch.Tensor, ndof: int) -> Tuple[torch.Tensor, torch.Tensor, int, int]:
    """Rows against a target path: x [S*W, d], target [W, 7] with W > 0 -> (x, target, n = S*W, W)."""
    x, target = rows_tensor(x, ndof), _require_device_tensor(target, "target_path")
    assert target.dim() == 2 and target.shape[1] == 7 and target.shape[0] > 0 and x.shape[0] % target.shape[0] == 0, (
        f"x has {x.shape[0]} rows, not a multiple of the waypoints of a target path [W, 7] with W > 0, which is {tuple(target.shape)}"
    )
    return x, target, int(x.shape[0]), int(target.shape[0])


def paths_tensor(q: torch.Tensor, ndof: int) -> Tuple[torch.Tensor, int, int]:
    """Candidate paths q [k, T, d] -> (q, k, T)."""
    q = _require_device_tensor(q, "q")
    assert q.dim() == 3 and q.shape[2] == ndof, f"q must be [k, ntimesteps, {ndof}], is {tuple(q.shape)}"
    return q, int(q.shape[0]), int(q.shape[1])


def _scene_boxes(box_lo: torch.Tensor, box_hi: torch.Tensor, dev: torch.device, rows: str = "q"):
    """The cuboids of a device scene, world-frame corners [O, 3] on the device of the rows (`rows`: their name) -> (box_lo, box_hi, O)."""
    box_lo, box_hi = _require_device_tensor(box_lo, "box_lo"), _require_device_tensor(box_hi, "box_hi")
    assert box_lo.dim() == 2 and box_lo.shape[1] == 3 and box_hi.shape == box_lo.shape, (tuple(box_lo.shape), tuple(box_hi.shape))
    assert box_lo.device == dev and box_hi.device == dev, f"{rows}, box_lo and box_hi must be on one device"
    return box_lo, box_hi, int(box_lo.shape[0])


def _ptr(res: Dict[str, torch.Tensor], k: str) -> Optional[int]:
    """the pointer of the output res[k], or None where it was not asked for"""
    return res[k].data_ptr() if k in res else None


# ---- sizes the library is asked for, and the buffers of that size ---------------------------------------------------------------
def query_size(entry: str, *args) -> int:
    """What the `*_bytes` / `*_floats` entry point `entry` reports for `args` (its size_t out-parameter comes last)."""
    size = ctypes.c_size_t(0)
    _hip.check(getattr(_hip.lib(), entry)(*args, ctypes.byref(size)))
    return size.value


def sized_buffer(entry: str, dev: torch.device, *args) -> torch.Tensor:
    """A uint8 tensor on `dev` of as many bytes as `query_size(entry, *args)` reports: a call's workspace, a voxel map."""
    return torch.empty(query_size(entry, *args), dtype=torch.uint8, device=dev)


def optional_outputs(want: Sequence[str], spec: Dict[str, object], shape, dev: torch.device, given: Optional[Dict[str, torch.Tensor]] = None,
                     new=torch.empty) -> Dict[str, torch.Tensor]:  # fmt: skip
    """The outputs of a call that returns only what it is asked for: `spec` maps every allowed name to its dtype -- or to (dtype,
    shape) where an output does not have the common `shape` --, `want` names the ones to allocate with `new`; `given` holds the
    outputs the call has anyway."""
    assert set(want) <= set(spec), tuple(want)
    res = dict(given or {})
    for k, v in spec.items():
        if k in want and k not in res:
            dtype, shp = v if isinstance(v, tuple) else (v, shape)
            res[k] = new(shp, dtype=dtype, device=dev)
    return res


# ---- the outputs of a fused launch ------------------------------------------------------------------------------------------------
def _check_summary_buffer(t: torch.Tensor, S: int, dev) -> None:
    assert t.shape == (S, 8) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.device == dev, (
        f"summary_out must be a contiguous fp32 [{S}, 8] tensor on {dev}"
    )


def device_packed_views(packed: torch.Tensor, n: int, dev: torch.device) -> Dict[str, torch.Tensor]:
    """`packed_views` of a buffer a launch on `dev` reads or writes"""
    assert packed.is_cuda and packed.device == dev, f"the packed buffer must be on {dev}, is on {packed.device}"
    return packed_views(packed, n)


def fill_lm_outputs(out: "_hip.LmOutputs", x: torch.Tensor, W: int, x_out: torch.Tensor, packed_out: Optional[torch.Tensor] = None,
                    errors_out: Optional[Sequence[torch.Tensor]] = None,
                    summary_out: Optional[torch.Tensor] = None) -> Tuple[Dict[str, torch.Tensor], List[torch.Tensor]]:  # fmt: skip
    """Point `out` (a fresh `cppf_lm_outputs`, or the one of a batch item) at the caller's buffers of a fused launch over the rows
    x [S*W, d]: `x_out` like x, `packed_out` (packed_rows) or else `errors_out` = (pos_err_m [n], rot_err_rad [n]), `summary_out`
    [S, 8] -- every one a contiguous tensor on x's device, as the kernel writes through its pointer.  -> (the named output views, the
    tensors the holder of `out` must keep alive)."""
    n, dev = x.shape[0], x.device
    x_out = _require_output_tensor(x_out, "x_out")
    assert x_out.shape == x.shape and x_out.device == dev, f"x_out must be like x: {tuple(x.shape)} on {dev}"
    views = {"x": x_out}
    if packed_out is not None:
        views.update(device_packed_views(packed_out, n, dev))
    if errors_out is not None:
        assert packed_out is None, "packed_out already holds the pose errors"
        for k, t in zip(("pos_err_m", "rot_err_rad"), errors_out):
            views[k] = _require_output_tensor(t, k)
            assert t.numel() == n and t.device == dev, f"{k} must hold {n} values on {dev}"
    if summary_out is not None:
        _check_summary_buffer(summary_out, n // W, dev)
        views["seed_summary"] = summary_out
    for k, t in views.items():
        setattr(out, "x_out" if k == "x" else k, t.data_ptr())
    return views, list(views.values())
