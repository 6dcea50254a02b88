"""Reading (and packing) tests/golden/reference_runs_<robot>.npz: runs of the reference's own cppflow code, recorded as data by
tests/golden/make_reference_runs.py.  Shared by the CPU tests (tests/test_reference_runs.py), the GPU tests
(tests/test_gpu_reference_runs.py) and the generator; it needs neither the reference nor a GPU.

A robot's file holds some three hundred small arrays.  As separate members of the archive their headers alone would outweigh the
data, so they are packed: one flat array per element type plus a directory (name, type, shape, offset).  `load(name)` gives back
the {key: array} dictionary the generator produced, bit for bit, read-only.  Keys are "<section>__<field>" or
"step_<family>__s<trajectory>__<field>"; inputs recorded as float16 are exactly representable in fp32 and fp64 too.
"""

import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROBOTS = ("panda", "fetch", "fetch_arm")
_KINDS = ("float64", "float32", "float16", "int32", "uint8", "bool")
_STORE = {"float64": "float64", "float32": "float32", "float16": "float16", "int32": "int32", "uint8": "uint8", "bool": "uint8"}
_MAX_DIMS = 4

# the fields of OptimizationParameters a coupled-step case records, in the order of its `params` vector (NaN = None)
PARAM_NAMES = (
    "lm_lambda", "alpha_position", "alpha_rotation", "alpha_differencing", "alpha_differencing_prismatic_scaling",
    "alpha_virtual_configs", "alpha_self_collision", "alpha_env_collision", "use_pose", "pose_do_scale_down_satisfied",
    "pose_ignore_satisfied_threshold_scale", "pose_ignore_satisfied_scale_down", "use_differencing",
    "differencing_do_ignore_satisfied", "differencing_ignore_satisfied_margin_deg", "differencing_ignore_satisfied_margin_cm",
    "differencing_do_scale_satisfied", "differencing_scale_down_satisfied_scale",
    "differencing_scale_down_satisfied_shift_invalid_to_threshold", "use_virtual_configs", "n_virtual_configs",
    "use_self_collisions", "use_env_collisions",
)  # fmt: skip
_BOOL_PARAMS = {k for k in PARAM_NAMES if k.startswith("use_") or "_do_" in k or k.endswith("shift_invalid_to_threshold")}
BLOCKS = ("pose", "differencing", "virtual_configs", "self_collisions", "env_collisions")
STEP_FAMILIES = ("pose_plain", "diff_plain", "pose_scale", "diff_scale_shift", "diff_scale_noshift", "diff_filter", "virtual_configs",
                 "self_collision", "env_collision_1", "env_collision_2", "everything")  # fmt: skip
DP_CASES = ((1, 4), (5, 9), (64, 7), (65, 2), (40, 12), (97, 33), (257, 5))


def pack(arrays):
    """{key: array} -> the few arrays that are written to the .npz"""
    names, kinds, shapes, offsets = [], [], [], []
    blobs = {k: [] for k in _KINDS if k != "bool"}
    fill = {k: 0 for k in blobs}
    for key, a in arrays.items():
        a = np.asarray(a)
        if a.dtype == np.int64:
            assert np.abs(a).max(initial=0) < 2**31, key
            a = a.astype(np.int32)
        kind = str(a.dtype)
        assert kind in _KINDS and a.ndim <= _MAX_DIMS, (key, kind, a.shape)
        store = _STORE[kind]
        names.append(key), kinds.append(_KINDS.index(kind)), offsets.append(fill[store])
        shapes.append(list(a.shape) + [-1] * (_MAX_DIMS - a.ndim))
        blobs[store].append(a.astype(store).reshape(-1))
        fill[store] += a.size
    out = {"names": np.array(names, dtype="S"), "kinds": np.array(kinds, dtype=np.uint8), "shapes": np.array(shapes, dtype=np.int32),
           "offsets": np.array(offsets, dtype=np.int64)}  # fmt: skip
    for k, parts in blobs.items():
        out[f"data_{k}"] = np.concatenate(parts) if parts else np.zeros(0, dtype=k)
    return out


def unpack(z):
    out = {}
    for name, kind, shape, off in zip(z["names"], z["kinds"], z["shapes"], z["offsets"]):
        kind = _KINDS[int(kind)]
        shape = tuple(int(v) for v in shape if v >= 0)
        n = int(np.prod(shape, dtype=np.int64))
        a = np.array(z[f"data_{_STORE[kind]}"][int(off) : int(off) + n]).astype(kind).reshape(shape)
        a.setflags(write=False)
        out[name.decode()] = a
    return out


def fixture_path(name):
    return os.path.join(GOLDEN, f"reference_runs_{name}.npz")


@functools.lru_cache(maxsize=None)
def load(name):
    """The recorded runs of one robot: {key: read-only array}"""
    with np.load(fixture_path(name), allow_pickle=False) as z:
        return unpack({k: z[k] for k in z.files})


def section(runs, prefix):
    """{field: array} of the keys "<prefix>__<field>" """
    p = prefix + "__"
    return {k[len(p) :]: v for k, v in runs.items() if k.startswith(p)}


def params_dict(values):
    """the recorded `params` vector -> keyword arguments of an OptimizationParameters (virtual_configs left to the caller)"""
    d = {}
    for k, v in zip(PARAM_NAMES, values):
        if np.isnan(v):
            d[k] = None
        elif k in _BOOL_PARAMS:
            d[k] = bool(v)
        elif k == "n_virtual_configs":
            d[k] = int(v)
        else:
            d[k] = float(v)
    d["seed_w_only_pose"] = None
    return d


def project_params(values, virtual_configs=None):
    """cppflow_amd's OptimizationParameters for a recorded case"""
    import warnings

    from cppflow_amd.lm_hyper_parameters import OptimizationParameters

    import torch

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return OptimizationParameters(virtual_configs=torch.tensor([]) if virtual_configs is None else virtual_configs, **params_dict(values))


def project_constraints(values):
    from cppflow_amd.data_types import Constraints

    return Constraints(*[float(v) for v in values])
