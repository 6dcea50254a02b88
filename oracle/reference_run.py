"""Import the reference's own cppflow modules on the CPU, without its dependencies (TEST INFRASTRUCTURE ONLY).

The reference is pure Python over `jrl` (kinematics, capsule distances) and `klampt` (meshes, drawing), neither of which is
installed.  Its cppflow-side logic -- residual stacking and row options, the LM steps, the search recurrence, the validity rules --
needs from them only a robot object and a few quaternion helpers, which oracle/reference_standin/ supplies from oracle/ref_torch.py.
`load_reference(root)` makes that logic importable and returns it; tests/golden/make_reference_runs.py records what it computes.
"""

import contextlib
import importlib
import io
import os
import sys
import types

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
STANDIN_DIR = os.path.join(_HERE, "reference_standin")
SUBMODULES = ("config", "utils", "evaluation_utils", "data_types", "collision_detection", "lm_hyper_parameters",
              "optimization_utils", "search", "optimization")  # fmt: skip


def load_reference(root: str) -> types.SimpleNamespace:
    """`root` is a checkout of the reference (the directory that holds `cppflow/`).  Returns a namespace with the imported
    submodules (`.search`, `.optimization`, `.optimization_utils`, `.evaluation_utils`, `.collision_detection`, `.data_types`,
    `.lm_hyper_parameters`, `.config`, `.utils`) and `.Robot`, the stand-in class they were imported against.

    The package's own `__init__` is skipped (it pulls in the learned IK model): `cppflow` is registered as an empty package
    whose `__path__` is the reference's directory.  Importing `cppflow.config` sets torch's default dtype and device; the default
    dtype found on entry is put back before returning, and the default device is cleared again."""
    pkg_dir = os.path.join(root, "cppflow")
    if not os.path.isfile(os.path.join(pkg_dir, "optimization_utils.py")):
        raise FileNotFoundError(f"no reference checkout at {root!r}: {pkg_dir}/optimization_utils.py does not exist")
    repo = os.path.dirname(_HERE)
    for p in (repo, STANDIN_DIR):
        if p not in sys.path:
            sys.path.insert(0, p)
    pkg = sys.modules.get("cppflow")
    if pkg is None or list(getattr(pkg, "__path__", [])) != [pkg_dir]:
        for k in [k for k in sys.modules if k == "cppflow" or k.startswith("cppflow.")]:
            del sys.modules[k]
        pkg = types.ModuleType("cppflow")
        pkg.__path__ = [pkg_dir]
        sys.modules["cppflow"] = pkg
    dtype0 = torch.get_default_dtype()
    out = types.SimpleNamespace(root=root)
    try:
        with contextlib.redirect_stdout(io.StringIO()):  # (config.py prints the device on import)
            for name in SUBMODULES:
                setattr(out, name, importlib.import_module(f"cppflow.{name}"))
    finally:
        torch.set_default_dtype(dtype0)
        torch.set_default_device(None)  # (config.py asked for "cpu", which is what no default device means)
    from jrl.robot import Robot

    out.Robot = Robot
    return out
