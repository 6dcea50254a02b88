"""The decision function of the device-side optimiser loop (`optloop_decide`, cppflow_amd/csrc/kernels_optloop.h) compiled for the
host: the function is `__host__ __device__` without a HIP intrinsic, so the host C++ compiler builds it behind a ten-line
extern "C" shim and ctypes drives it -- no GPU, no hipcc.  Shared by tests/test_optloop_decide.py (the function against the Python
loop it restates) and tests/test_gpu_optloop_gate.py (the device's decision kernel against the function, byte for byte)."""

import ctypes
import os
import shutil
import subprocess

from cppflow_amd import _hip
from cppflow_amd import optimization as opt

CSRC = os.path.join(os.path.dirname(os.path.abspath(opt.__file__)), "csrc")

SHIM = """
#include "kernels_optloop.h"
extern "C" int shim_decide(const cppf_optloop_params* P, cppf_optloop_record* rec, const float* metrics, int G,
                           cppf_optloop_trace* tr) {
    return optloop_decide(*P, *rec, metrics, G, *tr);
}
extern "C" unsigned long shim_control_words(int S, const cppf_optloop_params* P) { return (unsigned long)optloop_control_words(S, *P); }
extern "C" int shim_sizeof(int which) {
    return which == 0 ? (int)sizeof(cppf_optloop_params) : which == 1 ? (int)sizeof(cppf_optloop_record) : (int)sizeof(cppf_optloop_trace);
}
"""


def build_shim(directory):
    """compile the shim into `directory` (a pytest tmp path) and return the loaded library with its signatures set"""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the one oracle/Makefile builds the C oracle with)"
    src, so = directory / "shim.cpp", directory / "liboptloop_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.shim_decide.restype = ctypes.c_int
    lib.shim_decide.argtypes = [ctypes.POINTER(_hip.OptloopParams), ctypes.POINTER(_hip.OptloopRecord), ctypes.c_void_p, ctypes.c_int,
                                ctypes.POINTER(_hip.OptloopTrace)]  # fmt: skip
    lib.shim_control_words.restype = ctypes.c_ulong
    lib.shim_control_words.argtypes = [ctypes.c_int, ctypes.POINTER(_hip.OptloopParams)]
    return lib
