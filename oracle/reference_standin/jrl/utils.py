"""The helpers the reference's modules take from jrl.utils."""

import os

import torch

from jrl.config import DEVICE


def safe_mkdir(dir_name: str) -> None:
    os.makedirs(dir_name, exist_ok=True)


def to_torch(x, device: str = DEVICE, dtype=None) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x
    return torch.tensor(x, device=device, dtype=dtype if dtype is not None else torch.get_default_dtype())
