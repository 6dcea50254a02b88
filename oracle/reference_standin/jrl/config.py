"""The two names the reference's modules take from jrl.config."""

from typing import Union

import numpy as np
import torch

DEVICE = "cpu"
PT_NP_TYPE = Union[np.ndarray, torch.Tensor]
