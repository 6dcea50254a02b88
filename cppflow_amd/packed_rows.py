"""The packed per-row output buffer of a fused launch: the one buffer one all-gather ships to every rank.

For n rows: ext_cost | pos_err_m | rot_err_rad as float32 [n] each, then self_mask | env_mask | jlim_mask as uint8 [n] each, back to
back.  This module is the only place that knows the layout; it imports neither `robots` nor `distributed`, which both use it.
"""

from typing import Dict

import torch

PACKED_BYTES_PER_ROW = 15  # 3 x fp32 (ext_cost, pos_err_m, rot_err_rad) + 3 x u8 (self, env, jlim masks)


def packed_views(packed: torch.Tensor, n: int) -> Dict[str, torch.Tensor]:
    """The six named views into a packed buffer of n rows (CPU or device), in the order of the layout.  The kernels write the fp32
    part through 4-byte stores, hence the alignment."""
    assert packed.dtype == torch.uint8 and packed.is_contiguous(), "a packed buffer is a contiguous uint8 tensor"
    assert packed.numel() == PACKED_BYTES_PER_ROW * n, f"{n} rows pack into {PACKED_BYTES_PER_ROW * n} bytes, not {packed.numel()}"
    assert packed.data_ptr() % 4 == 0, "a packed buffer starts 4-byte aligned"
    f, m = packed[: 12 * n].view(torch.float32), packed[12 * n :]
    return dict(ext_cost=f[:n], pos_err_m=f[n : 2 * n], rot_err_rad=f[2 * n :], self_mask=m[:n], env_mask=m[n : 2 * n],
                jlim_mask=m[2 * n :])  # fmt: skip
