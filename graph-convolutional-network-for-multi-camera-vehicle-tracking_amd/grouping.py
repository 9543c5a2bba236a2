"""`group_by_index`: a stable grouping of int64 keys on the device (`mtmc_group_by_index`, csrc/group_index.hip).

`index` [D] names the group of every row; the result lists the rows group by group, each group's rows in increasing row
order, with the offsets that cut the list.  It is what `pool_tracklets(index=)` pools through and what the repeatable
`scatter_*(..., deterministic=)` forwards reduce over.  A `Grouping` can be made once and used many times: a training run
keeps one edge list for every round and every step.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _call, _lib


class Grouping(NamedTuple):
    """index [D] int64 (as given, contiguous), perm [D] int64: the rows by group, equal groups in increasing row order,
    offsets [num_groups + 1] int64: group g owns perm[offsets[g]:offsets[g+1]]; rows whose index lies outside
    [0, num_groups) lie behind offsets[-1], in row order, and belong to no group."""
    index: torch.Tensor
    perm: torch.Tensor
    offsets: torch.Tensor
    num_groups: int


def check_num_groups(name, num_groups) -> int:
    if isinstance(num_groups, bool) or not isinstance(num_groups, (int, np.integer)) or not 0 <= num_groups < 2 ** 31:
        raise ValueError(f"mtmc_mpn.{name}: the number of groups must be a host int in [0, 2^31)")
    return int(num_groups)


def group_raw(index: torch.Tensor, num_groups: int, digit_bits: int = 0, info=None):
    """The raw library call: index [D] int64, contiguous, on a ROCm GPU -> (perm [D], offsets [num_groups + 1]).  Nothing
    is read back and nothing synchronises: legal inside `torch.cuda.graph`.  `info`: an int32 tensor whose first word
    receives the number of rows outside [0, num_groups)."""
    d, dev = index.numel(), index.device
    if d >= 2 ** 31:
        raise RuntimeError("mtmc_mpn.group_by_index: at most 2^31 - 1 rows")
    lib = _lib.load()
    perm = torch.empty(d, dtype=torch.int64, device=dev)
    offsets = torch.empty(num_groups + 1, dtype=torch.int64, device=dev)
    need = lib.mtmc_group_by_index_workspace_bytes(d, num_groups, digit_bits)
    if need == 0:
        raise RuntimeError("mtmc_mpn.group_by_index: unsupported size")
    ws = torch.empty(need if d and num_groups else 0, dtype=torch.uint8, device=dev)
    _call.run(dev, lib.mtmc_group_by_index, index.data_ptr(), d, num_groups, digit_bits, perm.data_ptr(), offsets.data_ptr(),
              None if info is None else info.data_ptr(), ws.data_ptr() if ws.numel() else None, ws.numel(), _call.stream(dev))
    return perm, offsets


def group_by_index(index: torch.Tensor, num_groups: int) -> Grouping:
    """Group the rows of `index` (an integer [D] tensor on a ROCm GPU) into `num_groups` groups (a host int, so that
    nothing is read back to size the result).  Three to four kernel launches, capturable."""
    n = check_num_groups("group_by_index", num_groups)
    _call.require_gpu("group_by_index", index)
    from . import torch_ops  # noqa: F401  (registers torch.ops.mtmc_mpn.group_by_index)
    if index.dim() != 1 or index.dtype not in (torch.int64, torch.int32):
        raise RuntimeError("mtmc_mpn.group_by_index: index must be a 1-D int64 or int32 tensor")
    index = index.contiguous().long()
    perm, offsets = torch.ops.mtmc_mpn.group_by_index(index, n)
    return Grouping(index, perm, offsets, n)
