"""Host glue shared by the stand-alone operators (ops, metrics, pool, graph_build, postprocess, the scatter part of
torch_ops): which stream a call goes to, which tensors it may take, and how a library call is made and checked."""
from __future__ import annotations

import torch

from . import _lib


def stream(dev):
    """The current HIP stream of `dev`, as the `void* stream` of the C ABI."""
    return torch.cuda.current_stream(dev).cuda_stream


def require_gpu(name, *tensors):
    """RuntimeError unless every tensor lives on one ROCm GPU: there is no CPU path behind the operators."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        raise RuntimeError(f"mtmc_mpn.{name}: tensors must be on a ROCm GPU (no CPU path)")
    if any(t.device != tensors[0].device for t in tensors):
        raise RuntimeError(f"mtmc_mpn.{name}: the tensors must be on one device, got " +
                           " and ".join(sorted({str(t.device) for t in tensors})))


def run(dev, fn, *args):
    """One library call on device `dev`; a negative return code raises with the library's error text (`_lib.check`)."""
    with torch.cuda.device(dev):
        _lib.check(fn(*args))


def steps_block(steps) -> bool:
    """Are the classified steps consecutive [E, C] float32 slices of one block (what a forward of this package returns)?"""
    s0 = steps[0]
    return all(t.shape == s0.shape and t.dtype == s0.dtype and t.device == s0.device and t.is_contiguous()
               and t.data_ptr() == s0.data_ptr() + i * s0.numel() * 4 for i, t in enumerate(steps))


def class_weight(weight, device, n, name):
    """A class-weight vector as the kernels read it: float32, contiguous, on `device`, `n` entries; None stays None."""
    if weight is None:
        return None
    weight = weight.to(device=device, dtype=torch.float32).contiguous()
    if weight.numel() != n:
        raise RuntimeError(f"mtmc_mpn.{name}: weight must have one entry per class")
    return weight
