"""`pool_tracklets`: from detections to node features on the GPU.

Replaces the reference's per-tracklet Python loop -- one `torch.mean(bboxes_embeds, 0)` per tracklet, then `torch.stack`
(train.py:305-316; once per tracklet with a `.cpu()` and a pickle each in libs/reid_feature_extraction.py:161-184) -- by
one library call (`mtmc_pool_tracklets`): a segmented mean over contiguous row ranges of the [D detections, F] embedding
matrix, with an HIP backward for fine-tuning the CNN.  The result is what `build_graph` takes as `node_feats`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _call, _lib

CHUNK_ROWS = 32          # mtmc_pool_chunk_rows(): rows per chunk of the kernels' decomposition
MAX_FEAT_DIM = 16384
_STATUS = {1: "offsets are not strictly increasing, or leave [0, D]",
           2: "offsets[0] != 0 or offsets[N] != D"}


def offsets_from_lengths(lengths, n_rows: int) -> np.ndarray:
    """N positive tracklet lengths (sequence, numpy array or CPU int tensor) -> the int64 [N+1] row offsets.
    ValueError on a zero or negative length and when the lengths do not add up to `n_rows`."""
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda:
            raise ValueError("mtmc_mpn.pool_tracklets: lengths live on the host (pass device offsets as offsets=)")
        lengths = lengths.numpy()
    arr = np.asarray(lengths)
    if arr.size == 0:
        arr = arr.astype(np.int64)
    if arr.ndim != 1 or arr.dtype.kind not in "iu":
        raise ValueError("mtmc_mpn.pool_tracklets: lengths must be a 1-d sequence of ints")
    arr = arr.astype(np.int64)
    if arr.size and int(arr.min()) <= 0:
        raise ValueError("mtmc_mpn.pool_tracklets: every tracklet length must be positive")
    offsets = np.zeros(arr.size + 1, dtype=np.int64)
    np.cumsum(arr, out=offsets[1:])
    if int(offsets[-1]) != int(n_rows):
        raise ValueError(f"mtmc_mpn.pool_tracklets: lengths add up to {int(offsets[-1])}, embeds has {int(n_rows)} rows")
    return offsets


def _usable(t: torch.Tensor) -> torch.Tensor:
    """A [rows, F] view the kernels read or write in place, else a contiguous copy."""
    ok = t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0
    return t if ok or t.numel() == 0 else t.contiguous()


def _forward_raw(embeds: torch.Tensor, offsets_dev: torch.Tensor, out=None, info=None) -> torch.Tensor:
    """The raw library call: embeds [D, F] float32, offsets_dev [N+1] int64 on the same device.  `out` [N, F] (contiguous) and
    `info` [4] int32 are written when given.  Nothing is read back."""
    d, f = embeds.shape
    n = offsets_dev.numel() - 1
    dev = embeds.device
    if out is None:
        out = torch.empty((n, f), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n, f) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError("mtmc_mpn.pool_tracklets: out must be a contiguous float32 [N, F] tensor on the device of embeds")
    if info is None:
        info = torch.empty(_lib.POOL_INFO, dtype=torch.int32, device=dev)
    if n == 0 or d == 0:                       # the library launches nothing
        out.zero_()
        info.zero_()
        return out
    embeds = _usable(embeds)
    lib = _lib.load()
    need = lib.mtmc_pool_tracklets_workspace_bytes(d, f)
    if need == 0:
        raise RuntimeError("mtmc_mpn.pool_tracklets: unsupported size")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _call.run(dev, lib.mtmc_pool_tracklets, embeds.data_ptr(), embeds.stride(0), d, f, offsets_dev.data_ptr(), n, out.data_ptr(),
              info.data_ptr(), ws.data_ptr(), ws.numel(), _call.stream(dev))
    return out


def _backward_raw(grad_out: torch.Tensor, offsets_dev: torch.Tensor, n_rows: int, out=None) -> torch.Tensor:
    """grad_out [N, F] float32 -> the gradient [n_rows, F] of the embeddings (written into `out` when given: unit column
    stride, row stride a multiple of 4)."""
    n, f = grad_out.shape
    dev = grad_out.device
    grad_out = grad_out.contiguous()
    if out is None:
        out = torch.empty((n_rows, f), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n_rows, f) or out.dtype != torch.float32 or out.device != dev or _usable(out) is not out:
        raise RuntimeError("mtmc_mpn.pool_tracklets: backward out must be float32 [D, F] with unit column stride and a row "
                           "stride that is a multiple of 4")
    if n == 0 or n_rows == 0:
        out.zero_()
        return out
    _call.run(dev, _lib.load().mtmc_pool_tracklets_backward, grad_out.data_ptr(), n_rows, f, offsets_dev.data_ptr(), n,
              out.data_ptr(), out.stride(0), _call.stream(dev))
    return out


class _PoolTracklets(torch.autograd.Function):
    """`pool_tracklets` with its HIP backward (`mtmc_pool_tracklets_backward`).  Only the offsets are kept for it."""

    @staticmethod
    def forward(ctx, embeds, offsets_dev, info):
        ctx.save_for_backward(offsets_dev)
        ctx.n_rows = embeds.shape[0]
        return _forward_raw(embeds.detach(), offsets_dev, info=info)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (offsets_dev,) = ctx.saved_tensors
        return _backward_raw(g.float(), offsets_dev, ctx.n_rows), None, None


def pool_tracklets(embeds: torch.Tensor, lengths=None, *, offsets=None, check: bool = True) -> torch.Tensor:
    """embeds: [D, F] float32 on a ROCm GPU, the detections' embeddings with each tracklet's rows next to each other.
    Returns the [N, F] float32 per-tracklet means.  Give exactly one of

    lengths  N positive ints on the host (sequence, numpy array, CPU int tensor: the reference's `imgs_bboxes.shape[0]`),
             checked on the host (`offsets_from_lengths`) and uploaded once; nothing is read back;
    offsets  an int64 [N+1] tensor on the device of `embeds`, used as is (a captured graph reads it at replay time).
             check=True reads the kernels' status word with one small D2H copy and raises RuntimeError on bad offsets;
             check=False never synchronises, so the call is legal inside `torch.cuda.graph`.

    With grad mode on and `embeds.requires_grad` the result carries the gradient back to `embeds`."""
    if (lengths is None) == (offsets is None):
        raise ValueError("mtmc_mpn.pool_tracklets: give exactly one of lengths and offsets")
    _call.require_gpu("pool_tracklets", embeds)
    if embeds.dim() != 2 or embeds.dtype != torch.float32 or embeds.shape[1] % 4 or not 4 <= embeds.shape[1] <= MAX_FEAT_DIM:
        raise RuntimeError(f"mtmc_mpn.pool_tracklets: embeds must be float32 [D, F] with F a multiple of 4, at most {MAX_FEAT_DIM}")
    dev = embeds.device
    if lengths is not None:
        offsets_dev = torch.from_numpy(offsets_from_lengths(lengths, embeds.shape[0])).to(dev)
        check = False                              # checked on the host already
    else:
        if not (isinstance(offsets, torch.Tensor) and offsets.device == dev and offsets.dtype == torch.int64 and
                offsets.dim() == 1 and offsets.numel() >= 1):
            raise RuntimeError("mtmc_mpn.pool_tracklets: offsets must be an int64 [N+1] tensor on the device of embeds")
        offsets_dev = offsets.contiguous()
    info = torch.empty(_lib.POOL_INFO, dtype=torch.int32, device=dev)
    if torch.is_grad_enabled() and embeds.requires_grad:
        out = _PoolTracklets.apply(embeds, offsets_dev, info)
    else:
        out = _forward_raw(embeds, offsets_dev, info=info)
    if check:
        status = info.cpu().tolist()[0]
        if status:
            raise RuntimeError("mtmc_mpn.pool_tracklets: " + _STATUS.get(status, f"status {status}"))
    return out
