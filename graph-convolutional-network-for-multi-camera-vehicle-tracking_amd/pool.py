"""`pool_tracklets`: from detections to node features on the GPU.

Replaces the reference's per-tracklet Python loop -- one `torch.mean(bboxes_embeds, 0)` per tracklet, then `torch.stack`
(train.py:305-316; once per tracklet with a `.cpu()` and a pickle each in libs/reid_feature_extraction.py:161-184) -- by
one library call (`mtmc_pool_tracklets`): a segmented mean over contiguous row ranges of the [D detections, F] embedding
matrix, with an HIP backward for fine-tuning the CNN.  The result is what `build_graph` takes as `node_feats`.
Detections in any order (`index=`: a stable grouping on the device, then the same sums through a row permutation) and
per-detection weights (`weights=`: box-area / ROI filters of libs/filter_mtmc.py, confidences, a learned quality score) go
through `mtmc_pool_tracklets_weighted` and its two backwards.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _call, _lib
from .grouping import Grouping

CHUNK_ROWS = 32          # mtmc_pool_chunk_rows(): rows per chunk of the kernels' decomposition
MAX_FEAT_DIM = 16384
_STATUS = {1: "offsets are not strictly increasing, or leave [0, D]",
           2: "offsets[0] != 0 or offsets[N] != D"}
# mtmc_pool_tracklets_weighted: info[0] is a set of bits; info[1] tracklets with a bad range, info[2] tracklets that got a
# zero row (empty, or weights adding up to 0), info[3] detections of no tracklet
_STATUS_BITS = {1: "offsets decrease (without index: do not strictly increase), or leave [0, D]",
                2: "offsets[0] != 0 or offsets[N] != D",
                4: "perm has entries outside [0, D) (the grouping of index)",
                8: "weights must be finite and >= 0"}


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


def _forward_call(entry, embeds, offsets_dev, out, info, wsum=None, extra=()):
    """What the two forward entry points share: `out` [N, F] and `info` [4] made or checked, the early-out of a call in
    which the library launches nothing, the workspace, the call.  `wsum` and `extra` (perm, weights) go to the weighted one."""
    d, f = embeds.shape
    n = offsets_dev.numel() - 1
    dev = embeds.device
    if out is None:
        out = torch.empty((n, f), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n, f) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError("mtmc_mpn.pool_tracklets: out must be a contiguous float32 [N, F] tensor on the device of embeds")
    if info is None:
        info = torch.empty(_lib.POOL_INFO, dtype=torch.int32, device=dev)
    results = [out] if wsum is None else [out, wsum]
    if n == 0 or d == 0:                       # the library launches nothing
        for t in results + [info]:
            t.zero_()
        return out
    embeds = _usable(embeds)
    lib = _lib.load()
    need = getattr(lib, entry + "_workspace_bytes")(d, f)
    if need == 0:
        raise RuntimeError("mtmc_mpn.pool_tracklets: unsupported size")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _call.run(dev, getattr(lib, entry), embeds.data_ptr(), embeds.stride(0), d, f, offsets_dev.data_ptr(), n,
              *[None if t is None else t.data_ptr() for t in extra], *[t.data_ptr() for t in results], info.data_ptr(),
              ws.data_ptr(), ws.numel(), _call.stream(dev))
    return out


def _backward_call(entry, grad_out, offsets_dev, n_rows, out, extra=()):
    """What the two backward entry points share: `out` [n_rows, F] made or checked (unit column stride, row stride a
    multiple of 4), the early-out, the call.  `extra` (perm, weights, wsum) goes to the weighted one."""
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
    _call.run(dev, getattr(_lib.load(), entry), grad_out.data_ptr(), n_rows, f, offsets_dev.data_ptr(), n,
              *[None if t is None else t.data_ptr() for t in extra], out.data_ptr(), out.stride(0), _call.stream(dev))
    return out


def _forward_raw(embeds: torch.Tensor, offsets_dev: torch.Tensor, out=None, info=None) -> torch.Tensor:
    """The raw library call: embeds [D, F] float32, offsets_dev [N+1] int64 on the same device.  `out` [N, F] (contiguous) and
    `info` [4] int32 are written when given.  Nothing is read back."""
    return _forward_call("mtmc_pool_tracklets", embeds, offsets_dev, out, info)


def _backward_raw(grad_out: torch.Tensor, offsets_dev: torch.Tensor, n_rows: int, out=None) -> torch.Tensor:
    """grad_out [N, F] float32 -> the gradient [n_rows, F] of the embeddings (written into `out` when given: unit column
    stride, row stride a multiple of 4)."""
    return _backward_call("mtmc_pool_tracklets_backward", grad_out, offsets_dev, n_rows, out)


def group_by_index(index: torch.Tensor, num_tracklets: int):
    """Stable grouping of detections that arrive in any order: `index` [D] int64 on the device (the tracklet of each
    detection) -> (perm [D], offsets [num_tracklets + 1]), both int64 on that device.  perm lists the detection rows
    tracklet by tracklet, each tracklet's rows in increasing row order (a stable sort of D keys); tracklet s owns
    perm[offsets[s]:offsets[s+1]].  Detections whose index lies outside [0, num_tracklets) sort behind offsets[-1] and
    belong to no tracklet.  One library call (`mtmc_group_by_index`: a radix sort in HIP, csrc/group_index.hip): nothing is
    read back or synchronised, and the call can be captured.  `mtmc_mpn.group_by_index` returns the same two tensors as a
    `Grouping`, for `pool_tracklets(grouping=)`."""
    from . import torch_ops  # noqa: F401  (registers torch.ops.mtmc_mpn.group_by_index)
    _call.require_gpu("group_by_index", index)
    return torch.ops.mtmc_mpn.group_by_index(index.contiguous(), int(num_tracklets))


def _forward_weighted_raw(embeds, offsets_dev, perm=None, weights=None, out=None, info=None, wsum=None):
    """The raw call of `mtmc_pool_tracklets_weighted`: embeds [D, F] float32, offsets_dev [N+1] int64, perm [D] int64 or
    None, weights [D] float32 (contiguous) or None, all on one device.  Returns (out [N, F], wsum [N]); `info` [4] int32
    is written when given.  Nothing is read back."""
    if wsum is None:
        wsum = torch.empty(offsets_dev.numel() - 1, dtype=torch.float32, device=embeds.device)
    return _forward_call("mtmc_pool_tracklets_weighted", embeds, offsets_dev, out, info, wsum, (perm, weights)), wsum


def _backward_weighted_raw(grad_out, offsets_dev, n_rows, wsum, perm=None, weights=None, out=None):
    """grad_out [N, F] float32 -> the gradient [n_rows, F] of the embeddings, w_r g[s(r)] / W_s, each row written once
    through `perm` (into `out` when given: unit column stride, row stride a multiple of 4)."""
    return _backward_call("mtmc_pool_tracklets_weighted_backward", grad_out, offsets_dev, n_rows, out, (perm, weights, wsum))


def _weight_grad_raw(embeds, grad_out, pooled, offsets_dev, wsum, perm=None):
    """The gradient [D] of the weights: g[s] . (x_r - out[s]) / W_s (`mtmc_pool_tracklets_weight_grad`); 0 for a
    detection of no tracklet and in a tracklet whose weights add up to 0."""
    d, f = embeds.shape
    n = offsets_dev.numel() - 1
    dev = embeds.device
    grad_w = torch.zeros(d, dtype=torch.float32, device=dev)
    if n == 0 or d == 0:
        return grad_w
    embeds, grad_out, pooled = _usable(embeds), grad_out.contiguous(), pooled.contiguous()
    _call.run(dev, _lib.load().mtmc_pool_tracklets_weight_grad, embeds.data_ptr(), embeds.stride(0), d, f, offsets_dev.data_ptr(),
              n, None if perm is None else perm.data_ptr(), grad_out.data_ptr(), pooled.data_ptr(), wsum.data_ptr(),
              grad_w.data_ptr(), _call.stream(dev))
    return grad_w


class _PoolWeighted(torch.autograd.Function):
    """`pool_tracklets(index=, weights=)` with its HIP backwards.  Kept for them: the offsets, the permutation, the
    weights and the [N] weight sums; `embeds` and the result only when the weights take a gradient."""

    @staticmethod
    def forward(ctx, embeds, weights, offsets_dev, perm, info):
        w = None if weights is None else weights.detach().contiguous()
        out, wsum = _forward_weighted_raw(embeds.detach(), offsets_dev, perm, w, info=info)
        ctx.n_rows = embeds.shape[0]
        ctx.weight_grad = weights is not None and ctx.needs_input_grad[1]
        if ctx.weight_grad:
            ctx.save_for_backward(offsets_dev, perm, w, wsum, embeds, out)
        else:
            ctx.save_for_backward(offsets_dev, perm, w, wsum)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        offsets_dev, perm, w, wsum = ctx.saved_tensors[:4]
        g = g.float()
        grad_e = grad_w = None
        if ctx.needs_input_grad[0]:
            grad_e = _backward_weighted_raw(g, offsets_dev, ctx.n_rows, wsum, perm, w)
        if ctx.weight_grad:
            embeds, out = ctx.saved_tensors[4:]
            grad_w = _weight_grad_raw(embeds, g, out, offsets_dev, wsum, perm)
        return grad_e, grad_w, None, None, None


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


def _raise_on(info: torch.Tensor, by_index: bool):
    """check=True: one 16-byte D2H copy of the status words, RuntimeError on what they report."""
    status, _, _, lost = info.cpu().tolist()
    said = [text for bit, text in _STATUS_BITS.items() if status & bit]
    if by_index and lost and not said:
        said = [f"{lost} entries of index lie outside [0, num_tracklets)"]
    if said:
        raise RuntimeError("mtmc_mpn.pool_tracklets: " + "; ".join(said))


def pool_tracklets(embeds: torch.Tensor, lengths=None, *, offsets=None, index=None, num_tracklets=None, weights=None,
                   check: bool = True, grouping=None) -> torch.Tensor:
    """embeds: [D, F] float32 on a ROCm GPU, the detections' embeddings.  Returns the [N, F] float32 per-tracklet means
    (contiguous).  Give exactly one of

    lengths  N positive ints on the host (sequence, numpy array, CPU int tensor: the reference's `imgs_bboxes.shape[0]`):
             each tracklet's rows lie next to each other.  Checked on the host (`offsets_from_lengths`) and uploaded once;
    offsets  an int64 [N+1] tensor on the device of `embeds`, used as is (a captured graph reads it at replay time);
    index    an int64 [D] tensor on the device of `embeds`: the tracklet of each detection, rows in any order (frame by
             frame, say), with `num_tracklets` = N as a host int so that nothing is read back to size the result.  The
             rows of a tracklet are added in increasing row order (`group_by_index`: a stable sort on the device), so the
             result has the same bits on every run and the bits of the grouped call on the same rows.  A tracklet no
             detection names gets a zero row.  A detection whose index is outside [0, N) belongs to no tracklet: it adds
             nothing and its gradient row is zero (check=True raises RuntimeError about `index`);
    grouping a `Grouping` of the D detections made beforehand (`mtmc_mpn.group_by_index(index, N)`): the `index` form
             without its grouping step, with the same bits.  Group once, pool many times.

    weights  optional float32 [D] tensor on that device (any stride), one weight per detection ROW, finite and >= 0:
             out[s] = sum_r w_r x_r / sum_r w_r.  A weight of 0 removes a detection without repacking `embeds`; a
             tracklet whose weights add up to 0 gets a zero row and zero gradients.  All weights 1 give the bits of the
             plain call.  A negative or non-finite weight counts as 0 (check=True raises RuntimeError about `weights`).

    check=True reads the kernels' four status words with one small D2H copy and raises RuntimeError on bad offsets,
    index or weights (with `lengths` and no weights there is nothing to read).  check=False never synchronises, so the
    `offsets`, `index` and `grouping` forms, weighted or not, are legal inside `torch.cuda.graph` (the grouping of `index`
    is three to four kernel launches of this library on the current stream).

    With grad mode on the result carries the gradient back to `embeds` (d_embeds[r] = w_r g[s] / W_s) and, when
    `weights.requires_grad`, to the weights (d_w[r] = g[s] . (x_r - out[s]) / W_s; `embeds` and the result are kept for
    the backward only then).  Once differentiable."""
    if sum(v is not None for v in (lengths, offsets, index, grouping)) != 1:
        raise ValueError("mtmc_mpn.pool_tracklets: give exactly one of lengths, offsets, index and grouping")
    if (index is None) != (num_tracklets is None):
        raise ValueError("mtmc_mpn.pool_tracklets: num_tracklets goes with index (a host int), and only with it")
    _call.require_gpu("pool_tracklets", embeds)
    if embeds.dim() != 2 or embeds.dtype != torch.float32 or embeds.shape[1] % 4 or not 4 <= embeds.shape[1] <= MAX_FEAT_DIM:
        raise RuntimeError(f"mtmc_mpn.pool_tracklets: embeds must be float32 [D, F] with F a multiple of 4, at most {MAX_FEAT_DIM}")
    dev = embeds.device
    d = embeds.shape[0]
    perm = None
    if lengths is not None:
        offsets_dev = torch.from_numpy(offsets_from_lengths(lengths, d)).to(dev)
        check = check and weights is not None      # the lengths are checked on the host already
    elif offsets is not None:
        if not (isinstance(offsets, torch.Tensor) and offsets.device == dev and offsets.dtype == torch.int64 and
                offsets.dim() == 1 and offsets.numel() >= 1):
            raise RuntimeError("mtmc_mpn.pool_tracklets: offsets must be an int64 [N+1] tensor on the device of embeds")
        offsets_dev = offsets.contiguous()
    elif grouping is not None:
        if not (isinstance(grouping, Grouping) and grouping.perm.device == dev and tuple(grouping.perm.shape) == (d,)):
            raise RuntimeError("mtmc_mpn.pool_tracklets: grouping must be a Grouping of the D rows of embeds, on its device")
        perm, offsets_dev = grouping.perm, grouping.offsets
    else:
        if not (isinstance(index, torch.Tensor) and index.device == dev and index.dtype == torch.int64 and
                tuple(index.shape) == (d,)):
            raise RuntimeError("mtmc_mpn.pool_tracklets: index must be an int64 [D] tensor on the device of embeds")
        if isinstance(num_tracklets, bool) or not isinstance(num_tracklets, (int, np.integer)) or not 0 <= num_tracklets < 2 ** 31:
            raise ValueError("mtmc_mpn.pool_tracklets: num_tracklets must be a host int in [0, 2^31)")
        perm, offsets_dev = group_by_index(index, int(num_tracklets))
    if weights is not None and not (isinstance(weights, torch.Tensor) and weights.device == dev and
                                    weights.dtype == torch.float32 and tuple(weights.shape) == (d,)):
        raise RuntimeError("mtmc_mpn.pool_tracklets: weights must be a float32 [D] tensor on the device of embeds")
    info = torch.empty(_lib.POOL_INFO, dtype=torch.int32, device=dev)
    grad_w = weights is not None and weights.requires_grad
    if perm is None and weights is None:           # the grouped mean: its own entry points and kernels
        if torch.is_grad_enabled() and embeds.requires_grad:
            out = _PoolTracklets.apply(embeds, offsets_dev, info)
        else:
            out = _forward_raw(embeds, offsets_dev, info=info)
        if check:
            status = info.cpu().tolist()[0]
            if status:
                raise RuntimeError("mtmc_mpn.pool_tracklets: " + _STATUS.get(status, f"status {status}"))
        return out
    if torch.is_grad_enabled() and (embeds.requires_grad or grad_w):
        out = _PoolWeighted.apply(embeds, weights, offsets_dev, perm, info)
    else:
        out, _ = _forward_weighted_raw(embeds, offsets_dev, perm, None if weights is None else weights.detach().contiguous(),
                                       info=info)
    if check:
        _raise_on(info, perm is not None)
    return out
