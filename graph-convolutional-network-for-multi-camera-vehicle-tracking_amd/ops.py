"""Stand-alone ops of the hot path, for callers that use the pieces on their own:

  scatter_add / scatter_mean / scatter_max   the call forms of the third-party `torch_scatter` op the
      reference aggregates with (`scatter_*(src, index, dim=0, dim_size=N)`, reference models/mpn.py:196-202);
      differentiable (once) with respect to a floating `src`, like the op they stand in for; `deterministic=True` or a
      `Grouping` makes the forward a segmented reduction in one fixed order instead of float atomics
  mlp_forward                                `MLP.forward` (reference models/mlp.py:32-33), eval mode
  cross_entropy                              `F.cross_entropy(input, target, weight, reduction=...)` on the [E, C<=4]
      edge logits, forward and backward fused (the training callers' loss, reference train.py:88-93, :109-142)
  edge_confusion                             TP / FP / TN / FN of argmax(logits) against the edge labels in one pass,
      without the device synchronisations of boolean-mask indexing (reference train.py:98-107, inference.py:20-67)
  edge_loss                                  everything the training / validation loops' `compute_loss_acc` returns
      (reference train.py:36-245: balanced CE or one-logit BCE, FPR term, per-class losses and probabilities, confusion
      counts) for every classified step in one pass, with a fused backward and no host read; `gamma` > 0: focal rows
  focal_loss / FocalLoss                     the `Focal` loss of the reference's training config (config_training.yaml:37,
      main_training.py:273-276, whose class is commented out) on [E, 2] or [E, 1] logits: mean, sum or per row

All of them run HIP kernels through the C ABI; CPU tensors are refused.
"""
from __future__ import annotations

import collections
import ctypes as C

import torch

from . import _call, _lib
from . import torch_ops  # noqa: F401  (registers torch.ops.mtmc_mpn.*)
from .grouping import Grouping, group_by_index


def _scatter(name, src, index, dim, out, dim_size, deterministic=False):
    if out is not None:
        raise NotImplementedError(f"mtmc_mpn.{name}: `out=` is not supported")
    if deterministic is False or deterministic is None:
        _call.require_gpu(name, src, index)
        return getattr(torch.ops.mtmc_mpn, name)(src, index, dim, dim_size)
    # the repeatable forward: a segmented reduction over a stable grouping of the rows (csrc/group_index.hip)
    g = deterministic if isinstance(deterministic, Grouping) else None
    if g is None and deterministic is not True:
        raise TypeError(f"mtmc_mpn.{name}: deterministic must be False, True or a Grouping (mtmc_mpn.group_by_index)")
    if g is None and dim_size is None:
        raise ValueError(f"mtmc_mpn.{name}: deterministic=True needs dim_size: without it the size of the result is found "
                         "with a host read of index.max(), which the repeatable forward never does (it synchronises and "
                         "cannot be captured)")
    if g is not None and dim_size is not None and int(dim_size) != g.num_groups:
        raise ValueError(f"mtmc_mpn.{name}: dim_size is {int(dim_size)}, the Grouping has {g.num_groups} groups")
    if g is not None and index is None:
        index = g.index
    _call.require_gpu(name, src, index)
    if dim not in (0, -max(src.dim(), 1)):
        raise NotImplementedError("mtmc_mpn.scatter_*: only dim=0 (the reference's call form) is implemented")
    if index.dim() != 1 or src.dim() < 1 or index.shape[0] != src.shape[0]:
        raise RuntimeError("mtmc_mpn.scatter_*: index must be 1-D with one entry per row of src")
    if not src.dtype.is_floating_point:                # exact int64 sums: no order to fix
        return getattr(torch.ops.mtmc_mpn, name)(src, index, dim, g.num_groups if g is not None else dim_size)
    if g is None:
        g = group_by_index(index, dim_size)
    elif g.index.device != src.device or g.perm.shape[0] != src.shape[0]:
        raise RuntimeError(f"mtmc_mpn.{name}: the Grouping must group the rows of src, on its device")
    return getattr(torch.ops.mtmc_mpn, name + "_grouped")(src, g.index, g.perm, g.offsets)


def scatter_add(src, index, dim=0, out=None, dim_size=None, deterministic=False):
    """`torch_scatter.scatter_add(src, index, dim=0, dim_size=N)`; integer `src` (the 1-D int64 form of reference
    utils.py:173-174) is summed exactly and keeps its dtype.  Differentiable with respect to a floating `src`:
    d_src[e] = grad[index[e]], zeros for a row whose index lies outside [0, N).

    deterministic=False adds with float atomics: the last bits of a sum change from run to run.  deterministic=True groups
    the rows on the device (`mtmc_mpn.group_by_index`) and reduces group by group in one fixed order: the same bits on
    every run, no fill launch and no float atomic; `dim_size` is then required, nothing is read back, and forward and
    backward are legal inside `torch.cuda.graph`.  deterministic=G, a `Grouping` made beforehand from the same index,
    skips the grouping (`index` may then be `G.index` or None): group once, scatter every round and every step.  The
    gradients are those of the default call, bit for bit."""
    return _scatter("scatter_add", src, index, dim, out, dim_size, deterministic)


scatter_sum = scatter_add


def scatter_mean(src, index, dim=0, out=None, dim_size=None, deterministic=False):
    """`torch_scatter.scatter_mean(src, index, dim=0, dim_size=N)`: the sum divided by max(count, 1).  Differentiable with
    respect to `src`: d_src[e] = grad[index[e]] / max(count[index[e]], 1).  `deterministic`: as in `scatter_add`."""
    return _scatter("scatter_mean", src, index, dim, out, dim_size, deterministic)


def scatter_max(src, index, dim=0, out=None, dim_size=None, deterministic=False):
    """Returns (values, argmax) like torch_scatter; rows nobody writes hold 0 and argmax = src.size(0).  `values` is
    differentiable with respect to `src`: the gradient of values[r, c] goes to row argmax[r, c], the first row that attains
    the maximum, and to no other; the argmax carries none.  `deterministic`: as in `scatter_add` (a maximum has the same
    bits either way; the grouped form needs no fill and no atomic)."""
    return _scatter("scatter_max", src, index, dim, out, dim_size, deterministic)


def layer_forward(a: torch.Tensor, weight, bias, gamma=None, beta=None) -> torch.Tensor:
    """One Linear (+ BatchNorm1d with batch statistics + ReLU when gamma/beta are given) on the GPU."""
    if gamma is not None and a.shape[0] < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(list(a.shape)))
    a = a.float()
    if a.stride(-1) != 1:
        a = a.contiguous()
    out_dim, in_dim = weight.shape
    lay = _lib.Layer()
    lay.weight, lay.bias = weight.data_ptr(), bias.data_ptr()
    lay.gamma = gamma.data_ptr() if gamma is not None else None
    lay.beta = beta.data_ptr() if beta is not None else None
    lay.in_dim, lay.out_dim = in_dim, out_dim
    y = torch.empty((a.shape[0], out_dim), dtype=torch.float32, device=a.device)
    stats = torch.empty((2 * out_dim,), dtype=torch.float64, device=a.device)
    _call.run(a.device, _lib.load().mtmc_mlp_layer_forward, C.byref(lay), a.data_ptr(), a.stride(0), a.shape[0], y.data_ptr(),
              stats.data_ptr(), _call.stream(a.device))
    return y


def mlp_forward(mlp, inp: torch.Tensor) -> torch.Tensor:
    """Eval-mode `MLP.forward`: per hidden layer Linear -> BatchNorm1d (batch statistics) -> ReLU."""
    _call.require_gpu("MLP", inp)
    if mlp.training and any(l.dropout_p for l in mlp.layers):
        raise NotImplementedError("mtmc_mpn.MLP: training-mode Dropout is not built yet; use .eval()")
    if torch.is_grad_enabled() and (inp.requires_grad or any(p.requires_grad for p in mlp.parameters())):
        raise NotImplementedError("mtmc_mpn.MLP: backward is not built yet; call under torch.no_grad()")
    a = inp
    for spec in mlp.layers:
        lin = mlp.fc_layers[spec.lin_slot]
        bn = mlp.fc_layers[spec.bn_slot] if spec.bn_slot is not None else None
        a = layer_forward(a, lin.weight, lin.bias, bn.weight if bn is not None else None,
                          bn.bias if bn is not None else None)
        if spec.relu and bn is None:
            a = torch.relu_(a)
    return a


_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}


class _CrossEntropy(torch.autograd.Function):
    """One [E, C] tensor (any reduction: mtmc_cross_entropy_*), or the classified steps of one forward, consecutive [E, C]
    slices of one block (mean or sum: mtmc_cross_entropy_steps_*, one pass over all of them)."""

    @staticmethod
    def forward(ctx, target, weight, mode, ignore_index, *steps):
        s = len(steps)
        x = steps[0].contiguous() if s == 1 else steps[0]
        n, c = x.shape
        dev = x.device
        lib = _lib.load()
        sums = torch.empty(2 * _lib.STAT_REPLICAS, dtype=torch.float64, device=dev)
        out = torch.empty(n if mode == 2 else (), dtype=torch.float32, device=dev)
        head = (x.data_ptr(), target.data_ptr(), weight.data_ptr() if weight is not None else None, n, c)
        if s == 1:
            per, loss = (out.data_ptr(), None) if mode == 2 else (None, out.data_ptr())
            _call.run(dev, lib.mtmc_cross_entropy_forward, *head, ignore_index, mode, per, sums.data_ptr(), loss, _call.stream(dev))
        else:
            _call.run(dev, lib.mtmc_cross_entropy_steps_forward, *head, s, ignore_index, mode, sums.data_ptr(), out.data_ptr(),
                      _call.stream(dev))
        ctx.save_for_backward(target, weight, sums, x, *steps[1:])
        ctx.mode, ctx.ignore_index = mode, ignore_index
        return out

    @staticmethod
    def backward(ctx, grad):
        target, weight, sums, *steps = ctx.saved_tensors
        s = len(steps)
        n, c = steps[0].shape
        dev = steps[0].device
        lib = _lib.load()
        d = torch.empty((s, n, c), dtype=torch.float32, device=dev)
        g = grad.contiguous().float()
        head = (steps[0].data_ptr(), target.data_ptr(), weight.data_ptr() if weight is not None else None, n, c)
        tail = (ctx.ignore_index, ctx.mode, g.data_ptr(), sums.data_ptr(), d.data_ptr(), _call.stream(dev))
        if s == 1:
            _call.run(dev, lib.mtmc_cross_entropy_backward, *head, *tail)
        else:
            _call.run(dev, lib.mtmc_cross_entropy_steps_backward, *head, s, *tail)
        return (None, None, None, None) + d.unbind(0)


def cross_entropy(input, target, weight=None, reduction: str = "mean", ignore_index: int = -100):
    """Drop-in for `torch.nn.functional.cross_entropy(input, target, weight=weight, reduction=reduction)` with class
    indices as targets, for the [E, C<=4] float32 edge logits of the MPN."""
    _call.require_gpu("cross_entropy", input, target)
    if input.dim() != 2 or input.dtype != torch.float32 or input.shape[1] > 4 or target.shape != input.shape[:1]:
        raise NotImplementedError("mtmc_mpn.cross_entropy: input must be float32 [E, C<=4], target int64 [E]")
    if reduction not in _REDUCTIONS:
        raise ValueError(f"{reduction} is not a valid value for reduction")
    weight = _call.class_weight(weight, input.device, input.shape[1], "cross_entropy")
    return _CrossEntropy.apply(target.contiguous().long(), weight, _REDUCTIONS[reduction], int(ignore_index), input)


def cross_entropy_steps(steps, target, weight=None, reduction: str = "mean", ignore_index: int = -100):
    """`sum(cross_entropy(step, target, weight, reduction) for step in steps)` -- the training loop's loss over
    `outputs['classified_edges']` (reference train.py:118-138) -- in ONE pass when the steps are the consecutive slices
    of the logits block a forward of this package returns (4 launches instead of 4 per step); any other list of
    tensors is summed step by step."""
    steps = list(steps)
    if not steps:
        raise ValueError("cross_entropy_steps: no classified steps")
    if reduction not in ("mean", "sum"):
        raise ValueError("cross_entropy_steps: reduction must be 'mean' or 'sum'")
    s0 = steps[0]
    block = (s0.dim() == 2 and s0.dtype == torch.float32 and s0.is_cuda and target.is_cuda and s0.shape[1] <= 4
             and target.shape == s0.shape[:1] and _call.steps_block(steps))
    if not block or len(steps) == 1:
        return sum(cross_entropy(t, target, weight=weight, reduction=reduction, ignore_index=ignore_index) for t in steps)
    weight = _call.class_weight(weight, s0.device, s0.shape[1], "cross_entropy_steps")
    return _CrossEntropy.apply(target.contiguous().long(), weight, _REDUCTIONS[reduction], int(ignore_index), *steps)


def edge_confusion(logits, labels):
    """int64 tensor [TP, FP, TN, FN] (on the device) of `argmax(logits, 1) == 1` against 0/1 `labels`; e.g.
    FPR = FP / (FP + TN) as in train.py:100-102.  No host synchronisation."""
    _call.require_gpu("edge_confusion", logits, labels)
    if logits.dim() != 2 or logits.dtype != torch.float32 or not 2 <= logits.shape[1] <= 4 or labels.shape != logits.shape[:1]:
        raise NotImplementedError("mtmc_mpn.edge_confusion: logits must be float32 [E, 2..4], labels [E]")
    x, y = logits.contiguous(), labels.contiguous().long()
    out = torch.empty(4, dtype=torch.int64, device=x.device)
    _call.run(x.device, _lib.load().mtmc_edge_confusion, x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(),
              _call.stream(x.device))
    return out


EdgeLoss = collections.namedtuple("EdgeLoss", ["loss", "class_loss", "class_prob", "confusion", "fpr", "class_weight"])


class _EdgeLoss(torch.autograd.Function):
    """Consecutive [E, C] slices of one logits block, C in {1, 2}: 3 launches forward (memset, pass, finalize), 1 backward.
    gamma = 0 without `rows` is mtmc_edge_loss_*; anything else mtmc_edge_focal_*, the row loss q^gamma * l.  `rows`: one
    more output, the [S, E] weighted row losses (one more launch), and THEY are what is differentiable, through the per-row
    backward; the loss is not then."""

    @staticmethod
    def forward(ctx, target, weight, mode, fpr_alpha, gamma, rows, *steps):
        n, c = steps[0].shape
        s = len(steps)
        dev = steps[0].device
        lib = _lib.load()
        nbytes = lib.mtmc_edge_loss_scratch_bytes(s)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        record = torch.empty(_lib.EDGE_LOSS_RECORD, dtype=torch.float64, device=dev)
        out = torch.empty(3 + 5 * s, dtype=torch.float32, device=dev)
        confusion = torch.empty((s, 4), dtype=torch.int64, device=dev)
        per_row = torch.empty((s, n), dtype=torch.float32, device=dev) if rows else None
        args = (steps[0].data_ptr(), target.data_ptr(), n, c, s, mode, weight.data_ptr() if weight is not None else None,
                fpr_alpha, scratch.data_ptr(), nbytes, record.data_ptr(), out.data_ptr(), confusion.data_ptr())
        ctx.plain = gamma == 0.0 and not rows
        if ctx.plain:
            _call.run(dev, lib.mtmc_edge_loss_forward, *args, _call.stream(dev))
        else:
            _call.run(dev, lib.mtmc_edge_focal_forward, *args, gamma, per_row.data_ptr() if rows else None, _call.stream(dev))
        ctx.save_for_backward(target, record, *steps)
        ctx.gamma, ctx.rows = gamma, rows
        r = (out[0], out[3:3 + 2 * s].view(s, 2), out[3 + 2 * s:3 + 4 * s].view(s, 2), confusion, out[3 + 4 * s:], out[1:3])
        if rows:
            ctx.mark_non_differentiable(*r)
            return r + (per_row,)
        ctx.mark_non_differentiable(*r[1:])
        return r

    @staticmethod
    def backward(ctx, *grads):
        target, record, *steps = ctx.saved_tensors
        n, c = steps[0].shape
        dev = steps[0].device
        lib = _lib.load()
        d = torch.empty((len(steps), n, c), dtype=torch.float32, device=dev)
        g = (grads[6] if ctx.rows else grads[0]).contiguous().float()
        args = (steps[0].data_ptr(), target.data_ptr(), n, c, len(steps), g.data_ptr(), record.data_ptr(), d.data_ptr())
        if ctx.plain:
            _call.run(dev, lib.mtmc_edge_loss_backward, *args, _call.stream(dev))
        else:
            _call.run(dev, lib.mtmc_edge_focal_backward, *args, ctx.gamma, int(ctx.rows), _call.stream(dev))
        return (None,) * 6 + d.unbind(0)


def _edge_loss(steps, labels, weight, pos_weight, fpr_alpha, gamma, rows):
    """The checks and the call behind edge_loss and focal_loss: the six EdgeLoss fields, then the [S, E] rows if asked for."""
    steps = list(steps)
    if not steps:
        raise ValueError("edge_loss: no classified steps")
    gamma = float(gamma)
    if not 0.0 <= gamma < float("inf"):
        raise ValueError(f"mtmc_mpn.edge_loss: gamma must be finite and >= 0, got {gamma}")
    s0 = steps[0]
    if s0.dim() != 2 or s0.dtype != torch.float32 or s0.shape[1] not in (1, 2) or labels.shape != s0.shape[:1] \
            or any(t.shape != s0.shape or t.dtype != s0.dtype or t.device != s0.device for t in steps):
        raise NotImplementedError("mtmc_mpn.edge_loss: steps must be float32 [E, 1] or [E, 2] tensors of one shape, labels [E]")
    c = s0.shape[1]
    given, other, name = (weight, pos_weight, "weight") if c == 2 else (pos_weight, weight, "pos_weight")
    if other is not None:
        raise ValueError(f"mtmc_mpn.edge_loss: [E, {c}] logits take `{name}`, not `{'pos_weight' if c == 2 else 'weight'}`")
    if isinstance(given, str) and given != "balanced":
        raise ValueError(f"mtmc_mpn.edge_loss: {name} must be None, a tensor or 'balanced', got {given!r}")
    _call.require_gpu("edge_loss", s0, labels)
    if given is None:
        mode = _lib.EDGE_W_ONE
    elif isinstance(given, str):
        mode, given = _lib.EDGE_W_BALANCED, None
    else:
        mode = _lib.EDGE_W_GIVEN
        if not isinstance(given, torch.Tensor):
            given = torch.full((1,), float(given), dtype=torch.float32, device=s0.device)    # (a fill: capture-safe)
        given = given.detach().to(device=s0.device, dtype=torch.float32).contiguous().view(-1)
        if given.numel() != (2 if c == 2 else 1):
            raise ValueError(f"mtmc_mpn.edge_loss: {name} must have {2 if c == 2 else 1} element(s)")
    if not _call.steps_block(steps):
        steps = list(torch.stack(steps).unbind(0))           # autograd reaches the pieces through the stack
    return _EdgeLoss.apply(labels.contiguous().long(), given, mode, float(fpr_alpha), gamma, rows, *steps)


def edge_loss(steps, labels, weight=None, pos_weight=None, fpr_alpha: float = 0.0, gamma: float = 0.0):
    """The training / validation loops' `compute_loss_acc` (reference train.py:36-245) over `outputs['classified_edges']`
    in one pass over the logits block, without a host read (it can sit inside `capture_training_step`):

      C = 2 (CE / CE_weighted):  loss = sum_s F.cross_entropy(step_s, labels, weight) + fpr_alpha * sum_s FPR_s
          `weight`: None, a [2] tensor, or "balanced" = (1, n0/n1) from the label counts of this call (train.py:124-130)
      C = 1 (BCE / BCE_weighted): loss = sum_s F.binary_cross_entropy_with_logits(step_s[:, 0], labels, pos_weight=pw)
          + fpr_alpha * sum_s FPR_s;  `pos_weight`: None, a number, a one-element tensor, or "balanced" = n0/n1
      gamma > 0 (the config's `Focal`): every row loss l above becomes (1 - p_t)^gamma * l, p_t the probability of the
          true class; weights, the denominator of the mean and every other field are formed as before, and `class_loss`
          is the per-class mean of the focal rows.  gamma = 0 is the loss above, through the same kernels.

    "balanced" with an empty class falls back to (1, 1) (the reference divides by zero there).  `labels` [E]: int64 or the
    float 0/1 tensor the reference keeps; rows labelled neither 0 nor 1 count for nothing.  Returns the named tuple
    EdgeLoss(loss, class_loss [S,2], class_prob [S,2], confusion [S,4] = TP FP TN FN, fpr [S], class_weight [2]); only
    `loss` is differentiable (the FPR term has no gradient, as in the reference).  Steps that are the consecutive slices
    of one block (what a forward of this package returns) are used in place; any other list is stacked first."""
    return EdgeLoss(*_edge_loss(steps, labels, weight, pos_weight, fpr_alpha, gamma, False))


def focal_loss(input, target, gamma: float = 2.0, weight=None, pos_weight=None, reduction: str = "mean"):
    """Focal loss (Lin et al. 2017) of [E, 2] or [E, 1] float32 logits against 0/1 targets: what the `criterion` /
    `criterion_no_reduction` of the reference's `Focal` setting were meant to be (main_training.py:273-276; the class they
    name is commented out).  Row loss f = (1 - p_t)^gamma * CE resp. BCE-with-logits; w = `weight` ([E, 2]) or
    (1, `pos_weight`) ([E, 1]), each None, numbers or "balanced" as in `edge_loss`; rows labelled neither 0 nor 1 are skipped.

      "mean": `edge_loss([input], target, weight, pos_weight, gamma=gamma).loss`
      "sum" : sum_i w[y_i] f_i
      "none": the [E] tensor w[y_i] f_i, 0 on skipped rows

    With one logit, `0.9 * focal_loss(x, t, 5.0, reduction="none")` is the reference's `FocalLoss_binary(5, 0.9, 'none')`
    (utils.py:695-724).  Its `reduction='mean'` modulates the mean BCE, one scalar, instead of the rows; that form is not a
    focal loss and is not offered."""
    if reduction not in _REDUCTIONS:
        raise ValueError(f"{reduction} is not a valid value for reduction")
    r = _edge_loss([input], target, weight, pos_weight, 0.0, gamma, reduction != "mean")
    if reduction == "mean":
        return r[0]
    return r[6][0] if reduction == "none" else r[6].sum()


class FocalLoss(torch.nn.Module):
    """`focal_loss` as a module, for the `utils.FocalLoss(reduction=..., alpha=...)` calls of reference
    main_training.py:275-276.  `alpha`: None; "balanced"; a [2] tensor of class weights; or a number a, the class weights
    (1 - a, a) of Lin et al.  One-logit input has a single `pos_weight`, so weights (w0, w1) are passed there as
    pos_weight = w1 / w0 with the result scaled by w0 -- for a number a: pos_weight = a / (1 - a), times (1 - a), a < 1.
    (The reduction "mean" of one-logit input divides by the row count, as BCEWithLogitsLoss does, that of two-logit input
    by the sum of the rows' weights, as CrossEntropyLoss does.)"""

    def __init__(self, gamma: float = 2.0, alpha=None, reduction: str = "mean"):
        super().__init__()
        if not isinstance(alpha, (str, torch.Tensor)) and alpha is not None and not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"FocalLoss: alpha must lie in [0, 1], got {alpha}")
        self.gamma, self.alpha, self.reduction = float(gamma), alpha, reduction

    def forward(self, input, target):
        a, one = self.alpha, input.dim() == 2 and input.shape[1] == 1
        if a is None or isinstance(a, str):
            return focal_loss(input, target, self.gamma, **{"pos_weight" if one else "weight": a}, reduction=self.reduction)
        if isinstance(a, torch.Tensor):
            w = a.detach().to(input.device, torch.float32).view(2)
            if one:
                return w[0] * focal_loss(input, target, self.gamma, pos_weight=w[1:] / w[:1], reduction=self.reduction)
            return focal_loss(input, target, self.gamma, weight=w, reduction=self.reduction)
        a = float(a)
        if one:
            if a >= 1.0:
                raise ValueError("FocalLoss: one-logit input needs alpha < 1 (pos_weight = alpha / (1 - alpha))")
            return (1.0 - a) * focal_loss(input, target, self.gamma, pos_weight=a / (1.0 - a), reduction=self.reduction)
        w = torch.full((2,), a, dtype=torch.float32, device=input.device)           # (fills: capture-safe)
        w[:1].fill_(1.0 - a)
        return focal_loss(input, target, self.gamma, weight=w, reduction=self.reduction)


