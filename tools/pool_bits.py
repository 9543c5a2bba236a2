"""pytest plugin: the sha256 of every output of the pooling and grouped-scatter raw calls that the tests make, in call order.

    PYTHONPATH=tools HASH_OUT=bits.txt python -m pytest -p pool_bits tests/test_gpu_pool_tracklets.py ... [MTMC_MPN_LIB=other.so]

One line per call of pool._forward_raw / _forward_weighted_raw (out, wsum, info), _backward_raw / _backward_weighted_raw (the
gradient), _weight_grad_raw and torch_ops._scatter_grouped (out, arg): index, function, sha256 over the outputs' bytes, their
dtypes and shapes.  Calls inside a graph capture are skipped (nothing to read until the replay).  Two libraries of one ABI
give equal files iff every output has the same bits (profiles/seg_walk_refactor_bits.txt was made this way)."""
import hashlib
import os

import torch

_lines = []


def _sha(ts):
    h = hashlib.sha256()
    shapes = []
    for t in ts:
        if isinstance(t, torch.Tensor):
            c = t.detach().contiguous().cpu()
            h.update(c.view(torch.uint8).numpy().tobytes() if c.numel() else b"")
            shapes.append(f"{str(c.dtype).replace('torch.', '')}{list(c.shape)}")
    return h.hexdigest(), " ".join(shapes)


def _wrap(mod, name, extra=()):
    fn = getattr(mod, name)

    def wrapped(*a, **k):
        r = fn(*a, **k)
        if torch.cuda.is_current_stream_capturing():       # a captured call: nothing to read until the replay
            return r
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode(0)
        try:
            return _record(r, k)
        finally:
            torch.cuda.set_sync_debug_mode(mode)

    def _record(r, k):
        torch.cuda.synchronize()
        outs = list(r) if isinstance(r, tuple) else [r]
        outs += [k[x] for x in extra if k.get(x) is not None]
        sha, shapes = _sha(outs)
        _lines.append(f"{len(_lines):05d} {name} {sha} {shapes}")
        return r
    setattr(mod, name, wrapped)


def pytest_configure(config):
    from mtmc_mpn import pool, torch_ops
    for n in ("_forward_raw", "_forward_weighted_raw"):
        _wrap(pool, n, ("info", "wsum"))
    for n in ("_backward_raw", "_backward_weighted_raw", "_weight_grad_raw"):
        _wrap(pool, n)
    _wrap(torch_ops, "_scatter_grouped")


def pytest_unconfigure(config):
    with open(os.environ["HASH_OUT"], "w") as f:
        f.write("\n".join(_lines) + "\n")
