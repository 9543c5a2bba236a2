"""Time forward + backward of the focal edge loss beside the plain one at S02 size (E = 150 454, S = 3, about 2 % positives),
in one process on one GPU:

  plain      mtmc_mpn.edge_loss(weight="balanced", fpr_alpha=1)
  focal2     ... gamma=2.0          (is an integer-gamma form worth having?)
  focal2.5   ... gamma=2.5          (powf on a non-integer exponent)
  torch      the same focal loss written in torch on the device, eager, loss only (no metrics, weights given): for scale

As tools/edge_loss_time.py: each way is timed with device events, the public ops with autograd issued eagerly from Python
(the host sets the pace of such small kernels) and -- the HIP ways -- the same kernels through the C ABI on preallocated
buffers, replayed as a HIP graph (the GPU's own time).  The ways alternate inside every round; the figure is the median
over the rounds, the spread (max - min over the rounds, relative to the median) is printed for each.

    python tools/focal_loss_time.py [--classes 2] [--rounds 15] [--reps 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtmc_mpn  # noqa: E402
from mtmc_mpn import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=150454)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--classes", type=int, default=2, choices=(1, 2))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("focal_loss_time: needs a GPU (there is nothing to time without one)")
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    e, s, c = a.edges, a.steps, a.classes
    block = (torch.randn(s, e, c, generator=g) * 3).to(dev).requires_grad_(True)
    labels = (torch.rand(e, generator=g) < 0.02).long().to(dev)
    n1 = float(labels.sum())
    w_given = torch.tensor([1.0, (e - n1) / n1], device=dev)
    wkw = dict(weight="balanced") if c == 2 else dict(pos_weight="balanced")
    lib, rc = _lib.load(), _lib.check

    def steps():                                                # fresh views, as a forward hands them out
        return [block[i] for i in range(s)]

    def torch_focal(gamma=2.0):
        total = 0.0
        for x in steps():
            if c == 2:
                ce = F.cross_entropy(x, labels, reduction="none")
                pt = torch.softmax(x, 1).gather(1, labels.view(-1, 1)).view(-1)
            else:
                ce = F.binary_cross_entropy_with_logits(x[:, 0], labels.float(), reduction="none")
                pt = torch.exp(-ce)
            wy = w_given[labels]
            total = total + (wy * (1 - pt) ** gamma * ce).sum() / (wy.sum() if c == 2 else e)
        return total

    eager = {
        "plain": lambda: mtmc_mpn.edge_loss(steps(), labels, fpr_alpha=1.0, **wkw).loss,
        "focal2": lambda: mtmc_mpn.edge_loss(steps(), labels, fpr_alpha=1.0, gamma=2.0, **wkw).loss,
        "focal2.5": lambda: mtmc_mpn.edge_loss(steps(), labels, fpr_alpha=1.0, gamma=2.5, **wkw).loss,
        "torch": torch_focal,
    }

    nbytes = lib.mtmc_edge_loss_scratch_bytes(s)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    record = torch.empty(_lib.EDGE_LOSS_RECORD, dtype=torch.float64, device=dev)
    out = torch.empty(3 + 5 * s, dtype=torch.float32, device=dev)
    conf = torch.empty((s, 4), dtype=torch.int64, device=dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    d = torch.empty_like(block)
    xp, yp = block.data_ptr(), labels.data_ptr()

    def stream():
        return torch.cuda.current_stream(dev).cuda_stream

    def raw_plain():
        rc(lib.mtmc_edge_loss_forward(xp, yp, e, c, s, _lib.EDGE_W_BALANCED, None, 1.0, scratch.data_ptr(), nbytes,
                                      record.data_ptr(), out.data_ptr(), conf.data_ptr(), stream()))
        rc(lib.mtmc_edge_loss_backward(xp, yp, e, c, s, one.data_ptr(), record.data_ptr(), d.data_ptr(), stream()))

    def raw_focal(gamma):
        def run():
            rc(lib.mtmc_edge_focal_forward(xp, yp, e, c, s, _lib.EDGE_W_BALANCED, None, 1.0, scratch.data_ptr(), nbytes,
                                           record.data_ptr(), out.data_ptr(), conf.data_ptr(), gamma, None, stream()))
            rc(lib.mtmc_edge_focal_backward(xp, yp, e, c, s, one.data_ptr(), record.data_ptr(), d.data_ptr(), gamma, 0,
                                            stream()))
        return run

    raw = {"plain": raw_plain, "focal2": raw_focal(2.0), "focal2.5": raw_focal(2.5)}
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graphs = {}
    with torch.cuda.stream(side), torch.no_grad():
        for name, fn in raw.items():
            for _ in range(5):
                fn()
            side.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                fn()
            graphs[name] = gr
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()

    def timed(run):
        for _ in range(20):
            run()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            run()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / a.reps               # us per forward + backward

    samples = {}
    for _ in range(a.rounds):
        for name, fn in eager.items():
            samples.setdefault(name + "/eager", []).append(timed(lambda: torch.autograd.grad(fn(), block)))
            if name in graphs:
                samples.setdefault(name + "/graph", []).append(timed(graphs[name].replay))
    torch.cuda.synchronize()
    res = {"shape": {"E": e, "S": s, "C": c, "positives": int(n1)}, "rounds": a.rounds, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "unit": "us per forward + backward"}
    for k, v in samples.items():
        med = statistics.median(v)
        res[k] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2),
                  "spread": round((max(v) - min(v)) / med, 4)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
