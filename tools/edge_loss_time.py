"""Time forward + backward of the edge loss on the config-3 shape (E = 172 954, S = 3, C = 2, about 2 % positives), three ways
in one process on one GPU:

  a  mtmc_mpn.edge_loss(weight="balanced", fpr_alpha=1)          loss + per-class losses / probabilities + counts + FPR
  b  mtmc_mpn.cross_entropy_steps(weight=w), w given             the loss only: computes less than (a); the floor
  c  the closest composition without a host read from the older ops: weights from labels.sum() on the device,
     cross_entropy_steps, one edge_confusion per step, per-class means by multiply-and-sum

Each way is timed twice with device events: the public ops with autograd, issued eagerly from Python (the host sets the pace
of such small kernels), and the same kernels through the C ABI on preallocated buffers, replayed as a HIP graph (the GPU's
own time; no autograd inside the capture).  The ways alternate inside every round; the figure
is the median over the rounds, the spread (max - min over the rounds, relative to the median) is printed for each.

    python tools/edge_loss_time.py [--rounds 15] [--reps 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtmc_mpn  # noqa: E402
from mtmc_mpn import _lib, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=172954)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_loss_time: needs a GPU (there is nothing to time without one)")
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    block = (torch.randn(a.steps, a.edges, 2, generator=g) * 3).to(dev).requires_grad_(True)
    labels = (torch.rand(a.edges, generator=g) < 0.02).long().to(dev)
    yf = labels.float()
    n1 = float(labels.sum())
    w_given = torch.tensor([1.0, (a.edges - n1) / n1], device=dev)
    lib, rc = _lib.load(), _lib.check
    e, s, wd = a.edges, a.steps, w_given.data_ptr()

    def steps():                                                # fresh views, as a forward hands them out
        return [block[i] for i in range(s)]

    # ---- the public ops with autograd, issued from Python
    def composition(ce_steps):
        """(c): everything but the loss itself is forward-only, as compute_loss_acc's metrics are"""
        with torch.no_grad():
            p1 = yf.sum()
            p0 = yf.numel() - p1
            w = torch.stack([torch.ones_like(p1), p0 / p1])
        loss = ce_steps(w)
        with torch.no_grad():
            extra = []
            for i in range(s):
                x = block.detach()[i]
                conf = ops.edge_confusion(x, labels).double()
                extra.append((conf[1] / (conf[1] + conf[2])).float())
                per = mtmc_mpn.cross_entropy(x, labels, reduction="none")
                prob = torch.softmax(x, 1)
                extra += [(per * yf).sum() / p1, (per * (1 - yf)).sum() / p0, (prob[:, 1] * yf).sum() / p1,
                          (prob[:, 0] * (1 - yf)).sum() / p0]
        return loss, extra

    eager = {
        "a_edge_loss": lambda: mtmc_mpn.edge_loss(steps(), labels, weight="balanced", fpr_alpha=1.0).loss,
        "b_cross_entropy_steps": lambda: mtmc_mpn.cross_entropy_steps(steps(), labels, weight=w_given),
        "c_composition": lambda: composition(lambda w: mtmc_mpn.cross_entropy_steps(steps(), labels, weight=w))[0],
    }

    def eager_run(fn):
        return lambda: torch.autograd.grad(fn(), block)

    # ---- the same kernels through the C ABI on preallocated buffers (no autograd), captured into a HIP graph
    nbytes = lib.mtmc_edge_loss_scratch_bytes(s)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    record = torch.empty(_lib.EDGE_LOSS_RECORD, dtype=torch.float64, device=dev)
    out = torch.empty(3 + 5 * s, dtype=torch.float32, device=dev)
    conf = torch.empty((s, 4), dtype=torch.int64, device=dev)
    sums = torch.empty(2 * _lib.STAT_REPLICAS, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    d = torch.empty_like(block)
    xp, yp = block.data_ptr(), labels.data_ptr()

    def stream():
        return torch.cuda.current_stream(dev).cuda_stream

    def raw_a():
        rc(lib.mtmc_edge_loss_forward(xp, yp, e, 2, s, _lib.EDGE_W_BALANCED, None, 1.0, scratch.data_ptr(), nbytes,
                                      record.data_ptr(), out.data_ptr(), conf.data_ptr(), stream()))
        rc(lib.mtmc_edge_loss_backward(xp, yp, e, 2, s, one.data_ptr(), record.data_ptr(), d.data_ptr(), stream()))

    def raw_b(w=None):
        w = wd if w is None else w.data_ptr()
        rc(lib.mtmc_cross_entropy_steps_forward(xp, yp, w, e, 2, s, -100, 0, sums.data_ptr(), loss.data_ptr(), stream()))
        rc(lib.mtmc_cross_entropy_steps_backward(xp, yp, w, e, 2, s, -100, 0, one.data_ptr(), sums.data_ptr(), d.data_ptr(),
                                                 stream()))

    raw = {"a_edge_loss": raw_a, "b_cross_entropy_steps": raw_b, "c_composition": lambda: composition(raw_b)}
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graphs, held = {}, []
    with torch.cuda.stream(side), torch.no_grad():
        for name, fn in raw.items():
            for _ in range(5):
                fn()
            side.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                held.append(fn())                               # (results stay alive as long as the graph)
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

    samples = {k + "/" + mode: [] for k in eager for mode in ("eager", "graph")}
    for _ in range(a.rounds):
        for name in eager:
            samples[name + "/eager"].append(timed(eager_run(eager[name])))
            samples[name + "/graph"].append(timed(graphs[name].replay))
    torch.cuda.synchronize()
    out = {"shape": {"E": a.edges, "S": a.steps, "C": 2, "positives": int(n1)}, "rounds": a.rounds, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "unit": "us per forward + backward"}
    for k, v in samples.items():
        med = statistics.median(v)
        out[k] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2),
                  "spread": round((max(v) - min(v)) / med, 4)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
