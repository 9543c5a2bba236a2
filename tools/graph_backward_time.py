#!/usr/bin/env python3
"""Time of the backward through `build_graph` on one GPU, beside torch autograd through the reference's own statements.

    python tools/graph_backward_time.py [--reps 200] [--out profiles/graph_backward_time.json]

Two sizes: S02 (450 nodes / 150 454 edges) and the config-3 training graph (430 nodes / 172 954 edges).  For each:
  (a) backward of mtmc_mpn.build_graph (mtmc_build_graph_backward), gradients of x and edge_attr both given;
  (b) torch autograd on the same device through normalize, two index gathers, pairwise_distance, cosine_similarity
      (reference train.py:316-342), the same gradients.
HIP events around `reps` backward calls after a warm-up of the same shape; the forward of each is outside the timed window
((a): one forward, its tape re-used with retain_graph; (b) likewise), so both figures are the backward alone.  The forward
times are reported beside them from windows of their own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mtmc_mpn  # noqa: E402
from mtmc_mpn import graphs  # noqa: E402


def cases():
    yield "s02", np.repeat(np.arange(4), graphs.S02_GT_CAMS), 2
    with open(os.path.join(ROOT, "tests", "golden", "train_tracklets.json")) as f:
        tr = json.load(f)["tracklets"]
    g = torch.Generator().manual_seed(3)                      # graphs.training_graph(tr, 100, 2048, 3): config 3
    ids = sorted({t[1] for t in tr})
    pick = [ids[i] for i in torch.randperm(len(ids), generator=g)[:100].tolist()]
    yield "config3_train", np.array([c for i in pick for (c, j) in sorted(tr) if j == i]), 1003


def timed(fn, reps, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def torch_statements(feats, row, col):
    x = F.normalize(feats, p=2, dim=0)
    a, b = x[row], x[col]
    return x, torch.stack([F.pairwise_distance(a, b), 1 - F.cosine_similarity(a, b)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": {}}
    for name, cams, seed in cases():
        feats = torch.randn(cams.size, 2048, generator=torch.Generator().manual_seed(seed)).to(dev)
        leaf = feats.clone().requires_grad_()
        g = mtmc_mpn.build_graph(leaf, cams)
        g_x, g_attr = torch.randn_like(g.x), torch.randn_like(g.edge_attr)
        ours = lambda: torch.autograd.grad([g.x, g.edge_attr], [leaf], [g_x, g_attr], retain_graph=True)
        leaf_t = feats.clone().requires_grad_()
        row, col = g.edge_index[0].contiguous(), g.edge_index[1].contiguous()
        x_t, attr_t = torch_statements(leaf_t, row, col)
        theirs = lambda: torch.autograd.grad([x_t, attr_t], [leaf_t], [g_x, g_attr], retain_graph=True)
        d_ours, d_theirs = ours()[0], theirs()[0]
        rec = {"nodes": int(cams.size), "edges": int(g.edge_attr.shape[0]),
               "max_abs_diff_vs_torch": (d_ours - d_theirs).abs().max().item(), "grad_abs_max": d_theirs.abs().max().item()}
        rounds = [(timed(ours, args.reps), timed(theirs, max(args.reps // 10, 5), warmup=3)) for _ in range(3)]   # alternating
        rec["backward_ms"] = sorted(r[0] for r in rounds)
        rec["torch_autograd_backward_ms"] = sorted(r[1] for r in rounds)
        with torch.no_grad():
            rec["forward_ms"] = timed(lambda: mtmc_mpn.build_graph(feats, cams), args.reps)
            rec["torch_forward_ms"] = timed(lambda: torch_statements(feats, row, col), max(args.reps // 10, 5), warmup=3)
        result["cases"][name] = rec
        del x_t, attr_t
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
