#!/usr/bin/env python3
"""Time of `build_graph(k=K)`, of the temporal gate and of both together beside the all-pairs `build_graph` on one GPU.

    python tools/knn_graph_time.py [--rounds 7] [--out profiles/knn_graph_time.txt]

Two sizes: (N, F, k) = (450, 2048, 16) with S02's camera split, and (8000, 2048, 32) over 8 equal cameras.  For each, the
all-pairs call, the k call, the gate-only call (`start_frames=, max_gap=`: starts uniform over 2110 frames with a gap of
300, resp. over 36000 frames with the reference's 1700) and the gate + k call; for the small one also `build_graph` + an
eval forward of MOTMPNet (num_enc_steps = 3) on the all-pairs and the k list.  Every figure is a whole Python call (a call
with k includes its one host read-back of E_k, a gated call its host count of the gated list), timed with HIP events
around `reps` calls after a warm-up of the same shape.  The variants alternate within a round; reported per variant: the
median of the rounds and their min .. max as the spread."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mtmc_mpn  # noqa: E402
from mtmc_mpn import graphs  # noqa: E402


def timed(fn, reps, warmup):
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


def compare(variants, reps, rounds, warmup):
    """{name: fn} -> {name: (median ms, min ms, max ms)} over `rounds` alternating rounds."""
    times = {name: [] for name in variants}
    for r in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, reps, warmup if r == 0 else 2))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(0)}; rounds: {args.rounds}; ms per call: median (min .. max)"]
    params = mtmc_mpn.default_params(num_enc_steps=3, num_class_steps=1)
    torch.manual_seed(0)
    model = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, "resnet101").eval().to(dev)
    cases = [("s02", np.repeat(np.arange(4), graphs.S02_GT_CAMS), 16, 2110, 300, 1000, True),
             ("8000 nodes, 8 cameras", np.repeat(np.arange(8), 1000), 32, 36000, 1700, 100, False)]
    for name, cams, k, span, gap, reps, with_forward in cases:
        feats = torch.randn(cams.size, 2048, generator=torch.Generator().manual_seed(2)).to(dev)
        starts = torch.randint(0, span, (cams.size,), generator=torch.Generator().manual_seed(34)).numpy()
        gate = dict(start_frames=starts, max_gap=gap)
        with torch.no_grad():
            dense, thin = mtmc_mpn.build_graph(feats, cams), mtmc_mpn.build_graph(feats, cams, k=k)
            e, e_k = dense.edge_index.shape[1], thin.edge_index.shape[1]
            del dense, thin
            e_g = mtmc_mpn.build_graph(feats, cams, **gate).edge_index.shape[1]
            e_gk = mtmc_mpn.build_graph(feats, cams, k=k, **gate).edge_index.shape[1]
            variants = {"build_graph": lambda: mtmc_mpn.build_graph(feats, cams),
                        f"build_graph k={k}": lambda: mtmc_mpn.build_graph(feats, cams, k=k),
                        f"build_graph gap={gap}": lambda: mtmc_mpn.build_graph(feats, cams, **gate),
                        f"build_graph gap={gap} k={k}": lambda: mtmc_mpn.build_graph(feats, cams, k=k, **gate)}
            if with_forward:
                variants["build_graph + forward"] = lambda: model(mtmc_mpn.build_graph(feats, cams))
                variants[f"build_graph k={k} + forward"] = lambda: model(mtmc_mpn.build_graph(feats, cams, k=k))
            res = compare(variants, reps, args.rounds, warmup=5)
        lines.append(f"{name}: N = {cams.size}, F = 2048, k = {k}, max_gap = {gap} of {span} frames, E = {e}, E_k = {e_k}, "
                     f"E_gated = {e_g}, E_gated_k = {e_gk}, reps per round = {reps}")
        for v, (med, lo, hi) in res.items():
            lines.append(f"    {v:<32s} {med:9.3f}  ({lo:.3f} .. {hi:.3f})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
