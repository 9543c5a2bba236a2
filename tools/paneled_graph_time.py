#!/usr/bin/env python3
"""Time of the paneled `build_graph` (`panel_rows=`, and by itself above 46 000 nodes) on one GPU, and of the existing
forms against another tree's library.

    python tools/paneled_graph_time.py forms   [--root TREE] [--rounds 5]      the four existing forms, S02 size and 8000 nodes
    python tools/paneled_graph_time.py ab      --other TREE [--processes 3]    `forms` in fresh processes, this tree and TREE
                                                                               alternating; median of the processes' medians
    python tools/paneled_graph_time.py panels  [--rounds 7]                    N = 8000, F = 2048, k = 32: the k call, the
                                                                               paneled call at P = auto and at P = 1024
    python tools/paneled_graph_time.py large                                   N = 100 000, F = 2048, 8 cameras, k = 50: the
                                                                               call, E_k, workspace, one eval forward

Figures are whole Python calls timed with HIP events, as in tools/knn_graph_time.py, whose `timed` / `compare` these are:
medians over alternating rounds, min .. max as the spread.  --root TREE imports `mtmc_mpn` from another checkout (one that
is built), so that the same tool times the parent commit's library and Python."""
import argparse
import copy
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _import(root):
    sys.path.insert(0, root)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import mtmc_mpn                                          # first: knn_graph_time puts its own tree in front
    import knn_graph_time
    assert os.path.abspath(mtmc_mpn.__path__[0]).startswith(os.path.abspath(root)), mtmc_mpn.__path__
    return mtmc_mpn, knn_graph_time


FORMS = [("s02", 4, None, 16, 2110, 300, 1000), ("8000", 8, 1000, 32, 36000, 1700, 100)]


def forms(args):
    """One line per (size, form): `name median min max`, for `ab` to read."""
    import numpy as np
    import torch
    mtmc_mpn, t = _import(args.root)
    from mtmc_mpn import graphs
    dev = torch.device("cuda:0")
    for name, n_cams, per_cam, k, span, gap, reps in FORMS:
        cams = np.repeat(np.arange(n_cams), graphs.S02_GT_CAMS if per_cam is None else per_cam)
        feats = torch.randn(cams.size, 2048, generator=torch.Generator().manual_seed(2)).to(dev)
        starts = torch.randint(0, span, (cams.size,), generator=torch.Generator().manual_seed(34)).numpy()
        gate = dict(start_frames=starts, max_gap=gap)
        variants = {"build_graph": lambda: mtmc_mpn.build_graph(feats, cams),
                    f"build_graph k={k}": lambda: mtmc_mpn.build_graph(feats, cams, k=k),
                    f"build_graph gap={gap}": lambda: mtmc_mpn.build_graph(feats, cams, **gate),
                    f"build_graph gap={gap} k={k}": lambda: mtmc_mpn.build_graph(feats, cams, k=k, **gate)}
        with torch.no_grad():
            res = t.compare(variants, reps, args.rounds, warmup=5)
        for v, (med, lo, hi) in res.items():
            print(f"{name:<5s} {v:<32s} {med:9.4f} {lo:9.4f} {hi:9.4f}", flush=True)


def ab(args):
    sides = {"this tree": ROOT, "other tree": os.path.abspath(args.other)}
    runs = {side: {} for side in sides}
    for _ in range(args.processes):
        for side, root in sides.items():                     # a fresh process each: nothing of one side lingers in the other
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "forms", "--root", root, "--rounds", str(args.rounds)],
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            for line in out.splitlines():
                *name, med, lo, hi = line.split()
                runs[side].setdefault(" ".join(name), []).append((float(med), float(lo), float(hi)))
    cell = lambda r: f"{statistics.median(m for m, _, _ in r):7.3f}  ({min(lo for _, lo, _ in r):.3f} .. {max(hi for _, _, hi in r):.3f})"
    lines = [f"{args.processes} processes of {args.rounds} rounds per side, alternating; ms per call: median of the processes' "
             f"medians (lowest min .. highest max)", f"{'':<40s}{'other tree':<28s}this tree"]
    for name in runs["this tree"]:
        lines.append(f"{name:<40s}{cell(runs['other tree'][name]):<28s}{cell(runs['this tree'][name])}")
        inside = min(lo for _, lo, _ in runs["other tree"][name]) <= statistics.median(m for m, _, _ in runs["this tree"][name]) \
            <= max(hi for _, _, hi in runs["other tree"][name])
        if not inside:
            lines[-1] += "   <- outside the other tree's min .. max"
    return lines


def panels(args):
    import numpy as np
    import torch
    mtmc_mpn, t = _import(ROOT)
    from mtmc_mpn import _lib
    lib = _lib.load()
    n, f, k = 8000, 2048, 32
    cams = np.repeat(np.arange(8), n // 8)
    feats = torch.randn(n, f, generator=torch.Generator().manual_seed(2)).cuda()
    auto = lib.mtmc_graph_panel_rows(n, f, 0)
    variants = {f"build_graph k={k}": lambda: mtmc_mpn.build_graph(feats, cams, k=k),
                f"build_graph k={k} panel_rows={auto} (auto: one panel, G formed once)":
                    lambda: mtmc_mpn.build_graph(feats, cams, k=k, panel_rows=auto),
                f"build_graph k={k} panel_rows=1024": lambda: mtmc_mpn.build_graph(feats, cams, k=k, panel_rows=1024)}
    with torch.no_grad():
        e_k = [fn().edge_index.shape[1] for fn in variants.values()]
        res = t.compare(variants, 50, args.rounds, warmup=5)
    assert len(set(e_k)) == 1
    lines = [f"N = {n}, F = {f}, k = {k}, 8 cameras, E_k = {e_k[0]}; workspace: k call {lib.mtmc_graph_knn_workspace_bytes(n, f)} "
             f"bytes, paneled auto {lib.mtmc_graph_paneled_workspace_bytes(n, f, k, 0)}, P = 1024 "
             f"{lib.mtmc_graph_paneled_workspace_bytes(n, f, k, 1024)}; {args.rounds} rounds of 50 calls"]
    lines += [f"    {v:<72s} {med:9.3f}  ({lo:.3f} .. {hi:.3f})" for v, (med, lo, hi) in res.items()]
    return lines


def large(args):
    import numpy as np
    import torch
    mtmc_mpn, t = _import(ROOT)
    from mtmc_mpn import _lib
    lib = _lib.load()
    n, f, k = 100000, 2048, 50
    cams = np.repeat(np.arange(8), n // 8)
    feats = torch.randn(n, f, generator=torch.Generator().manual_seed(2)).cuda()
    call = lambda: mtmc_mpn.build_graph(feats, cams, k=k)
    with torch.no_grad():
        times = [t.timed(call, 1, 1 if r == 0 else 0) for r in range(args.rounds)]
        g = call()
        e_k, pos = g.edge_index.shape[1], g.edge_pos
        ei = g.edge_index
        code = ei[0] * n + ei[1]
        symmetric = torch.equal(torch.sort(code).values, torch.sort(ei[1] * n + ei[0]).values)
        ordered = bool(torch.all(pos[1:] > pos[:-1]))
        params = mtmc_mpn.default_params(num_enc_steps=3, num_class_steps=1)
        torch.manual_seed(0)
        model = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, "resnet101").eval().cuda()
        fwd = [t.timed(lambda: model(g), 1, 1 if r == 0 else 0) for r in range(3)]
    return [f"N = {n}, F = {f}, 8 cameras, k = {k}: P = {lib.mtmc_graph_panel_rows(n, f, 0)}, workspace "
            f"{lib.mtmc_graph_paneled_workspace_bytes(n, f, k, 0)} bytes, E_k = {e_k} of {n * (n - n // 8)} all-pairs edges, "
            f"largest edge_pos {int(pos[-1])}, symmetric: {symmetric}, edge_pos increasing: {ordered}",
            f"    build_graph k={k} (whole call)      {statistics.median(times):9.1f}  ({min(times):.1f} .. {max(times):.1f}) ms, "
            f"{args.rounds} single calls",
            f"    MOTMPNet eval forward on it         {statistics.median(fwd):9.1f}  ({min(fwd):.1f} .. {max(fwd):.1f}) ms, 3 single calls"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["forms", "ab", "panels", "large"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--other", default=None)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    if args.what == "forms":
        return forms(args)
    lines = {"ab": ab, "panels": panels, "large": large}[args.what](args)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n\n")


if __name__ == "__main__":
    main()
