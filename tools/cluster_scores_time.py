"""Time `mtmc_mpn.cluster_scores` and `mtmc_mpn.evaluate` with device events, at two sizes in one process on one GPU:

  s02    n = 450 nodes, E = 150 454 edges (the four S02 cameras of 124 / 90 / 99 / 137 tracklets, every cross-camera
         pair in both directions): the scene the benchmark runs; 200 identities
  large  n = 46 000 nodes in clusters of 1-6 (no edge list of that size: `cluster_scores` alone)

s02: 0.2 % of the node pairs have their prediction flipped (both directions alike) and ID_pred is what `postprocess`
makes of that; large: the predicted labels are the true ones with 5 % of the nodes moved.  Each figure is the median over `--rounds` timed windows
of `--reps` eager calls (a warm-up of every shape first); min, max and the spread (max - min over the median) are kept.
When scikit-learn is importable, its five scores are timed on the host on the same vectors (after the copy to the host;
wall clock, median of 5) and the largest difference to the device's is recorded.  A record, not a gate.

    python tools/cluster_scores_time.py [--rounds 20] [--reps 20] [--out profiles/cluster_scores_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtmc_mpn  # noqa: E402
from mtmc_mpn import graphs  # noqa: E402


def labels_in_groups(n, largest, seed):
    """n nodes in consecutive identities of 1..largest nodes, then 5 % of the nodes moved to a random identity"""
    g = np.random.default_rng(seed)
    sizes = g.integers(1, largest + 1, size=n)
    ids = np.repeat(np.arange(n), sizes)[:n].astype(np.int64)
    pred = ids.copy()
    moved = g.random(n) < 0.05
    pred[moved] = g.integers(0, int(ids.max()) + 1, size=int(moved.sum()))
    return ids, pred


def s02_graph(dev):
    """cross-camera edges in both directions of the S02 cameras, labelled by identity"""
    cams = np.repeat(np.arange(len(graphs.S02_GT_CAMS)), graphs.S02_GT_CAMS)
    g = np.random.default_rng(1)
    ident = g.integers(0, 200, size=450)
    u, v = np.nonzero(cams[:, None] != cams[None, :])
    edge_index = torch.from_numpy(np.stack([u, v])).to(dev)
    labels = torch.from_numpy((ident[u] == ident[v]).astype(np.float32)).to(dev)
    flip = np.triu(g.random((450, 450)) < 0.002, 1)
    flip = (flip | flip.T)[u, v]
    predictions = torch.from_numpy(np.where(flip, 1 - (ident[u] == ident[v]), ident[u] == ident[v]).astype(np.int64)).to(dev)
    return edge_index, labels, predictions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_scores_time: needs a GPU (there is nothing to time without one)")
    if a.rounds < 20:
        raise SystemExit("cluster_scores_time: at least 20 rounds")
    dev = "cuda:0"

    def timed(run):
        for _ in range(5):
            run()
        samples = []
        for _ in range(a.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                run()
            t1.record()
            t1.synchronize()
            samples.append(t0.elapsed_time(t1) * 1e3 / a.reps)
        med = statistics.median(samples)
        return {"median": round(med, 2), "min": round(min(samples), 2), "max": round(max(samples), 2),
                "spread": round((max(samples) - min(samples)) / med, 4)}

    def sklearn_side(t, p, got):
        try:
            from sklearn import metrics
        except ImportError:
            return None
        fns = (metrics.adjusted_rand_score, metrics.adjusted_mutual_info_score, metrics.homogeneity_score,
               metrics.completeness_score, metrics.v_measure_score)
        walls, want = [], None
        for _ in range(5):
            w0 = time.perf_counter()
            want = [float(f(t, p)) for f in fns]
            walls.append((time.perf_counter() - w0) * 1e6)
        return {"host_us_median_of_5": round(statistics.median(walls), 1),
                "largest_abs_difference_to_device": max(abs(x - y) for x, y in zip(want, got))}

    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "unit": "us per eager call"}

    # ---- s02: 450 nodes / 150 454 edges
    edge_index, labels, predictions = s02_graph(dev)
    n = 450
    id_pred = mtmc_mpn.postprocess(None, edge_index, n, len(graphs.S02_GT_CAMS), cutting=False, pruning=False, splitting=False,
                                   preds_prob=predictions.float(), predictions=predictions).ID_pred
    r = mtmc_mpn.evaluate(id_pred, predictions, edge_index, labels, n)
    got = torch.stack(list(r.clusters[:5])).cpu().tolist()
    out["s02"] = {
        "n": n, "E": int(edge_index.shape[1]), "clusters": r.clusters.counts[:3].cpu().tolist(),
        "cluster_scores": timed(lambda: mtmc_mpn.cluster_scores(r.ID_GT, id_pred)),
        "edge_prf": timed(lambda: mtmc_mpn.edge_prf(predictions, labels)),
        "evaluate": timed(lambda: mtmc_mpn.evaluate(id_pred, predictions, edge_index, labels, n)),
        "scikit_learn": sklearn_side(r.ID_GT.cpu().numpy(), id_pred.cpu().numpy(), got),
    }

    # ---- large: 46 000 labels
    t, p = labels_in_groups(46000, 6, seed=2)
    dt, dp = torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev)
    big = mtmc_mpn.cluster_scores(dt, dp)
    got = torch.stack(list(big[:5])).cpu().tolist()
    out["large"] = {"n": 46000, "clusters": big.counts[:3].cpu().tolist(),
                    "cluster_scores": timed(lambda: mtmc_mpn.cluster_scores(dt, dp)),
                    "scikit_learn": sklearn_side(t, p, got)}
    torch.cuda.synchronize()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
