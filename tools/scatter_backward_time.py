"""Time the three scatter backward ops against `g.index_select(0, index)` on one GPU, on two shapes:

  s02   E = 150 454 rows of C = 32 from N = 450 destinations, index = the rows of graphs.camera_graph()'s edge list
  10m   E = 10 M rows of C = 32 from N = 100 000 destinations, index = the (sorted) rows of graphs.stress_graph

  add / mean / max   torch.ops.mtmc_mpn.scatter_{add,mean,max}_backward(g, [arg,] index, E)
  index_select       g.index_select(0, index): the same bytes as the add backward, torch's kernel

Every formulation is captured into a HIP graph on a side stream and timed with device events over `--reps` replays after a
warm-up; the formulations alternate inside each of the `--rounds` repetitions.  The figure is the median over the repetitions,
the spread max - min over them.  Bytes per call are counted from the shapes: 4 C E written + 8 E of index read; g (4 C N) and,
for max, arg (8 C N) are re-read once per row of a destination, mostly from cache, and are listed apart.  GB/s = those bytes
over the median.  A shape whose bytes fit the 256 MB Infinity Cache is replayed out of it, so its rate is not an HBM rate.

    python tools/scatter_backward_time.py [--rounds 7] [--reps 20] [--out profiles/scatter_backward_time.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtmc_mpn  # noqa: E402,F401
from mtmc_mpn import graphs  # noqa: E402

INFINITY_CACHE_MB = 256


def shapes(dev):
    cam_of_node = torch.repeat_interleave(torch.arange(len(graphs.S02_GT_CAMS)), torch.tensor(graphs.S02_GT_CAMS))
    yield "s02", graphs.camera_edge_index(cam_of_node)[0].contiguous().to(dev), 450
    yield "10m", graphs.stress_graph(100_000, 5_000_000, device=dev, with_features=False).edge_index[0].contiguous(), 100_000


def timed(run, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        run()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps                     # us per call


def capture(fn, dev):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            held = fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    return graph, held


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scatter_backward_time: needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    c = a.cols
    result = {"device": torch.cuda.get_device_name(0), "cols": c, "rounds": a.rounds, "reps": a.reps,
              "unit": "us per call (HIP-graph replay), median over the rounds; spread = max - min", "shapes": {}}
    for shape, index, n in shapes(dev):
        e = index.numel()
        gen = torch.Generator().manual_seed(7)
        g = torch.randn((n, c), generator=gen).to(dev)
        src = torch.randn((e, c), generator=torch.Generator(device=dev).manual_seed(8), device=dev)
        arg = torch.ops.mtmc_mpn.scatter_max(src, index, 0, n)[1]
        del src
        ops = torch.ops.mtmc_mpn
        forms = {"add": lambda: ops.scatter_add_backward(g, index, e),
                 "mean": lambda: ops.scatter_mean_backward(g, index, e),
                 "max": lambda: ops.scatter_max_backward(g, arg, index, e),
                 "index_select": lambda: g.index_select(0, index)}
        assert torch.equal(forms["add"](), forms["index_select"]())      # the same thing, before anything is timed
        runs = {k: capture(fn, dev) for k, fn in forms.items()}
        for graph, _ in runs.values():                           # warm-up of what the timed window uses
            for _ in range(5):
                graph.replay()
        torch.cuda.synchronize()
        samples = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, (graph, _) in runs.items():
                samples[k].append(timed(graph.replay, a.reps))
        torch.cuda.synchronize()
        stream = 4 * c * e + 8 * e
        table = {}
        for k, v in samples.items():
            med = statistics.median(v)
            table[k] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2),
                        "spread": round(max(v) - min(v), 2), "GBs": round(stream / (med * 1e-6) / 1e9, 1)}
        ours, torchs = table["add"], table["index_select"]
        margin = ours["median"] - torchs["median"]
        result["shapes"][shape] = {
            "E": e, "N": n, "stream_bytes": stream, "g_bytes": 4 * c * n, "arg_bytes": 8 * c * n,
            "fits_infinity_cache": bool(stream + 12 * c * n <= INFINITY_CACHE_MB * 2 ** 20),
            "times": table,
            "add_vs_index_select": {"add_minus_index_select_us": round(margin, 2), "ratio": round(ours["median"] / torchs["median"], 3),
                                    "slower_by_more_than_the_spread": bool(margin > max(ours["spread"], torchs["spread"]))}}
        del runs, forms
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
