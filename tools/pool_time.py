"""Time `pool_tracklets` against the torch formulations a user has without it, on one GPU, on two shapes:

  scene   N = 450 tracklets, lengths from a fixed-seed log-normal clipped to [1, 3000], F = 2048
  batch   N = 430 tracklets, lengths uniform in 4..64 (a training batch), F = 2048

Formulations, forward and forward + backward (gradient of the embeddings for a given gradient of the means):

  pool_tracklets   mtmc_mpn.pool_tracklets(e, offsets=..., check=False), autograd through its HIP backward
  loop_mean_stack  the reference's loop: torch.stack([torch.mean(e[a:b], 0) for each tracklet])   (train.py:305-316)
  index_add        torch.zeros(N, F).index_add_(0, tracklet_of_row, e) / lengths[:, None]
  segment_reduce   torch.segment_reduce(e, "mean", lengths=..., axis=0, unsafe=True), if this torch build runs it on the GPU

Every formulation is captured into a HIP graph on a side stream (autograd included) and timed with device events over
`--reps` replays after a warm-up; the formulations alternate inside each of the `--rounds` repetitions.  The figure is the
median over the repetitions; the spread is max - min over them.  A formulation that cannot be captured is timed as issued
from Python instead and marked "eager".  Bytes per call are counted from the shapes: forward D F 4 read + N F 4 written
(the partial sums, at most 2 ceil(D / R) F 4 written and read back, are listed apart and not counted); backward N F 4 read
+ D F 4 written.  GB/s = those bytes over the median; `of_achievable` = that over the 6.3 TB/s the MI355X reaches on HBM
streams.  A shape whose bytes fit the 256 MB Infinity Cache is replayed out of it, so its rate is not an HBM rate.

    python tools/pool_time.py [--rounds 5] [--reps 50] [--only index_add,segment_reduce] [--out profiles/pool_tracklets.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtmc_mpn  # noqa: E402
from mtmc_mpn import pool  # noqa: E402

ACHIEVABLE_TBS = 6.3
INFINITY_CACHE_MB = 256


def shapes():
    rng = np.random.default_rng(2024)
    scene = np.clip(np.rint(rng.lognormal(mean=np.log(40.0), sigma=1.2, size=450)), 1, 3000).astype(np.int64)
    batch = rng.integers(4, 65, size=430).astype(np.int64)
    return {"scene": scene, "batch": batch}


def formulations(e, lengths, dev):
    """name -> forward callable e -> [N, F]; built once per shape (index tensors live on the device already)."""
    n, d = lengths.size, int(lengths.sum())
    bounds = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    off_dev = torch.tensor(bounds, dtype=torch.int64, device=dev)
    len_dev = torch.tensor(lengths, dtype=torch.int64, device=dev)
    len_f = len_dev.to(torch.float32)[:, None]
    seg = torch.repeat_interleave(torch.arange(n, device=dev), len_dev, output_size=d)
    f = e.shape[1]
    out = {
        "pool_tracklets": lambda x: mtmc_mpn.pool_tracklets(x, offsets=off_dev, check=False),
        "loop_mean_stack": lambda x: torch.stack([torch.mean(x[bounds[s]:bounds[s + 1]], 0) for s in range(n)]),
        "index_add": lambda x: torch.zeros((n, f), dtype=x.dtype, device=dev).index_add_(0, seg, x) / len_f,
    }
    if hasattr(torch, "segment_reduce"):
        out["segment_reduce"] = lambda x: torch.segment_reduce(x, "mean", lengths=len_dev, axis=0, unsafe=True)
    return out


def timed(run, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        run()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps                     # us per call


def capture(fn, dev):
    """fn replayed as a HIP graph, or None when it cannot be captured."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    try:
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                held = fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        return graph, held
    except Exception as ex:  # noqa: BLE001  (whatever the capture refuses: the formulation is then timed eagerly)
        torch.cuda.synchronize()
        print(f"pool_time: not captured ({type(ex).__name__}: {str(ex).splitlines()[0][:120]})", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feat-dim", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default=None, help="comma list of torch formulations to keep beside pool_tracklets")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_time: needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    f, r = a.feat_dim, pool.CHUNK_ROWS
    result = {"device": torch.cuda.get_device_name(0), "feat_dim": f, "chunk_rows": r, "rounds": a.rounds, "reps": a.reps,
              "unit": "us per call, median over the rounds; spread = max - min", "achievable_TBs": ACHIEVABLE_TBS, "shapes": {}}
    for shape, lengths in shapes().items():
        n, d = int(lengths.size), int(lengths.sum())
        gen = torch.Generator().manual_seed(7)
        e = torch.randn((d, f), generator=gen).to(dev).requires_grad_()
        g = torch.randn((n, f), generator=gen).to(dev)
        forms = formulations(e, lengths, dev)
        if a.only is not None:
            forms = {k: v for k, v in forms.items() if k == "pool_tracklets" or k in a.only.split(",")}
        # every formulation computes the same thing (any-order fp32 sums: a loose common tolerance) before anything is timed
        want = forms["pool_tracklets"](e.detach())
        want_grad = torch.autograd.grad(forms["pool_tracklets"](e), e, g)[0]
        skipped = []
        for name in list(forms):
            try:
                got = forms[name](e.detach())
                got_grad = torch.autograd.grad(forms[name](e), e, g)[0]
            except Exception as ex:  # noqa: BLE001  (segment_reduce without a GPU kernel in this build)
                skipped.append({"name": name, "why": f"{type(ex).__name__}: {str(ex).splitlines()[0][:120]}"})
                del forms[name]
                continue
            assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), name
            assert torch.allclose(got_grad, want_grad, rtol=1e-5, atol=1e-7), name
        runs = {}
        for name, fn in forms.items():
            fwd = (lambda fn=fn: fn(e.detach()))
            both = (lambda fn=fn: torch.autograd.grad(fn(e), e, g))
            for mode, call in (("forward", fwd), ("forward_backward", both)):
                cap = capture(call, dev)
                runs[(name, mode)] = (cap[0].replay, "graph", cap) if cap else (call, "eager", None)
        samples = {k: [] for k in runs}
        for k, (run, _, _) in runs.items():                      # warm-up of what the timed window uses
            for _ in range(5):
                run()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, (run, _, _) in runs.items():
                samples[k].append(timed(run, a.reps))
        torch.cuda.synchronize()
        bytes_fwd = d * f * 4 + n * f * 4
        bytes_bwd = n * f * 4 + d * f * 4
        nbytes = {"forward": bytes_fwd, "forward_backward": bytes_fwd + bytes_bwd}
        table = {}
        for (name, mode), v in samples.items():
            med = statistics.median(v)
            gbs = nbytes[mode] / (med * 1e-6) / 1e9
            table.setdefault(mode, {})[name] = {
                "median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2), "spread": round(max(v) - min(v), 2),
                "issued": runs[(name, mode)][1], "GBs": round(gbs, 1), "of_achievable": round(gbs / (ACHIEVABLE_TBS * 1e3), 4)}
        verdict = {}
        for mode, rows in table.items():
            ours = rows["pool_tracklets"]
            best = min((k for k in rows if k != "pool_tracklets"), key=lambda k: rows[k]["median"])
            margin = rows[best]["median"] - ours["median"]
            verdict[mode] = {"fastest_torch": best, "margin_us": round(margin, 2), "speedup": round(rows[best]["median"] / ours["median"], 2),
                             "faster_by_more_than_the_spread": bool(margin > max(ours["spread"], rows[best]["spread"]))}
        result["shapes"][shape] = {
            "N": n, "D": d, "longest": int(lengths.max()), "median_length": float(np.median(lengths)),
            "bytes": dict(nbytes, partials_at_most=2 * -(-d // r) * f * 4),
            "fits_infinity_cache": bool(nbytes["forward_backward"] <= INFINITY_CACHE_MB * 2 ** 20),
            "times": table, "verdict": verdict, "skipped": skipped}
        del runs
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
