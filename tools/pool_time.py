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
    python tools/pool_time.py --weighted [--parent-tree DIR] --out profiles/pool_weighted.json     (weighted(), below)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

# (POOL_TIME_TREE: the built checkout whose package a --plain-only child times; default: the one this file lives in)
sys.path.insert(0, os.environ.get("POOL_TIME_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def measure(calls, dev, rounds, reps):
    """name -> {median, min, max, spread, issued} in us per call: every callable captured (else timed as issued), warmed up,
    then timed in turn inside each of the rounds."""
    runs = {}
    for name, call in calls.items():
        cap = capture(call, dev)
        runs[name] = (cap[0].replay, "graph", cap) if cap else (call, "eager", None)
    for run, _, _ in runs.values():
        for _ in range(5):
            run()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (run, _, _) in runs.items():
            samples[k].append(timed(run, reps))
    torch.cuda.synchronize()
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                "spread": round(max(v) - min(v), 2), "issued": runs[k][1]} for k, v in samples.items()}


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def plain_calls(e, g, off_dev):
    """The grouped call, forward and forward + backward: what --plain-only times in a library build of its own."""
    fn = lambda x: mtmc_mpn.pool_tracklets(x, offsets=off_dev, check=False)  # noqa: E731
    return {"plain/forward": no_grad(lambda: fn(e)), "plain/forward_backward": lambda: torch.autograd.grad(fn(e), e, g)}


def weighted(a, dev):
    """--weighted: the index / weights forms of one build against its own grouped call, against the torch formulations of the
    same results, and the grouped call against another built checkout (--parent-tree: child processes that time the
    grouped call alone, parent and this build in turn, twice).  The rows are frame-ordered: tracklets interleaved, each in its own order."""
    import subprocess
    f = a.feat_dim
    result = {"device": torch.cuda.get_device_name(0), "feat_dim": f, "rounds": a.rounds, "reps": a.reps,
              "unit": "us per call, median over the rounds; spread = max - min", "shapes": {}}

    def plain_run(tree):
        env = dict(os.environ, POOL_TIME_TREE=os.path.abspath(tree))
        cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--rounds", str(a.rounds), "--reps", str(a.reps),
               "--feat-dim", str(f)]
        return json.loads(subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()[-1])
    # the grouped call of both builds, each in processes of its own that time nothing else, in turn: parent, new, parent, new
    own = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    turns = [(who, plain_run(tree)) for _ in range(2) for who, tree in (("parent", a.parent_tree), ("new", own))] if a.parent_tree else []
    for shape, lengths in shapes().items():
        n, d = int(lengths.size), int(lengths.sum())
        gen = torch.Generator().manual_seed(7)
        e = torch.randn((d, f), generator=gen).to(dev).requires_grad_()              # grouped rows
        g = torch.randn((n, f), generator=gen).to(dev)
        w = torch.rand(d, generator=gen).add_(0.05).to(dev).requires_grad_()
        off_dev = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
        seg = torch.repeat_interleave(torch.arange(n, device=dev), torch.tensor(lengths, device=dev), output_size=d)
        index = seg[torch.randperm(d, generator=gen).to(dev)].contiguous()            # the frame-ordered assignment
        perm, _ = pool.group_by_index(index, n)
        mixed = torch.empty_like(e.detach())
        mixed[perm] = e.detach()                                                      # row perm[j] holds grouped row j
        mixed.requires_grad_()
        mixed_w = torch.empty_like(w.detach())
        mixed_w[perm] = w.detach()
        mixed_w.requires_grad_()
        counts = torch.tensor(lengths, dtype=torch.float32, device=dev)[:, None]
        zeros = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        forms = {          # name -> (ours, {torch formulation: fn}, the leaves the backward differentiates)
            "weights": (lambda: mtmc_mpn.pool_tracklets(e, offsets=off_dev, weights=w.detach(), check=False),
                        {"index_add": lambda: zeros(n, f).index_add_(0, seg, w.detach()[:, None] * e) /
                         zeros(n).index_add_(0, seg, w.detach())[:, None]}, (e,)),
            "index": (lambda: mtmc_mpn.pool_tracklets(mixed, index=index, num_tracklets=n, check=False),
                      {"index_add": lambda: zeros(n, f).index_add_(0, index, mixed) / counts,
                       "scatter_mean": lambda: mtmc_mpn.ops.scatter_mean(mixed, index, dim=0, dim_size=n),
                       "gather_then_plain": lambda: mtmc_mpn.pool_tracklets(mixed[pool.group_by_index(index, n)[0]], offsets=off_dev,
                                                                            check=False)}, (mixed,)),
            "both": (lambda: mtmc_mpn.pool_tracklets(mixed, index=index, num_tracklets=n, weights=mixed_w.detach(), check=False),
                     {"index_add": lambda: zeros(n, f).index_add_(0, index, mixed_w.detach()[:, None] * mixed) /
                      zeros(n).index_add_(0, index, mixed_w.detach())[:, None]}, (mixed,)),
            "both_d_weights": (lambda: mtmc_mpn.pool_tracklets(mixed, index=index, num_tracklets=n, weights=mixed_w, check=False),
                               {"index_add": lambda: zeros(n, f).index_add_(0, index, mixed_w[:, None] * mixed) /
                                zeros(n).index_add_(0, index, mixed_w)[:, None]}, (mixed, mixed_w)),
        }
        calls = plain_calls(e, g, off_dev)
        calls["grouping/forward"] = lambda: pool.group_by_index(index, n)
        skipped = []
        for name, (ours, others, leaves) in forms.items():
            want, want_grads = ours().detach(), torch.autograd.grad(ours(), leaves, g)
            for who, fn in dict(others, ours=ours).items():
                try:
                    got, got_grads = fn().detach(), torch.autograd.grad(fn(), leaves, g)
                except Exception as ex:  # noqa: BLE001  (a formulation this build does not run)
                    skipped.append({"name": f"{name}/{who}", "why": f"{type(ex).__name__}: {str(ex).splitlines()[0][:120]}"})
                    continue
                assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), (name, who)     # the same result before anything is timed
                for x, ref in zip(got_grads, want_grads):
                    assert torch.allclose(x, ref, rtol=1e-3, atol=1e-4), (name, who)
                calls[f"{name}/{who}/forward"] = no_grad(fn)
                calls[f"{name}/{who}/forward_backward"] = (lambda fn=fn, leaves=leaves: torch.autograd.grad(fn(), leaves, g))
        times = measure(calls, dev, a.rounds, a.reps)
        stream = {"forward": d * f * 4 + n * f * 4, "forward_backward": 2 * (d * f * 4 + n * f * 4)}
        extra = {"weights": d * 4 + n * 4, "index": d * 8, "both": d * 12 + n * 4}       # per pass, beside the stream
        table = {}
        for name in forms:
            for mode in ("forward", "forward_backward"):
                ours, base = times[f"{name}/ours/{mode}"], times[f"plain/{mode}"]
                others = {k.split("/")[1]: v for k, v in times.items() if k.startswith(name + "/") and k.endswith("/" + mode)
                          and "/ours/" not in k}
                best = min(others, key=lambda k: others[k]["median"])
                table[f"{name}/{mode}"] = {
                    "ours": ours, "torch": others, "fastest_torch": best, "speedup": round(others[best]["median"] / ours["median"], 2),
                    "over_plain": round(ours["median"] / base["median"], 3),
                    "beyond_spread_us": round(max(0.0, ours["median"] - base["median"] - max(ours["spread"], base["spread"])), 2)}
        result["shapes"][shape] = {
            "N": n, "D": d, "stream_bytes": stream, "plain": {m: times[f"plain/{m}"] for m in stream},
            "grouping": times["grouping/forward"], "forms": table, "skipped": skipped,
            "extra_compulsory_bytes_share": {k: round(v / stream["forward"], 5) for k, v in extra.items()}}
        del calls
    if a.parent_tree:
        for shape, rec in result["shapes"].items():
            verdict = {}
            for mode in rec["plain"]:
                runs = {who: [t[shape][f"plain/{mode}"] for w, t in turns if w == who] for who in ("parent", "new")}
                old, new = (min(runs[who], key=lambda r: r["median"]) for who in ("parent", "new"))   # each build's better process
                allowed = old["median"] + max(0.03 * old["median"], old["spread"])
                verdict[mode] = dict(runs, allowed=round(allowed, 2), **{"pass": bool(new["median"] <= allowed)})
            rec["against_parent"] = verdict
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feat-dim", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default=None, help="comma list of torch formulations to keep beside pool_tracklets")
    ap.add_argument("--out", default=None)
    ap.add_argument("--weighted", action="store_true", help="time the index= / weights= forms (profiles/pool_weighted.json)")
    ap.add_argument("--parent-tree", default=None, help="with --weighted: a built checkout of another commit to time the grouped call in")
    ap.add_argument("--plain-only", action="store_true", help="time the grouped call alone and print {shape: times}")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_time: needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    if a.plain_only or a.weighted:
        if a.plain_only:
            result = {}
            for shape, lengths in shapes().items():
                gen = torch.Generator().manual_seed(7)
                e = torch.randn((int(lengths.sum()), a.feat_dim), generator=gen).to(dev).requires_grad_()
                g = torch.randn((int(lengths.size), a.feat_dim), generator=gen).to(dev)
                off_dev = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
                result[shape] = measure(plain_calls(e, g, off_dev), dev, a.rounds, a.reps)
        else:
            result = weighted(a, dev)
        print(json.dumps(result))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
        return
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
