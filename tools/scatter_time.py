"""Time the repeatable scatter forwards and the HIP grouping they reduce over, on one GPU, by the method of
tools/pool_time.py (every call captured into a HIP graph and replayed, device events, the median of `--rounds` windows of
`--reps` replays, spread = max - min; the calls alternate inside each round).

  scatter_add / scatter_mean / scatter_max at (E, N, C) = (150 454, 450, 32), (150 454, 450, 4), (10 M, 100 000, 32), the
  index row-sorted and shuffled, three ways:
      atomics         the default call (float atomics; the kernels of the commit before)
      deterministic   deterministic=True: grouping + segmented reduction
      grouped         deterministic=G: the grouping made beforehand
  the grouping alone at D = 37 844 / N = 450 and D = 15 237 / N = 430 (the two pool shapes) and at the three edge lists,
  against the torch formulation it replaced (where, stable sort, searchsorted)

--parent-tree DIR (a built checkout of the commit before): child processes of both builds in turn (parent, new, parent,
new) time what both have -- the default scatter calls, the plain pool calls and the index= forms of pool_tracklets -- and
the verdict is DESIGN.md 3.10's rule: the better process of each build, pass = new <= parent + max(3 %, parent's spread).

    python tools/scatter_time.py [--rounds 5] [--reps 50] [--parent-tree DIR] [--out profiles/scatter_grouped.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_time as pt  # noqa: E402  (the method; it also puts the tree to time, POOL_TIME_TREE or this one, on sys.path)

import mtmc_mpn  # noqa: E402
from mtmc_mpn import _lib, ops, pool  # noqa: E402

SHAPES = ((150454, 450, 32), (150454, 450, 4), (10_000_000, 100_000, 32))
POOL_GROUPINGS = ((37844, 450), (15237, 430))
OPS = ("scatter_add", "scatter_mean", "scatter_max")


def make_index(e, n, order, dev):
    gen = torch.Generator().manual_seed(e + n)
    index = torch.randint(0, n, (e,), generator=gen)
    return (index.sort().values if order == "sorted" else index).to(dev).contiguous()


def torch_grouping(index, n):
    """The formulation pool.group_by_index had before the HIP grouping."""
    key = torch.where((index >= 0) & (index < n), index, torch.full_like(index, n))
    key, perm = torch.sort(key, stable=True)
    return perm, torch.searchsorted(key, torch.arange(n + 1, dtype=torch.int64, device=index.device))


def shape_name(e, n, c):
    return f"E{e}_N{n}_C{c}"


def atomics_calls(dev, shapes):
    """name -> callable of the default scatter calls: what a child process times in either build."""
    calls, keep = {}, []
    for e, n, c in shapes:
        src = torch.randn((e, c), generator=torch.Generator().manual_seed(c)).to(dev)
        for order in ("sorted", "shuffled"):
            index = make_index(e, n, order, dev)
            keep.append((src, index))
            for name in OPS:
                calls[f"{shape_name(e, n, c)}/{order}/{name}/atomics"] = pt.no_grad(
                    lambda name=name, src=src, index=index, n=n: getattr(ops, name)(src, index, dim_size=n))
    return calls, keep


def pool_calls(dev, feat_dim):
    """The plain pool calls and the index= forms (forward, forward + backward) of both pool shapes."""
    calls = {}
    for shape, lengths in pt.shapes().items():
        n, d = int(lengths.size), int(lengths.sum())
        gen = torch.Generator().manual_seed(7)
        e = torch.randn((d, feat_dim), generator=gen).to(dev).requires_grad_()
        g = torch.randn((n, feat_dim), generator=gen).to(dev)
        w = torch.rand(d, generator=gen).add_(0.05).to(dev)
        off_dev = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
        seg = torch.repeat_interleave(torch.arange(n, device=dev), torch.tensor(lengths, device=dev), output_size=d)
        index = seg[torch.randperm(d, generator=gen).to(dev)].contiguous()
        for k, v in pt.plain_calls(e, g, off_dev).items():
            calls[f"pool/{shape}/{k}"] = v
        forms = {"index": lambda e=e, index=index, n=n: mtmc_mpn.pool_tracklets(e, index=index, num_tracklets=n, check=False),
                 "both": lambda e=e, index=index, n=n, w=w: mtmc_mpn.pool_tracklets(e, index=index, num_tracklets=n, weights=w,
                                                                                    check=False)}
        for name, fn in forms.items():
            calls[f"pool/{shape}/{name}/forward"] = pt.no_grad(fn)
            calls[f"pool/{shape}/{name}/forward_backward"] = (lambda fn=fn, e=e, g=g: torch.autograd.grad(fn(), e, g))
    return calls


def child(a, dev):
    """What both builds have, in one process that times nothing else."""
    out = {}
    for shape in SHAPES:                                   # (one shape at a time: the 10 M-row one is 1.3 GB of src)
        print("scatter_time: child,", shape_name(*shape), file=sys.stderr, flush=True)
        calls, keep = atomics_calls(dev, [shape])
        out.update(pt.measure(calls, dev, a.rounds, a.reps))
        del calls, keep
    out.update(pt.measure(pool_calls(dev, a.feat_dim), dev, a.rounds, a.reps))
    return out


def against_parent(a):
    def run(tree):
        env = dict(os.environ, POOL_TIME_TREE=os.path.abspath(tree))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--reps", str(a.reps),
               "--feat-dim", str(a.feat_dim)]
        return json.loads(subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout.splitlines()[-1])
    own = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    turns = [(who, run(tree)) for _ in range(2) for who, tree in (("parent", a.parent_tree), ("new", own))]
    verdict = {}
    for name in turns[0][1]:
        runs = {who: [t[name] for w, t in turns if w == who] for who in ("parent", "new")}
        old, new = (min(runs[who], key=lambda r: r["median"]) for who in ("parent", "new"))      # each build's better process
        allowed = old["median"] + max(0.03 * old["median"], old["spread"])
        verdict[name] = {"parent": old, "new": new, "allowed": round(allowed, 2), "pass": bool(new["median"] <= allowed)}
    return {"rule": "better process of each build; pass = new <= parent + max(3 %, parent's max - min)",
            "all_pass": all(v["pass"] for v in verdict.values()), "calls": verdict}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--feat-dim", type=int, default=2048, help="of the pool shapes")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the commit before")
    ap.add_argument("--child", action="store_true", help="time what every build has and print {call: times}")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scatter_time: needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    if a.child:
        print(json.dumps(child(a, dev)))
        return
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps,
              "unit": "us per call, median over the rounds; spread = max - min", "tile_rows": int(_lib.load().mtmc_group_tile_rows()),
              "scatter": {}, "grouping": {}}
    for e, n, c in SHAPES:
        print("scatter_time:", shape_name(e, n, c), file=sys.stderr, flush=True)
        src = torch.randn((e, c), generator=torch.Generator().manual_seed(c)).to(dev)
        calls = {}
        for order in ("sorted", "shuffled"):
            index = make_index(e, n, order, dev)
            made = mtmc_mpn.group_by_index(index, n)
            for name in OPS:
                fn = getattr(ops, name)
                want = fn(src, index, dim_size=n)
                got = fn(src, index, dim_size=n, deterministic=True)
                want, got = (want[0], got[0]) if isinstance(want, tuple) else (want, got)
                assert torch.allclose(got, want, rtol=1e-4, atol=1e-3), (e, n, c, order, name)    # the same result before timing
                head = f"{order}/{name}"
                calls[f"{head}/atomics"] = pt.no_grad(lambda fn=fn, index=index: fn(src, index, dim_size=n))
                calls[f"{head}/deterministic"] = pt.no_grad(lambda fn=fn, index=index: fn(src, index, dim_size=n, deterministic=True))
                calls[f"{head}/grouped"] = pt.no_grad(lambda fn=fn, made=made: fn(src, None, deterministic=made))
            calls[f"{order}/grouping/hip"] = lambda index=index: pool.group_by_index(index, n)
            calls[f"{order}/grouping/torch"] = lambda index=index: torch_grouping(index, n)
        times = pt.measure(calls, dev, a.rounds, a.reps)
        table = {}
        for k, v in times.items():
            order, name, way = k.split("/")
            table.setdefault(order, {}).setdefault(name, {})[way] = v
        for order in table:
            for name in OPS:
                row = table[order][name]
                row["deterministic_over_atomics"] = round(row["deterministic"]["median"] / row["atomics"]["median"], 3)
                row["grouped_over_atomics"] = round(row["grouped"]["median"] / row["atomics"]["median"], 3)
        result["scatter"][shape_name(e, n, c)] = dict(table, bytes={"src": e * c * 4, "index": e * 8, "out": n * c * 4})
        del calls, src
    for d, n in POOL_GROUPINGS:
        gen = torch.Generator().manual_seed(d)
        index = torch.randint(0, n, (d,), generator=gen).to(dev)
        perm, offsets = pool.group_by_index(index, n)
        want = torch_grouping(index, n)
        assert torch.equal(perm, want[0]) and torch.equal(offsets, want[1])
        times = pt.measure({"hip": lambda index=index, n=n: pool.group_by_index(index, n),
                            "torch": lambda index=index, n=n: torch_grouping(index, n)}, dev, a.rounds, a.reps)
        result["grouping"][f"D{d}_N{n}"] = dict(times, speedup=round(times["torch"]["median"] / times["hip"]["median"], 2))
    if a.parent_tree:
        result["against_parent"] = against_parent(a)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
