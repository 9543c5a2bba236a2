"""Time `mtmc_mpn.idf1` piece by piece, at two shapes in one process on one GPU:

  s02    the 20 956 rows of the S02 ground truth (tests/golden/idf1_cases.npz) against the perturbed copy the tests use
         (5 % of the rows dropped, boxes jittered, 10 identities merged, 10 split): 7 435 groups of 2.8 rows on average
  large  synthetic: 40 cameras x 2 000 frames x 25 rows per (camera, frame), 2 M rows a side in 80 000 groups, 500
         identities that live 100 frames each, plus one crowded group of 300 x 300 rows

Per shape: the grouping in torch plus every pass (one `_id_passes`), then the filter pass, the overlap pass and the cell
compaction alone -- device events around `--reps` calls, the median of `--rounds` windows after a warm-up; then the two
host reads and `mtmc_id_assign` on the host (wall clock, median of 5), and one whole `idf1` call with a synchronise.  For
s02 the numpy yardstick (tests/idf1_ref.py) is timed once on the same host, the only other implementation there is.
A record, not a gate.

    python tools/idf1_time.py [--rounds 20] [--reps 5] [--out profiles/idf1_time.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mtmc_mpn  # noqa: E402
from mtmc_mpn import _call, _lib, metrics  # noqa: E402
import idf1_cases  # noqa: E402
import idf1_ref  # noqa: E402


def large_tables(seed=3):
    g = np.random.default_rng(seed)
    cams, frames, slots = 40, 2000, 25
    cam, frame, slot = np.meshgrid(np.arange(cams), np.arange(frames), np.arange(slots), indexing="ij")
    cam, frame, slot = cam.ravel(), frame.ravel(), slot.ravel()
    ident = frame // 100 * slots + slot
    x, y = slot % 5 * 380 + frame % 100 * 2, slot // 5 * 210 + g.integers(0, 30, cam.size)
    gt = np.stack([cam, ident, frame, x, y, np.full(cam.size, 120), np.full(cam.size, 90)], axis=1).astype(np.int64)
    crowd = np.stack([np.full(300, 40), 1000 + np.arange(300), np.zeros(300, dtype=np.int64), g.integers(0, 1800, 300),
                      g.integers(0, 1000, 300), g.integers(40, 200, 300), g.integers(40, 200, 300)], axis=1)
    crowd2 = crowd.copy()
    crowd2[:, 0] = 41                                   # (so that the crowd's identities have two cameras)
    gt = np.concatenate([gt, crowd, crowd2])
    pred = gt.copy()
    pred[:, 3:5] += g.integers(-15, 16, size=(pred.shape[0], 2))
    swap = g.random(pred.shape[0]) < 0.03
    pred[swap, 1] = g.integers(0, 500, size=int(swap.sum()))
    return gt, pred[g.permutation(pred.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("idf1_time: needs a GPU (there is nothing to time without one)")
    dev = "cuda:0"
    lib = _lib.load()

    def timed(run):
        for _ in range(3):
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
        return {"median": round(med, 1), "min": round(min(samples), 1), "max": round(max(samples), 1)}

    def wall(run, n=5):
        samples = []
        for _ in range(n):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - w0) * 1e6)
        return round(statistics.median(samples), 1)

    def shape(gt, pred):
        dgt, dpred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
        args = (0.75, 2, True, None, None, None, None)
        r = metrics._id_passes(dgt, dpred, *args)
        cap = r.n_obj * r.n_hyp
        triples = torch.empty((cap, 3), dtype=torch.int32, device=dev)
        cells_call = lambda: _call.run(dev, lib.mtmc_id_cells, r.ws.data_ptr(), r.n_obj, r.n_hyp, triples.data_ptr(), cap,   # noqa: E731
                                       r.counters[2:3].data_ptr(), _call.stream(dev))
        cells_call()
        n_cells = int(r.counters[2])
        host = triples[:n_cells].cpu().numpy()
        host = np.ascontiguousarray(host[np.lexsort((host[:, 1], host[:, 0]))])
        idtp, match, stats = ctypes.c_int64(0), np.empty(r.n_obj, dtype=np.int32), np.zeros(3, dtype=np.int64)

        def assign():
            _lib.check(lib.mtmc_id_assign(host.ctypes.data, n_cells, r.n_obj, r.n_hyp, ctypes.addressof(idtp), match.ctypes.data,
                                          stats.ctypes.data))
        assign()
        got = mtmc_mpn.idf1(dgt, dpred)
        assert got.idtp == idtp.value
        return got, {
            "rows": [int(gt.shape[0]), int(pred.shape[0])], "groups": r.n_groups, "identities": [r.n_obj, r.n_hyp],
            "pairs": int(((r.gt.offsets[1:] - r.gt.offsets[:-1]) * (r.pred.offsets[1:] - r.pred.offsets[:-1])).sum()),
            "nonzero_cells": n_cells, "components_largest_rows_cols": stats.tolist(),
            "idf1": got.idf1, "idtp": got.idtp, "idfp": got.idfp, "idfn": got.idfn,
            "device_us": {
                "grouping_and_all_passes": timed(lambda: metrics._id_passes(dgt, dpred, *args)),
                "filter_pass": timed(lambda: metrics._id_filter(r.pred, r.n_cam, r.counters[1:2], None, None, None, 2, True)),
                "overlap_pass": timed(lambda: metrics._id_overlap(r, 0.75)),
                "cell_compaction": timed(cells_call),
                # the overlap pass with a threshold no pair meets (d >= 0): every pair tested, not one atomic add
                "overlap_pass_without_adds": timed(lambda: metrics._id_overlap(r, -1.0))},
            "host_us_median_of_5": {
                "read_counters": wall(lambda: r.counters.tolist()),
                "read_cells": wall(lambda: triples[:n_cells].cpu()),
                "assign": wall(assign),
                "whole_idf1_call": wall(lambda: mtmc_mpn.idf1(dgt, dpred))}}

    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "atomics": "plain, one per counting pair"}
    gt = idf1_cases.s02_table()
    pred = idf1_cases.s02_perturbed(gt)
    got, out["s02"] = shape(gt, pred)
    w0 = time.perf_counter()
    ref = idf1_ref.idf1(gt, pred)
    out["s02"]["numpy_yardstick_wall_s"] = round(time.perf_counter() - w0, 2)
    assert (ref.idtp, ref.idfp, ref.idfn, ref.idf1) == (got.idtp, got.idfp, got.idfn, got.idf1)
    _, out["large"] = shape(*large_tables())
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
