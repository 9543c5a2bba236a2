"""Time `mtmc_mpn.mot_scores` piece by piece, at the two shapes of tools/idf1_time.py in one process on one GPU:

  s02    the 20 956 rows of the S02 ground truth (tests/golden/idf1_cases.npz) against the perturbed copy the tests use
  large  synthetic (tools/idf1_time.py::large_tables): 2 M rows a side in 80 000 groups plus one crowded 300 x 300 group

Per shape: the grouping in torch plus the filter passes (one `_id_passes` without the overlap pass), the candidate pass
alone and the candidate pass with its sort -- device events around `--reps` calls, the median of `--rounds` windows after
a warm-up; then the read-back of the candidates and row keys and `mtmc_mot_walk` on the host (wall clock, median of 5),
one whole `mot_scores` call, one whole `idf1` call on the same inputs beside it, and one `tracking_summary`.  For s02 the
numpy yardstick (tests/mot_ref.py) is timed once on the same host.  A record, not a gate.

    python tools/mot_time.py [--rounds 20] [--reps 5] [--out profiles/mot_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mtmc_mpn  # noqa: E402
from mtmc_mpn import _lib, metrics  # noqa: E402
import idf1_cases  # noqa: E402
import idf1_time  # noqa: E402
import mot_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mot_time: needs a GPU (there is nothing to time without one)")
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
        r = metrics._id_passes(dgt, dpred, *args, "mot_scores", False)
        g, q = r.gt, r.pred
        pairs, dist = metrics._mot_pairs(r, 0.75)
        n_pairs = pairs.shape[0]
        cap = max(n_pairs, 1)
        raw, raw_d = torch.empty((cap, 3), dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.mtmc_mot_pairs_workspace_bytes(r.n_groups), dtype=torch.uint8, device=dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)

        def pass_alone(max_dist=0.75):
            metrics._call.run(dev, lib.mtmc_mot_pairs, g.boxes.data_ptr(), g.offsets.data_ptr(), None, g.n, q.boxes.data_ptr(),
                              q.offsets.data_ptr(), q.keep.data_ptr(), q.n, r.n_groups, max_dist, raw.data_ptr(), raw_d.data_ptr(),
                              cap, counter.data_ptr(), ws.data_ptr(), ws.numel(), metrics._call.stream(dev))

        host = lambda t: np.ascontiguousarray(t.cpu().numpy())                        # noqa: E731
        read = lambda: [host(t) for t in (pairs, dist, g.group, g.ident, g.perm, q.group, q.ident, q.keep)]   # noqa: E731
        hp, hd, gg, gi, gp, qg, qi, qk = read()
        counts, total = np.zeros(_lib.MOT_COUNTS, dtype=np.int64), ctypes.c_double(0.0)
        match, stats = np.empty(max(g.n, 1), dtype=np.int32), np.zeros(3, dtype=np.int64)

        def walk():
            _lib.check(lib.mtmc_mot_walk(hp.ctypes.data, hd.ctypes.data, n_pairs, gg.ctypes.data, gi.ctypes.data, gp.ctypes.data,
                                         None, g.n, qg.ctypes.data, qi.ctypes.data, qk.ctypes.data, q.n, r.n_groups, r.n_obj,
                                         r.n_hyp, counts.ctypes.data, ctypes.addressof(total), match.ctypes.data,
                                         stats.ctypes.data))
        walk()
        got = mtmc_mpn.mot_scores(dgt, dpred)
        assert got.num_matches == counts[0] and got.num_switches == counts[1]
        return got, {
            "rows": [int(gt.shape[0]), int(pred.shape[0])], "groups": r.n_groups, "identities": [r.n_obj, r.n_hyp],
            "pairs": int(((g.offsets[1:] - g.offsets[:-1]) * (q.offsets[1:] - q.offsets[:-1])).sum()),
            "candidates": n_pairs, "groups_solved_largest_rows_cols": stats.tolist(),
            "mota": got.mota, "motp": got.motp, "matches": got.num_matches, "switches": got.num_switches,
            "misses": got.num_misses, "false_positives": got.num_false_positives, "fragmentations": got.num_fragmentations,
            "device_us": {
                "grouping_and_filter_passes": timed(lambda: metrics._id_passes(dgt, dpred, *args, "mot_scores", False)),
                "grouping_filter_and_overlap_passes": timed(lambda: metrics._id_passes(dgt, dpred, *args)),
                "candidate_pass": timed(pass_alone),
                # the candidate pass with a threshold no pair meets (d >= 0): every pair tested, nothing listed
                "candidate_pass_without_writes": timed(lambda: pass_alone(-1.0)),
                "candidate_pass_count_read_and_sort": timed(lambda: metrics._mot_pairs(r, 0.75))},
            "host_us_median_of_5": {
                "read_candidates_and_row_keys": wall(read),
                "walk": wall(walk),
                "whole_mot_scores_call": wall(lambda: mtmc_mpn.mot_scores(dgt, dpred)),
                "whole_idf1_call": wall(lambda: mtmc_mpn.idf1(dgt, dpred)),
                "whole_tracking_summary_call": wall(lambda: mtmc_mpn.tracking_summary(dgt, dpred))}}

    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps,
           "atomics": "integer, one counter add per wave and round of 1 024 pairs"}
    gt = idf1_cases.s02_table()
    pred = idf1_cases.s02_perturbed(gt)
    got, out["s02"] = shape(gt, pred)
    w0 = time.perf_counter()
    ref = mot_ref.mot_scores(gt, pred)
    out["s02"]["numpy_yardstick_wall_s"] = round(time.perf_counter() - w0, 2)
    assert all(getattr(ref, k) == getattr(got, k) for k in mot_ref.COUNTS) and ref.motp == got.motp
    _, out["large"] = shape(*idf1_time.large_tables())
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
