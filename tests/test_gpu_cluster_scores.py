"""GPU: `mtmc_mpn.cluster_scores`, `edge_prf` and `evaluate` against the fp64 yardstick of tests/cluster_scores_ref.py.

Every cluster-score case compares the seven integer counts exactly and the nine scores at BAR = 1e-9 absolute (the five
scores lie in [-1, 1]; two independent fp64 CPU implementations, scikit-learn and the yardstick, differ by up to 1.4e-10 on
the fixture's case list, so a third one with the device's lgamma and another summation order has several times that
margin; what the bar cannot see -- a missed or double-counted node, cell or pair -- the exact counts catch).  With
MTMC_CS_ACCURACY_OUT=FILE the largest |GPU - yardstick| per score over the whole module is written there as JSON
(profiles/cluster_scores_accuracy.json is such a run)."""
import json
import os

import numpy as np
import pytest
import torch

import cluster_scores_ref as ref
import cs_cases
import mtmc_mpn

pytestmark = pytest.mark.gpu
BAR = 1e-9
WORST = dict.fromkeys(ref.NAMES, 0.0)
FIVE = ref.NAMES[:5]


@pytest.fixture(scope="module", autouse=True)
def accuracy_record():
    yield
    path = os.environ.get("MTMC_CS_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write(json.dumps({"bar": BAR, "largest_abs_difference": WORST, "device": torch.cuda.get_device_name(0)},
                               indent=1) + "\n")


def gpu_scores(t, p):
    """-> (the nine scores as a float64 numpy vector, the seven counts as a list), one read"""
    r = mtmc_mpn.cluster_scores(t, p)
    assert all(x.dim() == 0 and x.dtype == torch.float64 and x.is_cuda for x in r[:9])
    assert r.counts.dtype == torch.int64 and r.counts.shape == (7,)
    assert r.ari.untyped_storage().data_ptr() == r.emi.untyped_storage().data_ptr()      # views of one buffer
    return torch.stack(list(r[:9])).cpu().numpy(), r.counts.cpu().tolist()


def check(name, t, p, keys=ref.NAMES):
    """t, p: numpy int64 vectors; compares with the yardstick and returns (GPU scores by name, counts)"""
    want, want_counts = ref.cluster_scores_ref(t, p)
    got, counts = gpu_scores(torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda())
    got = dict(zip(ref.NAMES, (float(v) for v in got)))
    print(name, "counts", counts, {k: f"{got[k]:.17g} ({got[k] - want[k]:+.2e})" for k in ref.NAMES})
    assert counts == want_counts, (name, counts, want_counts)
    for k in keys:
        WORST[k] = max(WORST[k], abs(got[k] - want[k]))
        assert abs(got[k] - want[k]) <= BAR, (name, k, got[k], want[k])
    return got, counts


def test_degenerate_cases_and_their_exact_values():
    cases = cs_cases.degenerate_cases()
    got = {name: check(name, t, p) for name, (t, p) in cases.items()}
    five = lambda name: [got[name][0][k] for k in FIVE]
    assert five("n1") == [1.0] * 5 and got["n1"][1] == [1, 1, 1, 0, 0, 0, 0]
    assert five("one_cluster_both") == [1.0] * 5
    assert [got["one_cluster_both"][0][k] for k in ("entropy_true", "entropy_pred", "mi", "emi")] == [0.0] * 4
    assert five("singletons_both") == [1.0] * 5                      # identical partitions: exactly 1
    assert five("two_swapped") == [1.0] * 5
    assert five("one_vs_singletons") == [0.0, 0.0, 1.0, 0.0, 0.0]
    assert five("singletons_vs_one") == [0.0, 0.0, 0.0, 1.0, 0.0]
    assert got["independent_2x2"][0]["ari"] == -0.5 and got["independent_2x2"][0]["mi"] == 0.0
    assert got["emi_lower_bound"][1][:3] == [2, 2, 3]                # 7 + 8 - 10 = 5 > 1: the n_ij sum starts at 5


def test_label_values_are_arbitrary_int64():
    (ct, cp), (et, ep) = cs_cases.extreme_value_case()
    assert {cs_cases.I64_MIN, -1, 0, 7, cs_cases.I64_MAX} <= set(et.tolist()) and 3 * 1000 + 11 in et
    compact, compact_counts = check("values_compact", ct, cp)
    extreme, extreme_counts = check("values_extreme", et, ep)
    assert extreme == compact and extreme_counts == compact_counts      # bit for bit: the scores see the partition only
    # smaller integer types are read as int64
    r32 = gpu_scores(torch.from_numpy(ct).cuda().int(), torch.from_numpy(cp).cuda().to(torch.int16))
    assert dict(zip(ref.NAMES, r32[0].tolist())) == compact and r32[1] == compact_counts


@pytest.mark.parametrize("name", list(cs_cases.edge_cases()))
def test_wave_and_workgroup_edges(name):
    t, p = cs_cases.edge_cases()[name]
    check(name, t, p)


@pytest.mark.parametrize("n", [1, 64, 257])
def test_counts_with_one_two_and_n_distinct_labels(n):
    """counts[7] exactly at one node, one wave and one row past a workgroup, for every pairing of 1, 2 and n distinct labels
    on either side (n = 1: all the same partition)"""
    i = np.arange(n, dtype=np.int64)
    for kt in (1, 2, n):
        for kp in (1, 2, n):
            t, p = i % kt, (5 * i + 1) % kp                           # 5 is coprime to 64 and 257: kp = n gives a permutation
            assert len(set(t.tolist())) == min(kt, n) and len(set(p.tolist())) == min(kp, n)
            _, counts = check(f"n{n}_{kt}x{kp}", t, p)
            assert counts[:2] == [min(kt, n), min(kp, n)] and sum(counts[3:]) == n * (n - 1)


def test_full_tables_all_labels_distinct():
    g = np.random.default_rng(11)
    n = 4096
    t = g.permutation(n).astype(np.int64) * 7 - 9000
    p = g.permutation(n).astype(np.int64) - n // 2
    got, counts = check("all_distinct_4096", t, p)
    assert counts == [n, n, n, 0, 0, 0, n * (n - 1)] and [got[k] for k in FIVE] == [1.0] * 5


def test_two_labels_per_side_every_lane_on_the_same_counters():
    g = np.random.default_rng(12)
    t = g.integers(0, 2, size=4096, dtype=np.int64)
    p = np.where(g.random(4096) < 0.2, 1 - t, t).astype(np.int64) * (2 ** 62) - 5
    _, counts = check("two_labels_4096", t, p)
    assert counts[:3] == [2, 2, 4]


def test_pair_counts_past_int64_products():
    """n = 65 536, 2 x 3 clusters assigned at random (the true ones 30 : 70): the denominator of the adjusted Rand index is
    about 0.53 n^4, past 2^63"""
    g = np.random.default_rng(13)
    n = 65536
    t = (g.random(n) < 0.3).astype(np.int64)
    p = g.integers(0, 3, size=n, dtype=np.int64)
    _, counts = check("overflow_65536", t, p)
    tp, fp, fn, tn = counts[3:]
    assert tp + fp + fn + tn == n * (n - 1) and (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn) > 2 ** 63


def test_non_contiguous_inputs_are_read_in_place_and_left_alone():
    t, p = cs_cases.random_pair(2 * 300, 9, seed=21)
    want, want_counts = ref.cluster_scores_ref(t[::2], p[::2])
    dt, dp = torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda()
    keep_t, keep_p = dt.clone(), dp.clone()
    got, counts = gpu_scores(dt[::2], dp[::2])
    assert counts == want_counts
    for k, v in zip(ref.NAMES, got.tolist()):
        WORST[k] = max(WORST[k], abs(v - want[k]))
        assert abs(v - want[k]) <= BAR, (k, v, want[k])
    assert torch.equal(dt, keep_t) and torch.equal(dp, keep_p)
    again, _ = gpu_scores(dt[::2].contiguous(), dp[::2].contiguous())
    assert np.array_equal(again, got)


def test_refusals_on_device_tensors():
    a = torch.zeros(4, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError):
        mtmc_mpn.cluster_scores(a, a[:3])
    with pytest.raises(ValueError):
        mtmc_mpn.cluster_scores(a[:0], a[:0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        mtmc_mpn.cluster_scores(a, a.cpu())
    with pytest.raises(ValueError):
        mtmc_mpn.edge_prf(a.float(), a)


# ---- edge_prf ----------------------------------------------------------------------------------------------------

def check_prf(name, pred, labels):
    """pred: numpy int64, labels: numpy (int64 or float); against compute_P_R_F written out in fp64 (edge_prf_ref)"""
    want_counts, want = ref.edge_prf_ref(pred, labels)
    r = mtmc_mpn.edge_prf(torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda())
    assert r.confusion.dtype == torch.int64 and r.class_precision.shape == (2,) and r.f_score.dim() == 0
    got = [float(r.precision), float(r.recall), float(r.f_score)] + r.class_precision.cpu().tolist()
    print(name, r.confusion.cpu().tolist(), got)
    assert r.confusion.cpu().tolist() == want_counts, name
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * max(1.0, abs(w)), (name, got, want)
    return want_counts, got


def test_edge_prf_cases():
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    g = np.random.default_rng(31)
    assert check_prf("empty", i64([]), i64([])) == ([0, 0, 0, 0], [0.0] * 5)
    pred = g.integers(0, 2, size=1000, dtype=np.int64)
    c, out = check_prf("only_class_1", pred, np.ones(1000, dtype=np.int64))
    assert c[1] == c[2] == 0 and out[3] == 0.0 and out[0] == 1.0
    c, out = check_prf("only_class_0", pred, np.zeros(1000, dtype=np.int64))
    assert c[0] == c[3] == 0 and out[:3] == [0.0, 0.0, 0.0] and out[4] == 0.0
    labels = g.integers(0, 2, size=1000, dtype=np.int64)
    c, out = check_prf("no_positive_predicted", np.zeros(1000, dtype=np.int64), labels)
    assert c[0] == c[1] == 0 and out[:3] == [0.0, 0.0, 0.0] and out[3] == 100.0 and out[4] == 0.0
    skipped = labels.copy()
    skipped[::7] = -100
    c, _ = check_prf("rows_labelled_-100", pred, skipped)
    assert sum(c) == int((skipped >= 0).sum())
    check_prf("float_labels", pred, labels.astype(np.float32))
    e = 150454
    labels = (g.random(e) < 0.02).astype(np.float32)
    pred = np.where(g.random(e) < 0.01, 1 - labels, labels).astype(np.int64)
    check_prf("config3_shape", pred, labels)
    # any stride
    r = mtmc_mpn.edge_prf(torch.from_numpy(pred).cuda()[::3], torch.from_numpy(labels).cuda()[::3])
    assert r.confusion.cpu().tolist() == ref.edge_prf_ref(pred[::3], labels[::3])[0]


@pytest.mark.parametrize("e", [1, 63, 64, 65, 255, 256, 257, 256 * 256 + 1])
def test_edge_prf_at_wave_and_workgroup_edges(e):
    """Exact counts around one wave (64) and one workgroup (256), and one row past a full grid of 256 workgroups, where the
    grid-stride loop takes a second trip; rows whose label or prediction is neither 0 nor 1 are skipped."""
    g = np.random.default_rng(e)
    labels = (g.random(e) < 0.3).astype(np.int64)
    pred = np.where(g.random(e) < 0.2, 1 - labels, labels).astype(np.int64)
    labels[3::11] = -100
    pred[4::13] = 2
    counts, _ = check_prf(f"edge_e{e}", pred, labels)
    assert sum(counts) == int((((labels == 0) | (labels == 1)) & ((pred == 0) | (pred == 1))).sum())


# ---- evaluate ----------------------------------------------------------------------------------------------------

def _partition(ids):
    """cluster numbering by first occurrence: equal lists <=> equal partitions"""
    first = {}
    return [first.setdefault(int(v), len(first)) for v in ids]


def test_evaluate_on_a_three_camera_graph():
    g = np.random.default_rng(41)
    nodes = []                                                   # (camera, identity)
    for ident in range(13):
        cams = g.permutation(3)[:int(g.integers(2, 4))]
        nodes += [(int(c), ident) for c in cams]
    nodes += [(0, 99), (0, 99)]                                  # one identity twice inside camera 0 and nowhere else
    nodes += [(1, 200), (2, 201), (0, 202)]                      # seen once
    nodes.sort(key=lambda cn: cn[0])
    cams = np.array([c for c, _ in nodes])
    idents = np.array([i for _, i in nodes])
    n = len(nodes)
    assert 35 <= n <= 50
    feats = torch.randn(n, 2048, generator=torch.Generator().manual_seed(4)).cuda()
    graph = mtmc_mpn.build_graph(feats, cams, idents)
    ei = graph.edge_index.cpu().numpy()
    labels = graph.edge_labels.cpu().numpy()
    e = ei.shape[1]
    # about 5 % of the node pairs flipped, both directions alike
    where = {(int(u), int(v)): k for k, (u, v) in enumerate(ei.T)}
    pred = labels.astype(np.int64)
    for (u, v), k in where.items():
        if u < v and g.random() < 0.05:
            pred[k] = pred[where[(v, u)]] = 1 - pred[k]
    assert 0 < int((pred != labels).sum()) < e // 5
    predictions = torch.from_numpy(pred).cuda()
    id_pred = mtmc_mpn.postprocess(None, graph.edge_index, n, 3, cutting=False, pruning=False, splitting=False,
                                   preds_prob=predictions.float(), predictions=predictions).ID_pred
    keep = graph.edge_labels.clone()
    r = mtmc_mpn.evaluate(id_pred, predictions, graph.edge_index, graph.edge_labels, n)
    assert torch.equal(graph.edge_labels, keep) and torch.equal(predictions, torch.from_numpy(pred).cuda())
    # ID_GT: the partition a union-find over the label-1 edges gives
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for k in np.nonzero(labels == 1)[0]:
        parent[find(int(ei[0, k]))] = find(int(ei[1, k]))
    id_gt = r.ID_GT.cpu().numpy()
    assert _partition(id_gt) == _partition([find(i) for i in range(n)])
    twins = [i for i in range(n) if idents[i] == 99]
    assert len(twins) == 2 and id_gt[twins[0]] != id_gt[twins[1]]     # no edge inside a camera: two GT clusters
    want, want_counts = ref.cluster_scores_ref(id_gt, id_pred.cpu().numpy())
    got = dict(zip(ref.NAMES, torch.stack(list(r.clusters[:9])).cpu().tolist()))
    assert r.clusters.counts.cpu().tolist() == want_counts
    for k in ref.NAMES:
        WORST[k] = max(WORST[k], abs(got[k] - want[k]))
        assert abs(got[k] - want[k]) <= BAR, (k, got[k], want[k])
    assert r.edges.confusion.cpu().tolist() == ref.edge_prf_ref(pred, labels)[0]
    assert abs(float(r.edges.f_score) - ref.edge_prf_ref(pred, labels)[1][2]) <= 1e-12


# ---- capture -------------------------------------------------------------------------------------------------------

def test_captured_call_replays_on_new_labels():
    t0, p0 = cs_cases.random_pair(1025, 40, seed=51)
    t1, p1 = cs_cases.random_pair(1025, 300, seed=52, flip=0.5)
    t, p = torch.from_numpy(t0).cuda(), torch.from_numpy(p0).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mtmc_mpn.cluster_scores(t, p)                              # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            r = mtmc_mpn.cluster_scores(t, p)
    torch.cuda.current_stream().wait_stream(side)
    for a, b in ((t0, p0), (t1 * 1000003 - 17, p1), (t0, p0)):
        t.copy_(torch.from_numpy(a).cuda())                        # overwritten in place: the graph reads these buffers
        p.copy_(torch.from_numpy(b).cuda())
        graph.replay()
        torch.cuda.synchronize()
        fresh = mtmc_mpn.cluster_scores(t.clone(), p.clone())
        assert torch.equal(torch.stack(list(r[:9])), torch.stack(list(fresh[:9])))
        assert torch.equal(r.counts, fresh.counts)
    want, want_counts = ref.cluster_scores_ref(t0, p0)
    assert r.counts.cpu().tolist() == want_counts
