"""GPU tests of `build_graph(k=...)`: the cross-camera list thinned to a symmetric k-nearest list (`mtmc_build_graph_knn`).

The selection is checked EXACTLY against the rule's CPU restatement (tests/knn_ref.py) applied to the bits the dense call
wrote for the same input (l2norm=False: nothing in that path is summed in arbitrary order), and as a SET against the
independent oracle (oracle/graph_oracle.py + knn_ref) outside a margin band around each row's k-th key."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import graph_cases
import knn_ref
import mtmc_mpn
from golden_util import ARCH
from mtmc_mpn import _lib

pytestmark = pytest.mark.gpu

COS_EPS = 5e-6          # the cosine tolerance tests/test_gpu_graph_build.py::check grants the builder


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def feats_for(n, f, seed):
    """Seeded features, column-normalised on the host (what l2norm=True would do on the device)."""
    return F.normalize(torch.randn(n, f, generator=torch.Generator().manual_seed(seed)), p=2, dim=0)


def structure(g, cams, k, e_dense):
    """What every k list must satisfy, whatever it was compared against."""
    cams = np.asarray(cams)
    n = cams.size
    ei, pos = g.edge_index.cpu(), g.edge_pos.cpu()
    e_k = pos.numel()
    assert g.edge_index.shape == (2, e_k) and g.edge_index.dtype == torch.int64 and pos.dtype == torch.int64
    assert g.edge_attr.shape == (e_k, 2) and g.x.shape[0] == n
    assert e_k <= min(e_dense, 2 * k * n)
    if e_k == 0:
        return
    assert not g.edge_index.is_contiguous() or e_k == 1                 # the [E_k, 2].T view, as without k
    assert torch.all(pos[1:] > pos[:-1]) and int(pos[0]) >= 0 and int(pos[-1]) < e_dense
    assert not np.any(cams[ei[0].numpy()] == cams[ei[1].numpy()])        # cross-camera only
    code = ei[0] * n + ei[1]
    assert torch.equal(torch.sort(code).values, torch.sort(ei[1] * n + ei[0]).values)   # (i, j) kept <=> (j, i) kept


def exact(feats, cams, labels, k):
    """Dense call and k call on the same input, l2norm=False: edge_pos is the rule applied to the dense call's own bits, and
    every kept edge carries the dense call's bits.  A second k call gives the same bits."""
    dev = feats.cuda()
    dense = mtmc_mpn.build_graph(dev, cams, labels, l2norm=False)
    g = mtmc_mpn.build_graph(dev, cams, labels, l2norm=False, k=k)
    e_dense = dense.edge_index.shape[1]
    structure(g, cams, k, e_dense)
    want = knn_ref.select(dense.edge_attr[:, 1].cpu(), dense.edge_index.cpu(), cams, k)
    got = g.edge_pos.cpu()
    assert got.shape == want.shape and torch.equal(got, want), \
        f"k={k}: {got.numel()} kept, {want.numel()} expected"
    assert torch.equal(g.edge_index.cpu(), dense.edge_index.cpu()[:, want])
    assert torch.equal(bits(g.edge_attr), bits(dense.edge_attr)[want])
    assert torch.equal(bits(g.x), bits(dense.x))
    if labels is not None:
        assert torch.equal(bits(g.edge_labels), bits(dense.edge_labels)[want]) and torch.equal(g.y, dense.y)
    else:
        assert g.edge_labels is None and g.y is None
    again = mtmc_mpn.build_graph(dev, cams, labels, l2norm=False, k=k)
    for name in ("x", "edge_attr", "edge_index", "edge_pos"):
        a, b = getattr(g, name), getattr(again, name)
        assert a.shape == b.shape and (torch.equal(bits(a), bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)), name
    return g, dense


def labels_for(n, seed=3):
    return torch.randint(0, max(2, n // 3), (n,), generator=torch.Generator().manual_seed(seed)).numpy()


@pytest.mark.parametrize("k", [1, 2, 5, 6, 100])
def test_exact_nine_nodes(k):
    cams = np.repeat(np.array([1, 2, 3]), (3, 2, 4))
    g, dense = exact(feats_for(9, 64, 7), cams, labels_for(9), k)
    if k >= 6:                                                           # k >= n_out of cameras 1 and 3: the dense list
        assert g.edge_pos.numel() == 52 and torch.equal(g.edge_pos.cpu(), torch.arange(52))


def test_exact_two_nodes():
    g, _ = exact(feats_for(2, 64, 1), np.array([3, 7]), np.array([1, 1]), 1)
    assert g.edge_index.cpu().tolist() == [[0, 1], [1, 0]]


def test_exact_one_node_camera_and_out_degrees_around_a_wave():
    exact(feats_for(76, 64, 11), np.repeat(np.array([0, 1, 2]), (5, 1, 70)), None, 3)       # out-degrees 71, 75, 6


def test_exact_interleaved_cameras():
    """Training order (train.py:295-302): cameras interleave, so in_list position order is not node order."""
    perm = torch.randperm(62, generator=torch.Generator().manual_seed(4)).numpy()
    cams = np.repeat(np.array([0, 1, 2]), (20, 17, 25))[perm]
    assert np.any(np.diff(cams) < 0)
    exact(feats_for(62, 256, 12), cams, labels_for(62), 4)


@pytest.mark.parametrize("k", [7, 300])
def test_exact_rows_longer_than_one_sweep_fp32_gram(k):
    exact(feats_for(1100, 64, 13), np.repeat(np.array([0, 1, 2]), (300, 257, 543)), None, k)   # 961 <= N <= 1920: exact fp32


def test_exact_bf16x6_gram_without_bitwise_symmetry():
    exact(feats_for(2000, 64, 14), np.repeat(np.array([0, 1, 2]), (700, 650, 650)), None, 5)   # N >= 1921: bf16x6


@pytest.mark.parametrize("k", [1, 2])
def test_ties_go_to_the_lower_column(k):
    """Nodes 4, 5 (camera 1) and 9 (camera 2) carry one feature row, the nearest to node 0's: row 0 sees one key three times
    and admits the lowest k columns of the three."""
    cams = np.repeat(np.array([0, 1, 2]), (4, 4, 4))
    gen = torch.Generator().manual_seed(21)
    feats = torch.randn(12, 64, generator=gen)
    feats[4] = feats[0] + 0.01 * torch.randn(64, generator=gen)
    feats[5] = feats[4]
    feats[9] = feats[4]
    feats = F.normalize(feats, p=2, dim=1)
    g, dense = exact(feats, cams, None, k)
    d_ei, d_attr = dense.edge_index.cpu(), dense.edge_attr.cpu()
    row0 = {int(d_ei[1, e]): d_attr[e, 1].item() for e in range(d_ei.shape[1]) if int(d_ei[0, e]) == 0}
    assert row0[4] == row0[5] == row0[9]                                                 # a three-way tie
    assert all(row0[4] < v for j, v in row0.items() if j not in (4, 5, 9))               # and the row's minimum
    ei = g.edge_index.cpu()
    kept0 = {int(ei[1, e]) for e in range(ei.shape[1]) if int(ei[0, e]) == 0}
    # top_0 = {4} resp. {4, 5}; 9 never picks 0 (its own nearest are 4 and 5 at distance ~0), and at k = 1 neither does 5
    # (its nearest is 9), so what row 0 keeps of the three is top_0
    assert kept0 & {4, 5, 9} == ({4} if k == 1 else {4, 5})


# ---- against the independent oracle, l2norm=True ----

S02_CAMS = np.repeat(np.array([6, 7, 8, 9]), graph_cases.S02_GT_CAMS)


def s02_inputs(name):
    ids = torch.randint(0, 145, (S02_CAMS.size,), generator=torch.Generator().manual_seed(3)).numpy()
    if name == "gaussian":
        return torch.randn(S02_CAMS.size, 2048, generator=torch.Generator().manual_seed(2)), ids
    gen = torch.Generator().manual_seed(5)                  # the near-duplicate recipe of graph_cases.inputs("interleaved")
    base = {i: torch.randn(2048, generator=gen) for i in sorted(set(ids.tolist()))}
    return torch.stack([base[i] + 0.05 * torch.randn(2048, generator=gen) for i in ids.tolist()]), ids


@functools.lru_cache(maxsize=None)
def s02_oracle(name):
    from oracle import graph_oracle
    feats, ids = s02_inputs(name)
    return graph_oracle.build(feats, S02_CAMS, ids, True)


@pytest.mark.parametrize("name", ["gaussian", "near_duplicates"])
def test_against_the_oracle_outside_the_margin_band(name):
    k, n = 8, S02_CAMS.size
    feats, ids = s02_inputs(name)
    x_ref, ei_ref, attr_ref, lab_ref = s02_oracle(name)
    e_dense = ei_ref.shape[1]
    g = mtmc_mpn.build_graph(feats.cuda(), S02_CAMS, ids, k=k)
    structure(g, S02_CAMS, k, e_dense)

    d = attr_ref[:, 1].double().numpy()
    row = ei_ref[0].numpy()
    rank = knn_ref.ranks(attr_ref[:, 1], ei_ref)
    in_top = rank < k
    t_k = np.full(n, -np.inf)                                # the oracle's k-th and (k+1)-th key of every row
    t_k1 = np.full(n, np.inf)
    t_k[row[rank == k - 1]] = d[rank == k - 1]
    t_k1[row[rank == k]] = d[rank == k]
    ambiguous = np.where(in_top, d > t_k1[row] - 2 * COS_EPS, d < t_k[row] + 2 * COS_EPS)
    excluded = ambiguous | ambiguous[knn_ref.reverse_positions(ei_ref, n)]
    want = np.zeros(e_dense, dtype=bool)
    want[knn_ref.select(attr_ref[:, 1], ei_ref, S02_CAMS, k).numpy()] = True
    got = np.zeros(e_dense, dtype=bool)
    pos = g.edge_pos.cpu().numpy()
    got[pos] = True
    n_excl = int((excluded & want).sum())
    print(f"{name}: oracle keeps {int(want.sum())}, library keeps {int(got.sum())}, {n_excl} of the oracle's in the margin band, "
          f"{int((got != want).sum())} differ in all")
    assert n_excl <= 0.01 * want.sum()
    assert np.array_equal(got[~excluded], want[~excluded])

    both = torch.from_numpy(np.nonzero(got & want)[0])       # the shared edges: what the library wrote for them
    at = torch.from_numpy(np.searchsorted(pos, both.numpy()))
    assert torch.equal(g.edge_index.cpu()[:, at], ei_ref[:, both])
    assert torch.equal(g.edge_labels.cpu()[at], lab_ref[both])
    assert (g.x.cpu() - x_ref).abs().max().item() <= 1e-6 * max(1.0, x_ref.abs().max().item())
    err = (g.edge_attr.cpu()[at] - attr_ref[both]).abs().max(0).values
    assert err[0].item() <= 2e-5 * max(1.0, attr_ref[:, 0].abs().max().item()), f"distance err {err[0]:.2e}"
    assert err[1].item() <= COS_EPS, f"cosine err {err[1]:.2e}"


def test_k_list_feeds_the_mpn_and_postprocess():
    from oracle import graph_oracle, mpn_oracle
    cams = np.repeat(np.arange(3), (20, 17, 25))
    feats = torch.randn(cams.size, 2048, generator=torch.Generator().manual_seed(8))
    params = mtmc_mpn.default_params(num_enc_steps=2, num_class_steps=1)
    torch.manual_seed(0)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, ei, attr, _ = graph_oracle.build(feats, cams)
    g = mtmc_mpn.build_graph(feats.cuda(), cams, k=6)
    structure(g, cams, 6, ei.shape[1])
    pos = g.edge_pos.cpu()
    assert 0 < pos.numel() < ei.shape[1] and torch.equal(g.edge_index.cpu(), ei[:, pos])
    with torch.no_grad():
        want, _ = mpn_oracle.forward(sd, copy.deepcopy(params), ARCH, x, ei[:, pos], attr[pos])
        got, _ = m.cuda()(g)
    logits = got["classified_edges"][-1]
    assert (logits.cpu() - want["classified_edges"][-1]).abs().max().item() <= 1e-4
    pp = mtmc_mpn.postprocess(logits, g.edge_index, cams.size, 3)
    assert pp.ID_pred.shape == (cams.size,) and pp.ID_pred.dtype == torch.int64


@pytest.mark.parametrize("l2norm", [True, False])
def test_backward_through_the_kept_edges(l2norm):
    """A: bit for bit the dense build_graph's backward fed the same gradients scattered to their dense positions (zero
    elsewhere).  B: fp64 CPU autograd of the reference's statements on the kept edges, at the project's gradient bar
    (tests/test_gpu_graph_build_backward.py::meets_bar: |d| <= 1e-6 + 2e-4 |grad|max)."""
    perm = torch.randperm(62, generator=torch.Generator().manual_seed(4)).numpy()
    cams = np.repeat(np.array([0, 1, 2]), (20, 17, 25))[perm]
    feats = torch.randn(62, 256, generator=torch.Generator().manual_seed(16))
    leaf = feats.cuda().requires_grad_()
    g = mtmc_mpn.build_graph(leaf, cams, None, l2norm, k=4)
    assert g.x.requires_grad and g.edge_attr.requires_grad
    assert not g.edge_index.requires_grad and not g.edge_pos.requires_grad
    pos = g.edge_pos
    gen = torch.Generator().manual_seed(11)
    g_x, g_attr = torch.randn(g.x.shape, generator=gen), torch.randn(g.edge_attr.shape, generator=gen)
    torch.autograd.backward([g.x, g.edge_attr], [g_x.cuda(), g_attr.cuda()])

    leaf_a = feats.cuda().requires_grad_()
    dense = mtmc_mpn.build_graph(leaf_a, cams, None, l2norm)
    assert 0 < pos.numel() < dense.edge_attr.shape[0]
    g_dense = torch.zeros_like(dense.edge_attr)
    g_dense[pos] = g_attr.cuda()
    torch.autograd.backward([dense.x, dense.edge_attr], [g_x.cuda(), g_dense])
    assert torch.equal(leaf.grad, leaf_a.grad)

    f64 = feats.double().requires_grad_()
    x = F.normalize(f64, p=2, dim=0) if l2norm else f64
    r, c = g.edge_index.cpu()[0], g.edge_index.cpu()[1]
    attr = torch.stack([F.pairwise_distance(x[r], x[c]), 1 - F.cosine_similarity(x[r], x[c])], dim=1)
    ((x * g_x.double()).sum() + (attr * g_attr.double()).sum()).backward()
    scale = f64.grad.abs().max().item()
    err = (leaf.grad.double().cpu() - f64.grad).abs().max().item()
    print(f"k list, l2norm={l2norm}: |dgrad| {err:.3e}, |grad|max {scale:.3e}")
    assert torch.isfinite(leaf.grad).all() and err <= 1e-6 + 2e-4 * scale


def test_refusals():
    feats = feats_for(9, 64, 7)
    cams = np.repeat(np.array([1, 2, 3]), (3, 2, 4))
    for bad in (0, -1, 2.5, "3", True):
        with pytest.raises(RuntimeError):
            mtmc_mpn.build_graph(feats.cuda(), cams, k=bad)
    with pytest.raises(RuntimeError):
        mtmc_mpn.build_graph(feats, cams, k=2)                           # CPU tensor
    g = mtmc_mpn.build_graph(feats.cuda(), np.zeros(9, dtype=int), k=2)   # one camera: no edges, as without k
    assert g.edge_index.shape == (2, 0) and g.edge_attr.shape == (0, 2) and g.edge_pos.shape == (0,)


def test_capacity_one_short_is_reported_and_nothing_is_written_past_it():
    """The C entry point with edge_capacity = E_k - 1: n_kept_out reports E_k > capacity, the first E_k - 1 edges are those
    of a full-sized call, and the word after each output buffer's capacity keeps its guard value."""
    from mtmc_mpn import graph_build
    cams = np.repeat(np.array([0, 1, 2]), (20, 17, 25))
    feats = feats_for(62, 64, 15).cuda()
    labels = torch.from_numpy(labels_for(62)).cuda()
    full = mtmc_mpn.build_graph(feats, cams, labels.cpu().numpy(), l2norm=False, k=3)
    e_k = full.edge_pos.numel()
    cap = e_k - 1
    tables = [torch.from_numpy(a).cuda() for a in graph_build.camera_tables(cams)[:5]]
    e_dense = int(tables[4][-1])
    lib = _lib.load()
    index = torch.full((cap + 1, 2), -7, dtype=torch.int64, device="cuda")
    attr = torch.full((cap + 1, 2), -7.0, dtype=torch.float32, device="cuda")
    elab = torch.full((cap + 1,), -7.0, dtype=torch.float32, device="cuda")
    pos = torch.full((cap + 1,), -7, dtype=torch.int64, device="cuda")
    n_kept = torch.zeros(1, dtype=torch.int64, device="cuda")
    x = torch.empty_like(feats)
    ws = torch.empty(lib.mtmc_graph_knn_workspace_bytes(62, 64) + 256, dtype=torch.uint8, device="cuda")
    rc = lib.mtmc_build_graph_knn(feats.data_ptr(), feats.stride(0), 62, 64, 0, *[t.data_ptr() for t in tables], 3, e_dense,
                                  labels.data_ptr(), x.data_ptr(), index.data_ptr(), attr.data_ptr(), elab.data_ptr(),
                                  3, cap, pos.data_ptr(), n_kept.data_ptr(), ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert n_kept.item() == e_k > cap                                    # the capacity error, in the status word
    assert index[cap].tolist() == [-7, -7] and attr[cap].tolist() == [-7.0, -7.0]
    assert elab[cap].item() == -7.0 and pos[cap].item() == -7
    assert torch.equal(pos[:cap], full.edge_pos[:cap]) and torch.equal(index[:cap].t(), full.edge_index[:, :cap])
    assert torch.equal(bits(attr[:cap]), bits(full.edge_attr[:cap])) and torch.equal(elab[:cap], full.edge_labels[:cap])
