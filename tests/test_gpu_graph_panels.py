"""GPU tests of `build_graph(..., panel_rows=P)` and of `build_graph` beyond 46 000 nodes (`mtmc_build_graph_paneled`): the k
list and the gated list with the Gram matrix formed in row panels and the picks kept as lists.

Up to 46 000 nodes the paneled call is compared BIT FOR BIT with the same call without `panel_rows` (l2norm=False), whose
own exactness tests/test_gpu_graph_knn.py and tests/test_gpu_graph_gate.py establish; their helpers are borrowed.  Beyond
it there is no unpaneled call: the structure of the whole list is checked, and sampled rows against fp64 on the host."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gate_cases
import gate_ref
import knn_ref
import mtmc_mpn
from mtmc_mpn import _lib, graph_build
from test_gpu_graph_knn import COS_EPS, S02_CAMS, bits, feats_for, labels_for, s02_inputs, s02_oracle, structure

pytestmark = pytest.mark.gpu

FIELDS = ("x", "edge_index", "edge_attr", "edge_labels", "edge_pos", "y")


def same(a, b):
    """Two results of build_graph agree bit for bit, field by field, the edge count included."""
    assert a.edge_index.shape == b.edge_index.shape
    for name in FIELDS:
        u, v = getattr(a, name), getattr(b, name)
        assert (u is None) == (v is None), name
        if u is not None:
            assert u.shape == v.shape and u.dtype == v.dtype, name
            assert torch.equal(bits(u), bits(v)) if u.dtype == torch.float32 else torch.equal(u, v), name


def exact(feats, cams, labels, rows, k=None, starts=None, gap=None):
    """The call without panel_rows, the paneled call and the paneled call again, l2norm=False: all three the same bits."""
    dev = feats.cuda()
    kw = dict(l2norm=False, k=k, start_frames=starts, max_gap=gap)
    want = mtmc_mpn.build_graph(dev, cams, labels, **kw)
    got = mtmc_mpn.build_graph(dev, cams, labels, panel_rows=rows, **kw)
    same(got, want)
    same(mtmc_mpn.build_graph(dev, cams, labels, panel_rows=rows, **kw), got)
    e_dense = int(graph_build.camera_tables(cams)[4][-1])
    structure(got, cams, k if k is not None else len(cams), e_dense)
    return got


@pytest.mark.parametrize("rows", [1, 4, 9, 100])          # a panel per row, a ragged last panel, one panel, a clipped request
@pytest.mark.parametrize("k", [1, 2, 6])
def test_exact_nine_nodes(k, rows):
    g = exact(feats_for(9, 64, 7), np.repeat(np.array([1, 2, 3]), (3, 2, 4)), labels_for(9), rows, k)
    assert g.edge_pos.numel() == 52 if k == 6 else 0 < g.edge_pos.numel() < 52


def test_exact_interleaved_cameras():
    """In_list position order is not node order: a panel's rows lie all over the list, found through the inverse map."""
    perm = torch.randperm(62, generator=torch.Generator().manual_seed(4)).numpy()
    cams = np.repeat(np.array([0, 1, 2]), (20, 17, 25))[perm]
    assert np.any(np.diff(cams) < 0)
    exact(feats_for(62, 256, 12), cams, labels_for(62), 16, 4)


def test_exact_one_node_camera_and_a_panel_edge_inside_a_camera():
    exact(feats_for(76, 64, 11), np.repeat(np.array([0, 1, 2]), (5, 1, 70)), None, 64, 3)


@pytest.mark.parametrize("k", [1, 2])
def test_ties_go_to_the_lower_column(k):
    """The three-way tie of tests/test_gpu_graph_knn.py (nodes 4, 5 and 9 carry one feature row, the nearest to node 0's)."""
    cams = np.repeat(np.array([0, 1, 2]), (4, 4, 4))
    gen = torch.Generator().manual_seed(21)
    feats = torch.randn(12, 64, generator=gen)
    feats[4] = feats[0] + 0.01 * torch.randn(64, generator=gen)
    feats[5] = feats[4]
    feats[9] = feats[4]
    g = exact(F.normalize(feats, p=2, dim=1), cams, None, 5, k)
    ei = g.edge_index.cpu()
    kept0 = {int(ei[1, e]) for e in range(ei.shape[1]) if int(ei[0, e]) == 0}
    assert kept0 & {4, 5, 9} == ({4} if k == 1 else {4, 5})


def test_exact_split_k_whole_product_needs_the_panels_slab():
    exact(feats_for(150, 256, 17), np.repeat(np.array([0, 1, 2]), (50, 40, 60)), labels_for(150), 64, 4)


def test_exact_unsplit_whole_product_where_a_panel_alone_would_split():
    exact(feats_for(1100, 256, 18), np.repeat(np.array([0, 1, 2]), (300, 257, 543)), None, 256, 4)


@pytest.mark.parametrize("k", [7, 300])
def test_exact_rows_longer_than_one_sweep(k):
    exact(feats_for(1100, 64, 13), np.repeat(np.array([0, 1, 2]), (300, 257, 543)), None, 256, k)


def test_exact_bf16x6_whole_product_where_a_panel_alone_would_not_be():
    exact(feats_for(2000, 64, 14), np.repeat(np.array([0, 1, 2]), (700, 650, 650)), None, 512, 5)


# ---- the gate

@pytest.mark.parametrize("k", [None, 4])
@pytest.mark.parametrize("gap, kept_nothing", [(30, False), (1, True)])
def test_exact_gate_with_empty_rows_and_with_nothing_kept(gap, kept_nothing, k):
    cams, starts = gate_cases.interleaved()
    ei = gate_cases.dense_gate("interleaved")[0]
    pg = gate_ref.select(starts, ei, gap)
    per_row = np.bincount(ei[0, pg].numpy(), minlength=62)
    assert (pg.numel() == 0) == kept_nothing and (per_row == 0).sum() >= 10      # some rows have no candidate
    g = exact(feats_for(62, 256, 12), cams, labels_for(62), 16, k, starts, gap)
    if kept_nothing:
        assert g.edge_index.shape == (2, 0) and g.edge_attr.shape == (0, 2) and g.edge_pos.shape == (0,)
    elif k is None:
        assert torch.equal(g.edge_pos.cpu(), pg)
    else:
        assert 0 < g.edge_pos.numel() <= pg.numel()


def test_exact_s02_split_gate_then_k():
    cams, starts, gap, _ = gate_cases.COUNTS["s02"]
    g = exact(feats_for(450, 2048, 2), cams, None, 128, 8, starts, gap)
    assert g.edge_pos.numel() == 4374                                 # tests/test_gpu_graph_gate.py's figure


def test_backward_through_a_paneled_forward():
    cams, starts, gap, _ = gate_cases.COUNTS["interleaved"]
    feats = torch.randn(62, 256, generator=torch.Generator().manual_seed(16))
    grads = []
    for rows in (None, 16):
        leaf = feats.cuda().requires_grad_()
        g = mtmc_mpn.build_graph(leaf, cams, None, True, k=4, start_frames=starts, max_gap=gap, panel_rows=rows)
        assert g.x.requires_grad and g.edge_attr.requires_grad and not g.edge_pos.requires_grad
        gen = torch.Generator().manual_seed(11)
        g_x, g_attr = torch.randn(g.x.shape, generator=gen), torch.randn(g.edge_attr.shape, generator=gen)
        torch.autograd.backward([g.x, g.edge_attr], [g_x.cuda(), g_attr.cuda()])
        grads.append(leaf.grad)
    assert grads[0].abs().max().item() > 0 and torch.equal(bits(grads[0]), bits(grads[1]))


def test_capacity_one_short_is_reported_and_nothing_is_written_past_it():
    """tests/test_gpu_graph_knn.py's capacity test on the paneled C entry: edge_capacity = E_k - 1."""
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
    ws = torch.empty(lib.mtmc_graph_paneled_workspace_bytes(62, 64, 3, 16) + 256, dtype=torch.uint8, device="cuda")
    rc = lib.mtmc_build_graph_paneled(feats.data_ptr(), feats.stride(0), 62, 64, 0, *[t.data_ptr() for t in tables], 3, e_dense,
                                      labels.data_ptr(), x.data_ptr(), index.data_ptr(), attr.data_ptr(), elab.data_ptr(),
                                      None, 0, 3, 16, cap, pos.data_ptr(), n_kept.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert n_kept.item() == e_k > cap
    assert index[cap].tolist() == [-7, -7] and attr[cap].tolist() == [-7.0, -7.0]
    assert elab[cap].item() == -7.0 and pos[cap].item() == -7
    assert torch.equal(pos[:cap], full.edge_pos[:cap]) and torch.equal(index[:cap].t(), full.edge_index[:, :cap])
    assert torch.equal(bits(attr[:cap]), bits(full.edge_attr[:cap])) and torch.equal(elab[:cap], full.edge_labels[:cap])


def test_refusals():
    feats = feats_for(9, 64, 7)
    cams = np.repeat(np.array([1, 2, 3]), (3, 2, 4))
    dev = feats.cuda()
    for bad in (0, -1, 2.5, "3", True):
        with pytest.raises(RuntimeError, match="panel_rows"):
            mtmc_mpn.build_graph(dev, cams, k=2, panel_rows=bad)
    with pytest.raises(RuntimeError, match="panel_rows"):
        mtmc_mpn.build_graph(dev, cams, panel_rows=4)                                # neither k nor a gate
    with pytest.raises(RuntimeError, match="GPU"):
        mtmc_mpn.build_graph(feats, cams, k=2, panel_rows=4)                         # CPU tensor
    g = mtmc_mpn.build_graph(dev, np.zeros(9, dtype=int), k=2, panel_rows=4)        # one camera: no edges
    assert g.edge_index.shape == (2, 0) and g.edge_attr.shape == (0, 2) and g.edge_pos.shape == (0,)


# ---- l2norm=True: the device normalises; against the independent oracle outside the margin band

def test_against_the_oracle_outside_the_margin_band():
    """tests/test_gpu_graph_knn.py's comparison and bars, on its "gaussian" input, for the paneled call."""
    k, n = 8, S02_CAMS.size
    feats, ids = s02_inputs("gaussian")
    x_ref, ei_ref, attr_ref, lab_ref = s02_oracle("gaussian")
    e_dense = ei_ref.shape[1]
    g = mtmc_mpn.build_graph(feats.cuda(), S02_CAMS, ids, k=k, panel_rows=128)
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
    print(f"oracle keeps {int(want.sum())}, library keeps {int(got.sum())}, {n_excl} of the oracle's in the margin band, "
          f"{int((got != want).sum())} differ in all")
    assert n_excl <= 0.01 * want.sum()
    assert np.array_equal(got[~excluded], want[~excluded])

    both = torch.from_numpy(np.nonzero(got & want)[0])
    at = torch.from_numpy(np.searchsorted(pos, both.numpy()))
    assert torch.equal(g.edge_index.cpu()[:, at], ei_ref[:, both])
    assert torch.equal(g.edge_labels.cpu()[at], lab_ref[both])
    assert (g.x.cpu() - x_ref).abs().max().item() <= 1e-6 * max(1.0, x_ref.abs().max().item())
    err = (g.edge_attr.cpu()[at] - attr_ref[both]).abs().max(0).values
    assert err[0].item() <= 2e-5 * max(1.0, attr_ref[:, 0].abs().max().item()), f"distance err {err[0]:.2e}"
    assert err[1].item() <= COS_EPS, f"cosine err {err[1]:.2e}"


# ---- beyond the old limit: N = 46 080, no unpaneled call to compare with

BIG_N, BIG_F, BIG_K = 46080, 32, 4
BIG_CAMS = np.repeat(np.array([0, 1, 2]), (15000, 15080, 16000))


def big_feats():
    return F.normalize(torch.randn(BIG_N, BIG_F, generator=torch.Generator().manual_seed(31)), p=2, dim=0)


def test_beyond_the_old_limit_k_list_against_fp64_on_sampled_rows():
    feats = big_feats()
    g = mtmc_mpn.build_graph(feats.cuda(), BIG_CAMS, l2norm=False, k=BIG_K)
    e_dense = int(graph_build.camera_tables(BIG_CAMS)[4][-1])
    structure(g, BIG_CAMS, BIG_K, e_dense)
    assert torch.equal(bits(g.x), bits(feats))

    x = feats.double()
    rho = x.norm(dim=1).clamp_min(1e-8)
    ei = g.edge_index.cpu()
    first = torch.searchsorted(ei[0].contiguous(), torch.arange(BIG_N + 1))      # rows ascend with the camera blocks here

    def keys(i):                                              # fp64 cosine distance of row i to every cross-camera node
        d = 1 - (x @ x[i]) / (rho * rho[i])
        d[torch.from_numpy(BIG_CAMS == BIG_CAMS[i])] = float("inf")
        return d

    def top(i):                                               # (the first k by (key, column), the gap behind the k-th)
        d = keys(i)
        order = torch.from_numpy(np.lexsort((np.arange(BIG_N), d.numpy())))
        return set(order[:BIG_K].tolist()), (d[order[BIG_K]] - d[order[BIG_K - 1]]).item()

    p = _lib.load().mtmc_graph_panel_rows(BIG_N, BIG_F, 0)
    assert 128 <= p < BIG_N and p % 128 == 0                  # more than one panel
    sample = set(range(0, BIG_N, 1500)) | {BIG_N - 1, 14999, 15000, 30079, 30080}
    for edge in range(p, BIG_N, p):
        sample |= {edge - 1, edge}
    assert 35 <= len(sample) <= 60
    skipped, smallest = 0, float("inf")
    for i in sorted(sample):
        top_i, gap = top(i)
        smallest = min(smallest, gap)
        if gap <= 4 * COS_EPS:
            skipped += 1
            continue
        kept = set(ei[1, first[i]:first[i + 1]].tolist())
        assert top_i <= kept, (i, top_i - kept)
        for j in kept - top_i:
            assert i in top(j)[0], (i, j)
    print(f"{len(sample)} rows sampled, {skipped} skipped, smallest gap behind a k-th key {smallest:.2e}")
    assert skipped <= 0.1 * len(sample)

    r, c = ei[0], ei[1]
    dist = (x[r] - x[c] + 1e-6).norm(dim=1)
    cos = 1 - (x[r] * x[c]).sum(1) / (rho[r] * rho[c])
    attr = g.edge_attr.cpu().double()
    assert (attr[:, 0] - dist).abs().max().item() <= 2e-5 * max(1.0, dist.max().item())
    assert (attr[:, 1] - cos).abs().max().item() <= COS_EPS


def test_beyond_the_old_limit_gate_alone():
    span, gap = 10_000_000, 1000
    starts = torch.randint(0, span, (BIG_N,), generator=torch.Generator().manual_seed(32)).numpy()
    want = graph_build.gated_edge_count(BIG_CAMS, starts, gap)
    assert 100_000 <= want <= 900_000
    g = mtmc_mpn.build_graph(big_feats().cuda(), BIG_CAMS, l2norm=False, start_frames=starts, max_gap=gap)
    ei, pos = g.edge_index.cpu().numpy(), g.edge_pos.cpu()
    assert pos.numel() == want and g.edge_attr.shape == (want, 2)
    assert torch.all(pos[1:] > pos[:-1]) and int(pos[0]) >= 0 and int(pos[-1]) < int(graph_build.camera_tables(BIG_CAMS)[4][-1])
    assert np.all(np.abs(starts[ei[0]] - starts[ei[1]]) < gap) and not np.any(BIG_CAMS[ei[0]] == BIG_CAMS[ei[1]])
    assert len(np.unique(ei[0] * BIG_N + ei[1])) == want      # no pair twice: with the count, every candidate once


def test_beyond_the_old_limit_a_gradient_is_refused_before_any_launch():
    leaf = torch.zeros(BIG_N, BIG_F, device="cuda").requires_grad_()
    with pytest.raises(NotImplementedError, match="backward"):
        mtmc_mpn.build_graph(leaf, BIG_CAMS, k=BIG_K)
    with pytest.raises(NotImplementedError):
        mtmc_mpn.build_graph(leaf.detach(), BIG_CAMS)          # the all-pairs list stays at 46 000 nodes
