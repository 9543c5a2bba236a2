"""GPU tests of `build_graph(start_frames=, max_gap=)`: the cross-camera list behind a temporal gate, alone or before the
k-nearest rule (`mtmc_build_graph_gated`).

As for the k list (tests/test_gpu_graph_knn.py, whose helpers these tests borrow), the selection is checked EXACTLY against
the rule's CPU restatement (tests/gate_ref.py, composed with tests/knn_ref.py when `k` is given) applied to the bits the
dense call wrote for the same input (l2norm=False), and with l2norm=True as a set outside a margin band around each row's
k-th key.  Inputs and the lengths of their gated lists: tests/gate_cases.py."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gate_cases
import gate_ref
import knn_ref
import mtmc_mpn
from golden_util import ARCH
from mtmc_mpn import _lib, graph_build
from test_gpu_graph_knn import COS_EPS, bits, feats_for, labels_for, structure

pytestmark = pytest.mark.gpu


def candidates_per_row(ei, pg, n):
    return np.bincount(ei[0, pg].numpy(), minlength=n)


def exact(feats, cams, labels, starts, G, k, pg=None):
    """Dense call and gated call on the same input, l2norm=False: edge_pos is the rule applied to the dense call's own bits,
    and every kept edge carries the dense call's bits.  A second gated call gives the same bits.  pg: the gate's positions in
    the dense list where a caller has them already (gate_cases.dense_gate)."""
    dev = feats.cuda()
    n = len(cams)
    dense = mtmc_mpn.build_graph(dev, cams, labels, l2norm=False)
    g = mtmc_mpn.build_graph(dev, cams, labels, l2norm=False, k=k, start_frames=starts, max_gap=G)
    d_ei = dense.edge_index.cpu()
    e_dense = d_ei.shape[1]
    if pg is None:
        pg = gate_ref.select(starts, d_ei, G)
    e_g = pg.numel()
    assert graph_build.gated_edge_count(cams, starts, G) == e_g
    want = pg if k is None else pg[knn_ref.select(dense.edge_attr[:, 1].cpu()[pg], d_ei[:, pg], cams, k)]
    got = g.edge_pos.cpu()
    assert got.shape == want.shape and torch.equal(got, want), f"G={G}, k={k}: {got.numel()} kept, {want.numel()} expected"

    structure(g, cams, k if k is not None else n, e_dense)              # (2 N N bounds nothing: the gate-only bound is below)
    e = got.numel()
    assert e <= e_g and (k is None or e <= 2 * k * n)
    if k is None:
        assert e == e_g                                                  # ... and the buffers were allocated at exactly E_g
        assert g.edge_attr.untyped_storage().nbytes() == 8 * e and g.edge_index.untyped_storage().nbytes() == 16 * e
        assert g.edge_pos.untyped_storage().nbytes() == 8 * e
        assert labels is None or g.edge_labels.untyped_storage().nbytes() == 4 * e

    assert torch.equal(g.edge_index.cpu(), d_ei[:, want])
    assert torch.equal(bits(g.edge_attr), bits(dense.edge_attr)[want])
    assert torch.equal(bits(g.x), bits(dense.x))
    if labels is not None:
        assert torch.equal(bits(g.edge_labels), bits(dense.edge_labels)[want]) and torch.equal(g.y, dense.y)
    else:
        assert g.edge_labels is None and g.y is None
    again = mtmc_mpn.build_graph(dev, cams, labels, l2norm=False, k=k, start_frames=starts, max_gap=G)
    for name in ("x", "edge_attr", "edge_index", "edge_pos"):
        a, b = getattr(g, name), getattr(again, name)
        assert a.shape == b.shape and (torch.equal(bits(a), bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)), name
    return g, dense


def case(name, feats, labels, k):
    cams, starts, gap, e_g = gate_cases.COUNTS[name]
    ei, pg = gate_cases.dense_gate(name)
    assert pg.numel() == e_g
    g, dense = exact(feats, cams, labels, starts, gap, k, pg)
    assert torch.equal(dense.edge_index.cpu(), ei)
    return g


@pytest.mark.parametrize("k, kept", [(None, 20), (1, 12), (2, 16)])
def test_exact_nine_nodes(k, kept):
    g = case("nine", feats_for(9, 64, 7), labels_for(9), k)
    assert g.edge_pos.numel() == kept
    ei, pg = gate_cases.dense_gate("nine")
    per_row = candidates_per_row(ei, pg, 9)
    assert per_row[0] == 1 and per_row[7] == per_row[8] == 0            # node 0: fewer candidates than k = 2
    src = set(g.edge_index[0].tolist())
    assert not {7, 8} & src


def test_exact_nine_nodes_whole_span():
    g = case("nine, whole span", feats_for(9, 64, 7), labels_for(9), None)
    assert torch.equal(g.edge_pos.cpu(), torch.arange(52))


@pytest.mark.parametrize("k", [None, 2])
def test_nine_nodes_nothing_kept(k):
    g = case("nine, nothing kept", feats_for(9, 64, 7), labels_for(9), k)
    assert g.edge_index.shape == (2, 0) and g.edge_attr.shape == (0, 2) and g.edge_pos.shape == (0,)
    assert g.edge_labels.shape == (0,) and g.x.shape == (9, 64)


@pytest.mark.parametrize("k, kept", [(None, 274), (3, 224)])
def test_exact_one_node_camera_and_out_degrees_around_a_wave(k, kept):
    g = case("wave", feats_for(76, 64, 11), None, k)                     # out-degrees 71, 75, 6
    assert g.edge_pos.numel() == kept
    per_row = candidates_per_row(*gate_cases.dense_gate("wave"), 76)
    assert (per_row == 0).sum() == 20 and ((per_row > 0) & (per_row < 3)).sum() == 21


@pytest.mark.parametrize("k, kept", [(None, 878), (4, 308)])
def test_exact_interleaved_cameras(k, kept):
    cams = gate_cases.COUNTS["interleaved"][0]
    assert np.any(np.diff(cams) < 0)                                     # in_list position order is not node order
    g = case("interleaved", feats_for(62, 256, 12), labels_for(62), k)
    assert g.edge_pos.numel() == kept


@pytest.mark.parametrize("k, kept", [(None, 474368), (7, 9812), (300, 378022)])
def test_exact_rows_longer_than_one_sweep_fp32_gram(k, kept):
    g = case("sweeps", feats_for(1100, 64, 13), None, k)                 # 961 <= N <= 1920: exact fp32
    assert g.edge_pos.numel() == kept
    per_row = candidates_per_row(*gate_cases.dense_gate("sweeps"), 1100)
    assert per_row.max() == 676 and (per_row < 300).sum() == 159


def test_exact_tight_gate_most_rows_empty():
    g = case("sweeps, tight gate", feats_for(1100, 64, 13), None, None)
    assert g.edge_pos.numel() == 770
    assert (candidates_per_row(*gate_cases.dense_gate("sweeps, tight gate"), 1100) == 0).sum() == 568


@pytest.mark.parametrize("G, kept", [((1 << 63) - 1, 6), (6, 4), (5, 0)])
def test_exact_at_the_ends_of_the_accepted_frames(G, kept):
    """Starts at -2^62 and 2^62 lie 2^63 apart, more than any int64 gap: the difference must not wrap on the device."""
    top = graph_build.FRAME_LIMIT
    g, _ = exact(feats_for(4, 64, 3), np.array([0, 1, 0, 1]), None, np.array([-top, top, top - 5, -top + 5]), G, None)
    assert g.edge_pos.numel() == kept
    assert (0, 1) not in {(int(a), int(b)) for a, b in g.edge_index.cpu().T}


@pytest.mark.parametrize("f, kept", [(2048, 4374), (64, 4314)])
def test_exact_s02_split_gate_then_k(f, kept):
    """S02's camera split, max_gap = 300, k = 8: 38 606 gated.  Of them 4 374 are kept with feats_for(450, 2048, 2), the
    reference's feature width, and 4 314 with feats_for(450, 64, 2) -- both figures from the rule's CPU restatement on
    oracle.graph_oracle.build's attributes (fp32 and fp64 agree on them)."""
    g = case("s02", feats_for(450, f, 2), None, 8)
    assert g.edge_pos.numel() == kept


# ---- l2norm=True: the device normalises, so the keys carry its rounding ----

@pytest.mark.parametrize("k", [None, 4])
def test_l2norm_against_the_rule_outside_the_margin_band(k):
    cams, starts, gap, e_g = gate_cases.COUNTS["interleaved"]
    ei, pg = gate_cases.dense_gate("interleaved")
    n = cams.size
    feats = torch.randn(n, 256, generator=torch.Generator().manual_seed(12)).cuda()
    dense = mtmc_mpn.build_graph(feats, cams)
    g = mtmc_mpn.build_graph(feats, cams, k=k, start_frames=starts, max_gap=gap)
    structure(g, cams, k if k is not None else n, ei.shape[1])
    assert torch.equal(dense.edge_index.cpu(), ei)
    pos = g.edge_pos.cpu()
    if k is None:                                             # the gate reads no float: exact
        assert torch.equal(pos, pg) and torch.equal(g.edge_index.cpu(), ei[:, pg])
        at, both = torch.arange(e_g), pg
    else:
        sub_ei, key = ei[:, pg], dense.edge_attr[:, 1].cpu()[pg]            # the candidates: the list the rows rank
        d = key.double().numpy()
        row = sub_ei[0].numpy()
        rank = knn_ref.ranks(key, sub_ei)
        in_top = rank < k
        t_k = np.full(n, -np.inf)                             # the k-th and (k+1)-th key of every row that has them
        t_k1 = np.full(n, np.inf)
        t_k[row[rank == k - 1]] = d[rank == k - 1]
        t_k1[row[rank == k]] = d[rank == k]
        ambiguous = np.where(in_top, d > t_k1[row] - 2 * COS_EPS, d < t_k[row] + 2 * COS_EPS)
        excluded = ambiguous | ambiguous[knn_ref.reverse_positions(sub_ei, n)]
        want = np.zeros(e_g, dtype=bool)
        want[knn_ref.select(key, sub_ei, cams, k).numpy()] = True
        assert int(want.sum()) == 308
        assert np.all(np.isin(pos.numpy(), pg.numpy()))       # only candidates are kept
        got = np.isin(pg.numpy(), pos.numpy())
        n_excl = int((excluded & want).sum())
        print(f"rule keeps {int(want.sum())}, library keeps {int(got.sum())}, {n_excl} of the rule's in the margin band, "
              f"{int((got != want).sum())} differ in all")
        assert n_excl <= 0.01 * want.sum()
        assert np.array_equal(got[~excluded], want[~excluded])
        both = pg[torch.from_numpy(np.nonzero(got & want)[0])]
        at = torch.from_numpy(np.searchsorted(pos.numpy(), both.numpy()))
        assert torch.equal(g.edge_index.cpu()[:, at], ei[:, both])
    d_attr = dense.edge_attr.cpu()
    err = (g.edge_attr.cpu()[at] - d_attr[both]).abs().max(0).values
    assert err[0].item() <= 2e-5 * max(1.0, d_attr[:, 0].abs().max().item()), f"distance err {err[0]:.2e}"
    assert err[1].item() <= 5e-6, f"cosine err {err[1]:.2e}"


def test_gated_k_list_feeds_the_mpn_and_postprocess():
    from oracle import graph_oracle, mpn_oracle
    cams, starts, gap, e_g = gate_cases.COUNTS["interleaved"]
    feats = torch.randn(cams.size, 2048, generator=torch.Generator().manual_seed(8))
    params = mtmc_mpn.default_params(num_enc_steps=2, num_class_steps=1)
    torch.manual_seed(0)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, ei, attr, _ = graph_oracle.build(feats, cams)
    g = mtmc_mpn.build_graph(feats.cuda(), cams, k=4, start_frames=starts, max_gap=gap)
    structure(g, cams, 4, ei.shape[1])
    pos = g.edge_pos.cpu()
    assert 0 < pos.numel() < e_g and torch.equal(g.edge_index.cpu(), ei[:, pos])
    assert np.all(np.isin(pos.numpy(), gate_cases.dense_gate("interleaved")[1].numpy()))
    with torch.no_grad():
        want, _ = mpn_oracle.forward(sd, copy.deepcopy(params), ARCH, x, ei[:, pos], attr[pos])
        got, _ = m.cuda()(g)
    logits = got["classified_edges"][-1]
    assert (logits.cpu() - want["classified_edges"][-1]).abs().max().item() <= 1e-4
    pp = mtmc_mpn.postprocess(logits, g.edge_index, cams.size, 3)
    assert pp.ID_pred.shape == (cams.size,) and pp.ID_pred.dtype == torch.int64


@pytest.mark.parametrize("k", [None, 4])
@pytest.mark.parametrize("l2norm", [True, False])
def test_backward_through_the_kept_edges(l2norm, k):
    """A: bit for bit the dense build_graph's backward fed the same gradients scattered to their dense positions (zero
    elsewhere).  B: fp64 CPU autograd of the reference's statements on the kept edges, at the project's gradient bar
    (tests/test_gpu_graph_build_backward.py::meets_bar: |d| <= 1e-6 + 2e-4 |grad|max)."""
    cams, starts, gap, _ = gate_cases.COUNTS["interleaved"]
    feats = torch.randn(62, 256, generator=torch.Generator().manual_seed(16))
    leaf = feats.cuda().requires_grad_()
    g = mtmc_mpn.build_graph(leaf, cams, None, l2norm, k=k, start_frames=starts, max_gap=gap)
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
    print(f"gated list, k={k}, l2norm={l2norm}: |dgrad| {err:.3e}, |grad|max {scale:.3e}")
    assert torch.isfinite(leaf.grad).all() and err <= 1e-6 + 2e-4 * scale


def test_backward_with_nothing_kept_is_the_gradient_of_x_alone():
    cams, starts, gap, _ = gate_cases.COUNTS["nine, nothing kept"]
    leaf = feats_for(9, 64, 7).cuda().requires_grad_()
    g = mtmc_mpn.build_graph(leaf, cams, None, False, start_frames=starts, max_gap=gap)
    g_x = torch.randn(9, 64, generator=torch.Generator().manual_seed(1)).cuda()
    torch.autograd.backward([g.x, g.edge_attr], [g_x, torch.zeros(0, 2).cuda()])
    assert torch.equal(leaf.grad, g_x)


@pytest.mark.parametrize("k", [0, 3])
def test_capacity_one_short_is_reported_and_nothing_is_written_past_it(k):
    """The C entry point with edge_capacity = E - 1: n_kept_out reports E > capacity, the first E - 1 edges are those of a
    full-sized call, and the word after each output buffer's capacity keeps its guard value."""
    cams, starts, gap, _ = gate_cases.COUNTS["interleaved"]
    feats = feats_for(62, 64, 15).cuda()
    labels = torch.from_numpy(labels_for(62)).cuda()
    full = mtmc_mpn.build_graph(feats, cams, labels.cpu().numpy(), l2norm=False, k=k or None, start_frames=starts, max_gap=gap)
    e = full.edge_pos.numel()
    cap = e - 1
    tables = [torch.from_numpy(a).cuda() for a in graph_build.camera_tables(cams)[:5]]
    e_dense = int(tables[4][-1])
    t_start = torch.from_numpy(starts).cuda()
    lib = _lib.load()
    index = torch.full((cap + 1, 2), -7, dtype=torch.int64, device="cuda")
    attr = torch.full((cap + 1, 2), -7.0, dtype=torch.float32, device="cuda")
    elab = torch.full((cap + 1,), -7.0, dtype=torch.float32, device="cuda")
    pos = torch.full((cap + 1,), -7, dtype=torch.int64, device="cuda")
    n_kept = torch.zeros(1, dtype=torch.int64, device="cuda")
    x = torch.empty_like(feats)
    ws = torch.empty(lib.mtmc_graph_knn_workspace_bytes(62, 64) + 256, dtype=torch.uint8, device="cuda")
    rc = lib.mtmc_build_graph_gated(feats.data_ptr(), feats.stride(0), 62, 64, 0, *[t.data_ptr() for t in tables], 3, e_dense,
                                    labels.data_ptr(), x.data_ptr(), index.data_ptr(), attr.data_ptr(), elab.data_ptr(),
                                    t_start.data_ptr(), gap, k, cap, pos.data_ptr(), n_kept.data_ptr(), ws.data_ptr(),
                                    ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert n_kept.item() == e > cap                                      # the capacity error, in the status word
    assert index[cap].tolist() == [-7, -7] and attr[cap].tolist() == [-7.0, -7.0]
    assert elab[cap].item() == -7.0 and pos[cap].item() == -7
    assert torch.equal(pos[:cap], full.edge_pos[:cap]) and torch.equal(index[:cap].t(), full.edge_index[:, :cap])
    assert torch.equal(bits(attr[:cap]), bits(full.edge_attr[:cap])) and torch.equal(elab[:cap], full.edge_labels[:cap])


def test_refusals():
    feats = feats_for(9, 64, 7)
    cams, starts = gate_cases.NINE_CAMS, gate_cases.NINE_STARTS
    dev = feats.cuda()
    with pytest.raises(RuntimeError, match="go together"):
        mtmc_mpn.build_graph(dev, cams, max_gap=100)
    with pytest.raises(RuntimeError, match="go together"):
        mtmc_mpn.build_graph(dev, cams, start_frames=starts)
    frames_2_63 = [int(v) for v in starts[:8]] + [(1 << 63) - 1]
    for bad in (starts[:8], starts.astype(np.float32), torch.from_numpy(starts).float(), starts > 100, frames_2_63,
                torch.from_numpy(starts).cuda()):
        with pytest.raises(RuntimeError, match="start"):
            mtmc_mpn.build_graph(dev, cams, start_frames=bad, max_gap=100)
    for bad in (0, -1, 2.5, "3", True):
        with pytest.raises(RuntimeError, match="max_gap"):
            mtmc_mpn.build_graph(dev, cams, start_frames=starts, max_gap=bad)
        with pytest.raises(RuntimeError, match="max_gap"):
            mtmc_mpn.build_graph(dev, cams, k=2, start_frames=starts, max_gap=bad)
    with pytest.raises(RuntimeError, match="k must be"):
        mtmc_mpn.build_graph(dev, cams, k=0, start_frames=starts, max_gap=100)
    with pytest.raises(RuntimeError, match="GPU"):
        mtmc_mpn.build_graph(feats, cams, start_frames=starts, max_gap=100)             # CPU tensor
    g = mtmc_mpn.build_graph(dev, np.zeros(9, dtype=int), start_frames=starts, max_gap=100)   # one camera: no edges
    assert g.edge_index.shape == (2, 0) and g.edge_attr.shape == (0, 2) and g.edge_pos.shape == (0,)
    # accepted forms of the same frames: a list, an int32 array, an integer CPU tensor, a numpy gap
    want = mtmc_mpn.build_graph(dev, cams, start_frames=starts, max_gap=100).edge_pos
    for frames in ([int(v) for v in starts], starts.astype(np.int32), torch.from_numpy(starts)):
        assert torch.equal(mtmc_mpn.build_graph(dev, cams, start_frames=frames, max_gap=np.int64(100)).edge_pos, want)
