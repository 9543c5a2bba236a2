"""BASELINE.json configs 4 and 5 at FULL size, checked -- not only timed.

* config 4 (100k nodes / 10M edges, L=3): the HIP forward against the CPU oracle evaluated in fp64 on the host
  (the reference's ATen ops in the reference's order; ~1 minute of CPU).
* config 5 (1M nodes / 100M edges, L=3) does not fit a CPU evaluation ([E,68] fp64 alone is 54 GB and minutes of
  work), so the same oracle code is evaluated by torch ON THE GPU in fp64 (rocBLAS / ATen kernels, nothing of this
  repo's) and compared on every edge; on top of that, size-independent properties of the result are checked
  directly from the definition: the last round's node state is the row-sum of non-negative messages (h >= 0,
  rows without out-edges exactly 0) and the logits are an affine image of a ReLU output (bounded by the classifier).

Tolerance: 1e-4 on the logits (north_star), labels equal outside the 2e-4 margin guard, h within 1e-4 relative.
"""
import copy
import gc
import types

import pytest
import torch

import mtmc_mpn
from golden_util import ARCH
from mtmc_mpn import graphs

pytestmark = pytest.mark.gpu
LOGIT_TOL, MARGIN_GUARD = 1e-4, 2e-4


def _model(seed=0):
    torch.manual_seed(seed)
    params = mtmc_mpn.default_params(num_enc_steps=3, num_class_steps=1)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m, sd, params


def _compare(got, want64, h, h64, tag):
    err = (got.double() - want64).abs().max().item()
    assert err <= LOGIT_TOL, f"{tag}: max |dlogit| {err:.3e}"
    margin = want64[:, 1] - want64[:, 0]
    guard = margin.abs() > MARGIN_GUARD
    flips = int((((got[:, 1] - got[:, 0]) > 0) != (margin > 0))[guard].sum())
    assert flips == 0, f"{tag}: {flips} label flips outside the margin guard"
    scale = max(1.0, h64.abs().max().item())
    herr = (h.double() - h64).abs().max().item()
    assert herr <= 1e-4 * scale, f"{tag}: h differs by {herr:.3e} (scale {scale:.3e})"
    return err


def test_config4_full_size_against_cpu_fp64_oracle():
    from oracle import mpn_oracle
    m, sd, params = _model()
    d = graphs.stress_graph(100_000, 5_000_000, seed=4)          # CPU generator: the bench's config-4 recipe
    assert d.edge_index.shape == (2, 10_000_000)
    with torch.no_grad():
        g = types.SimpleNamespace(x=d.x.cuda(), edge_index=d.edge_index.cuda(), edge_attr=d.edge_attr.cuda())
        out, h = m.cuda()(g)
        got, h = out["classified_edges"][0].cpu(), h.cpu()
        del g, out
        ora64, oh64 = mpn_oracle.forward(sd, copy.deepcopy(params), ARCH, d.x, d.edge_index, d.edge_attr,
                                         dtype=torch.float64)
    err = _compare(got, ora64["classified_edges"][0], h, oh64, "config 4")
    print(f"config 4 full size: max |logit - fp64 oracle| = {err:.3e}")


def test_config5_full_size_against_fp64_oracle_on_device_and_properties():
    from oracle import mpn_oracle
    free, total = torch.cuda.mem_get_info()
    if total < 200 * 2 ** 30:
        pytest.skip("needs the 288 GB of an MI355X")
    m, sd, params = _model()
    N, E = 1_000_000, 100_000_000
    d = graphs.stress_graph(N, E // 2, seed=5, device="cuda")
    assert d.edge_index.shape == (2, E)
    with torch.no_grad():
        out, h = m.cuda()(d)
        torch.cuda.synchronize()
        got = out["classified_edges"][0]
        # --- properties straight from the definition (mpn.py:97-99, :291-292) ---
        assert got.shape == (E, 2) and h.shape == (N, 32)
        assert torch.isfinite(got).all() and torch.isfinite(h).all()
        assert (h >= 0).all()                                       # sums of ReLU outputs
        deg = torch.bincount(d.edge_index[0], minlength=N)
        assert (h[deg == 0] == 0).all()                             # rows no edge starts from: exactly 0 (no residual)
        assert (h[deg > 0].sum(1) > 0).all()
        # --- the oracle's code, run by torch on the device in fp64 ---
        m.cpu()
        del m
        gc.collect()
        torch.cuda.empty_cache()
        sd_dev = {k: v.cuda() for k, v in sd.items()}
        ora64, oh64 = mpn_oracle.forward(sd_dev, copy.deepcopy(params), ARCH, d.x, d.edge_index, d.edge_attr,
                                         dtype=torch.float64)
        err = _compare(got, ora64["classified_edges"][0], h, oh64, "config 5")
    print(f"config 5 full size: max |logit - fp64 oracle (device)| = {err:.3e}")


def _skewed_graph(N, E, seed):
    """Row-sorted list with ascending columns whose rows are very unequal: two thirds of the nodes have no out-edge at all
    (whole 64-row waves of the blocked traversal are empty), a handful have thousands (sub-runs far longer than a wave's trip),
    columns cluster in the first column block for a tenth of the rows (seven of eight sub-runs empty), duplicates allowed."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    src = torch.randperm(N, device="cuda", generator=g)[:N // 3]
    w = torch.rand(src.numel(), device="cuda", generator=g)
    w[:8] = 400.0                                            # eight rows with ~1/6 of all edges each ... well, thousands
    row = src[torch.multinomial(w, E, replacement=True, generator=g)]
    col = torch.randint(0, N, (E,), device="cuda", generator=g)
    narrow = (row % 10) == 0
    col[narrow] = col[narrow] % (N // 8)
    key, _ = torch.sort(row * N + col)
    ei = torch.stack([key // N, key % N])
    x = torch.randn(N, 2048, device="cuda", generator=g)
    return types.SimpleNamespace(x=x, edge_index=ei, edge_attr=torch.rand(E, 2, device="cuda", generator=g))


@pytest.mark.parametrize("over,unsort_cols", [
    (dict(num_enc_steps=2, num_class_steps=2), False),                                   # first-round + later-round kernels
    (dict(num_enc_steps=2, num_class_steps=1, reattach_initial_edges=True, reattach_initial_nodes=True), False),
    (dict(num_enc_steps=2, num_class_steps=1), True),       # columns shuffled inside the rows: the in-order kernel must take over
    (dict(num_enc_steps=2, num_class_steps=1), "skewed"),   # empty rows, huge rows, empty sub-runs
    # the blocked path's correctness hangs on prep_kernel's flags[2] (columns ascending inside a row) and on the
    # sub-run boundaries snapped to multiples of four edges
    (dict(num_enc_steps=1, num_class_steps=1), "descending"),      # every row's columns in DESCENDING order: flag -> in-order kernel
    (dict(num_enc_steps=2, num_class_steps=1), "boundary_dups"),   # many equal columns exactly on the column-block boundaries
])
def test_column_blocked_pass_a_regime(over, unsort_cols):
    """Pass A by column blocks (csrc/edge_pass_a.hip pass_a_blocked_kernel: graphs whose Pc table, 16 B per node, outgrows
    an XCD's L2): 230 000 nodes / 9.2 M edges is the smallest size that takes it (8 blocks of 28 750 nodes, sub-runs of 5
    edges -- ragged: many are empty) -- against the oracle's code run by torch on the device in fp64, every edge."""
    from mtmc_mpn import _lib, engine
    from oracle import mpn_oracle
    torch.manual_seed(3)
    params = mtmc_mpn.default_params(**over)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    N, E = 230_000, 9_200_000
    d = _skewed_graph(N, E, 12) if unsort_cols == "skewed" else graphs.stress_graph(N, E // 2, seed=11, device="cuda")
    if unsort_cols == "descending":
        key = d.edge_index[0] * N + (N - 1 - d.edge_index[1])
        perm = torch.argsort(key, stable=True)
        d.edge_index, d.edge_attr = d.edge_index[:, perm].contiguous(), d.edge_attr[perm].contiguous()
        same_row = d.edge_index[0][1:] == d.edge_index[0][:-1]
        assert (d.edge_index[1][1:][same_row] <= d.edge_index[1][:-1][same_row]).all()
    if unsort_cols == "boundary_dups":
        wb = N // 8                                           # width of a column block (plan_col_blocks: 8 blocks)
        side = torch.randint(0, 2, (E,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        col = (d.edge_index[1] // wb).clamp(max=7) * wb + side * (wb - 1)        # first or last column of its block: runs of equal columns
        key, perm = torch.sort(d.edge_index[0] * N + col, stable=True)
        d.edge_index = torch.stack([key // N, key % N]).contiguous()
        d.edge_attr = d.edge_attr[perm].contiguous()
    plan = engine.ForwardEngine(m).plan(N, E)
    assert plan.pass_a_col_blocks == 8 and plan.pass_c == _lib.PASS_C_MFMA_SORTED
    if unsort_cols is True:                                  # same rows, columns of each row in random order
        perm = torch.argsort(d.edge_index[0] * 4 + torch.randint(0, 4, (E,), device="cuda"), stable=True)
        d.edge_index, d.edge_attr = d.edge_index[:, perm].contiguous(), d.edge_attr[perm].contiguous()
        assert (d.edge_index[0][1:] >= d.edge_index[0][:-1]).all()
    with torch.no_grad():
        out, h = m.cuda()(d)
        torch.cuda.synchronize()
        sd_dev = {k: v.cuda() for k, v in sd.items()}
        ora64, oh64 = mpn_oracle.forward(sd_dev, copy.deepcopy(params), ARCH, d.x, d.edge_index, d.edge_attr,
                                         dtype=torch.float64)
        for i, got in enumerate(out["classified_edges"]):
            _compare(got, ora64["classified_edges"][i], h, oh64, f"column-blocked pass A, output {i}")
