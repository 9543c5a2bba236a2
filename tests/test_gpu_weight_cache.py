"""The weight-plane cache verifies itself (csrc/split_body.h, engine.weight_plane_cache): every way of changing a weight that
fooled round 4's host-side (data_ptr, _version) key -- ADVICE round 4 -- must give the NEW weights' logits, on the few-row
path (every layer reads cached planes) and on the many-row path (layers 0 and 1 do)."""
import copy
import gc
import types

import pytest
import torch

import mtmc_mpn
from mtmc_mpn import _lib, engine, graphs, torch_ops

pytestmark = pytest.mark.gpu
ARCH = "resnet101"
TOL = 1e-4


def _oracle(model, params, d):
    from oracle import mpn_oracle
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        out, h = mpn_oracle.forward(sd, copy.deepcopy(params), ARCH, d.x.cpu(), d.edge_index.cpu(), d.edge_attr.cpu(), dtype=torch.float64)
    return out["classified_edges"][-1], h


def _fwd(model, d):
    with torch.no_grad():
        out, h = model(d)
    torch.cuda.synchronize()
    return out["classified_edges"][-1].cpu(), h.cpu()


def _graph(cams=(40, 30, 35), seed=3):
    d = graphs.camera_graph(cams, seed=seed)
    return types.SimpleNamespace(x=d.x.cuda(), edge_index=d.edge_index.cuda(), edge_attr=d.edge_attr.cuda())


def _model(seed, L=2):
    params = mtmc_mpn.default_params(num_enc_steps=L, num_class_steps=1)
    torch.manual_seed(seed)
    return mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH).eval().cuda(), params


def _assert_matches(model, params, d, tag):
    got, h = _fwd(model, d)
    want, h64 = _oracle(model, params, d)
    err = (got.double() - want).abs().max().item()
    assert err <= TOL, f"{tag}: max |dlogit| {err:.3e}"
    assert (h.double() - h64).abs().max().item() <= 1e-4 * max(1.0, h64.abs().max().item()), tag


def test_few_row_path_is_taken_and_uses_the_cache():
    m, params = _model(0)
    d = _graph()
    plan = engine.ForwardEngine(m).plan(d.x.shape[0], d.edge_index.shape[1])
    assert plan.enc_kernel[0] == _lib.GEMM_FEW_L0 and plan.enc_kernel[1] == _lib.GEMM_FEW_WAVE
    _assert_matches(m, params, d, "first forward (every chunk derived)")
    _assert_matches(m, params, d, "second forward (every chunk verified, none derived)")


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_write_through_param_data_is_seen(layer):
    """`param.data` writes do not bump Parameter._version: round 4's key called the planes valid and multiplied by the OLD
    weights without any error."""
    m, params = _model(1)
    d = _graph()
    _assert_matches(m, params, d, "before")
    w = engine.ordered_params(m)[4 * layer]
    v0 = w._version
    w.data[5, 7] += 0.5                                         # ONE element of one chunk
    w.data[w.shape[0] - 1].mul_(-1.0)                           # ... and a whole row of the last chunk
    assert w._version == v0
    _assert_matches(m, params, d, f"after a param.data write to encoder layer {layer}")


def test_new_module_at_recycled_addresses():
    """`del model; model = load(ckpt2)`: the caching allocator hands back the same addresses at the same _version; the engine
    (and its cache buffer) is process-global per configuration."""
    d = _graph()
    m1, params = _model(2)
    _assert_matches(m1, params, d, "model 1")
    ptrs1 = [p.data_ptr() for p in engine.ordered_params(m1)[:4]]
    del m1
    gc.collect()
    m2, params = _model(3)
    ptrs2 = [p.data_ptr() for p in engine.ordered_params(m2)[:4]]
    _assert_matches(m2, params, d, "model 2" + (" at recycled addresses" if ptrs1 == ptrs2 else ""))


def test_failed_call_then_good_call():
    """A call that fails before anything is launched must not leave a cache that a later call trusts."""
    m, params = _model(4)
    d = _graph()
    bad = types.SimpleNamespace(x=d.x[:1].clone(), edge_index=d.edge_index[:, :0], edge_attr=d.edge_attr[:0])
    with pytest.raises((ValueError, RuntimeError)):
        m(bad)                                                  # BatchNorm over one row: MTMC_E_ROWS
    _assert_matches(m, params, d, "good call after a failed one")
    w = engine.ordered_params(m)[0]
    w.data.mul_(0.5)
    with pytest.raises((ValueError, RuntimeError)):
        m(bad)
    _assert_matches(m, params, d, "good call after a failed one and a weight change")


def test_optimizer_step_and_load_state_dict():
    m, params = _model(5)
    d = _graph()
    _assert_matches(m, params, d, "before")
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.01 * torch.randn_like(p))
    _assert_matches(m, params, d, "after in-place updates of all 34 parameters")
    other, _ = _model(6)
    m.load_state_dict(other.state_dict())
    _assert_matches(m, params, d, "after load_state_dict")


def test_without_the_cache_the_split_k_kernels_still_run():
    m, params = _model(7)
    d = _graph()
    m.cache_weight_planes = False
    _assert_matches(m, params, d, "cache_weight_planes = False")
    got_off, _ = _fwd(m, d)
    m.cache_weight_planes = True
    got_on, _ = _fwd(m, d)
    assert (got_on - got_off).abs().max().item() <= 2e-5       # two kernel families, one answer


def test_captured_graph_follows_param_data_writes():
    """Under graph capture round 4 never used the cache; now the verification itself is part of the captured forward."""
    m, params = _model(8)
    d = _graph()
    replay = m.capture(d)
    out, _ = replay()
    torch.cuda.synchronize()
    want, _ = _oracle(m, params, d)
    assert (out["classified_edges"][-1].cpu().double() - want).abs().max().item() <= TOL
    engine.ordered_params(m)[4].data[3].add_(0.25)
    out, _ = replay()
    torch.cuda.synchronize()
    want2, _ = _oracle(m, params, d)
    assert (want2 - want).abs().max().item() > 1e-3             # (the change matters)
    assert (out["classified_edges"][-1].cpu().double() - want2).abs().max().item() <= TOL


def test_many_row_graph_sees_weight_changes():
    """8200 node rows: layer 0 on pre-split weights and layer 1 on the role-split kernel read the cached planes."""
    m, params = _model(9, L=1)
    g = graphs.stress_graph(8200, 30_000, seed=5)
    d = types.SimpleNamespace(x=g.x.cuda(), edge_index=g.edge_index.cuda(), edge_attr=g.edge_attr.cuda())
    plan = engine.ForwardEngine(m).plan(8200, d.edge_index.shape[1])
    assert plan.enc_kernel[:2] == [_lib.GEMM_PRESPLIT_256, _lib.GEMM_STAGED_128]
    _assert_matches(m, params, d, "before")
    for layer in (0, 1):
        engine.ordered_params(m)[4 * layer].data[11].mul_(1.5)
    _assert_matches(m, params, d, "after param.data writes to layers 0 and 1")


# -- the cache's bytes, bit for bit (tests/wcache_util.py: layout, plane decode, fingerprint mirror) ----------------------
import numpy as np  # noqa: E402

import wcache_util as wu  # noqa: E402

FEW_LAYERS, MANY_LAYERS = (0, 1, 2, 3), (0, 1)          # the layers whose planes each path reads from the cache


def _many_row_graph():
    g = graphs.stress_graph(8200, 30_000, seed=5)
    return types.SimpleNamespace(x=g.x.cuda(), edge_index=g.edge_index.cuda(), edge_attr=g.edge_attr.cuda())


def _case(path, seed):
    """(model, params, graph, layers read from the cache) of the few-row or the many-row path."""
    if path == "few":
        m, params = _model(seed)
        return m, params, _graph(), FEW_LAYERS
    m, params = _model(seed, L=1)
    return m, params, _many_row_graph(), MANY_LAYERS


def _weight(m, layer):
    return engine.ordered_params(m)[4 * layer]


def _assert_fingerprints_mirror(m, buf, layers, tag, others_empty=False):
    """Every stored fingerprint of `layers` is the mirror's for the current weights (others_empty: the other layers hold
    none, zeros)."""
    for l, lay in enumerate(wu.model_layout(m)):
        _, _, fp = wu.layer_views(buf, lay)
        got = fp.cpu().numpy()
        if l in layers:
            want = wu.fingerprints(_weight(m, l).detach().cpu().numpy())
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (f"{tag}: layer {l}: {bad.size} of {got.size} stored fingerprints differ from the mirror; "
                                   f"chunk {bad[0]}: {int(got[bad[0]]) & wu.M64:#018x} != {int(want[bad[0]]) & wu.M64:#018x}")
        elif others_empty:
            assert not got.any(), f"{tag}: layer {l} is not read from the cache on this path but has fingerprints"


def _assert_planes_are_the_weights(m, buf, layers, tag):
    """(h1 + h2) * inv reproduces the fp32 weights to 2^-21 of each row's |.|max (test_gpu_gemm_presplit's bound)."""
    for l, lay in enumerate(wu.model_layout(m)):
        if l not in layers:
            continue
        planes, inv, _ = wu.layer_views(buf, lay)
        W = _weight(m, l).detach().double()
        rec = (planes[0] + planes[1]) * inv.unsqueeze(1)
        amax = W.abs().amax(dim=1, keepdim=True)
        err = (rec - W).abs()
        assert (err <= amax * 2.0 ** -21 + 1e-300).all(), f"{tag}: layer {l}: planes off by {(err / amax).max().item():.3e} rel"


@pytest.mark.parametrize("path", ["few", "many"])
def test_stored_fingerprints_are_the_mirrors(path):
    """Pins tests/wcache_util.py (which tests/test_weight_fingerprint.py checks on the CPU) to what the kernels store:
    prep_kernel's passenger workgroups (few-row) and split_jobs_kernel (the 8200-row graph)."""
    m, _, d, layers = _case(path, 20)
    _fwd(m, d)
    buf = wu.live_cache(m)
    buf.zero_()                                          # nothing of an earlier test's module: every chunk derived now
    _fwd(m, d)
    _assert_fingerprints_mirror(m, buf, layers, path, others_empty=True)
    _assert_planes_are_the_weights(m, buf, layers, path)


def test_training_forward_stores_the_mirrors_fingerprints():
    """engine.prepare hands the cache to training forwards too (split_rows_body with amax_out != nullptr)."""
    m, params = _model(21)
    d = _graph()
    _fwd(m, d)
    buf = wu.live_cache(m)
    buf.zero_()
    m.train()
    out, h = m(d)
    labels = (torch.rand(d.edge_index.shape[1], generator=torch.Generator().manual_seed(3)) < 0.15).long().cuda()
    mtmc_mpn.cross_entropy_steps(out["classified_edges"], labels).backward()
    torch.cuda.synchronize()
    written = [l for l, lay in enumerate(wu.model_layout(m)) if wu.layer_views(buf, lay)[2].any().item()]
    assert 0 in written, f"the training forward stored no fingerprint of layer 0 (layers written: {written})"
    _assert_fingerprints_mirror(m, buf, written, "training forward")
    _assert_planes_are_the_weights(m, buf, written, "training forward")


def _edits(seed, d):
    """The edits the cache has to follow, as (name, function of the module): each changes node-encoder weights in a way a
    linear fingerprint can miss, or the way users do."""
    def advisor_swap(m):                                   # W[r][1] <-> W[r][8] in the first row of a chunk, every layer
        for l in range(4):
            w = _weight(m, l)
            w.data[8, [1, 8]] = w.data[8, [8, 1]].clone()

    def row_swap(m):
        w = _weight(m, 1)
        w.data[[17, 22]] = w.data[[22, 17]].clone()

    def column_swap(m):
        w = _weight(m, 0)
        w.data[[40, 45], 300] = w.data[[45, 40], 300].clone()

    def plus_minus_d(m):                                   # +d / -d on the bit patterns of two words of one round-5 multiplier
        bits = _weight(m, 0).data.view(torch.int32)
        bits[24, 1] += 0x1000
        bits[24, 8] -= 0x1000

    def load_state_dict(m):
        other, _ = _model(seed + 100)
        m.load_state_dict(other.state_dict())

    def training_step(m):
        m.train()
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        out, _ = m(d)
        labels = (torch.rand(d.edge_index.shape[1], generator=torch.Generator().manual_seed(4)) < 0.15).long().cuda()
        mtmc_mpn.cross_entropy_steps(out["classified_edges"], labels).backward()
        opt.step()
        m.eval()

    return [("advisor swap", advisor_swap), ("row swap", row_swap), ("column swap", column_swap),
            ("+d/-d pair", plus_minus_d), ("load_state_dict", load_state_dict), ("training step", training_step)]


@pytest.mark.parametrize("path", ["few", "many"])
def test_incremental_cache_equals_a_fresh_one(path):
    """After every edit, the cache kept from forward to forward is byte for byte the one derived from zero for the same
    weights (a zero-filled chunk never matches: fingerprints are odd), and its planes are the current weights."""
    m, _, d, layers = _case(path, 22)
    _fwd(m, d)
    buf = wu.live_cache(m)
    buf.zero_()
    _fwd(m, d)
    regions = [(lay[r], lay[r] + n) for l, lay in enumerate(wu.model_layout(m)) if l in layers
               for r, n in (("planes", 4 * lay["O"] * lay["K"]), ("inv", 4 * lay["O"]), ("fp", 8 * ((lay["O"] + 7) // 8)))]
    for name, edit in _edits(22, d):
        before = [_weight(m, l).detach().clone() for l in range(4)]
        edit(m)
        assert any(not torch.equal(b, _weight(m, l)) for l, b in enumerate(before)), name
        _fwd(m, d)
        assert wu.live_cache(m) is buf
        kept = buf.clone()
        buf.zero_()
        _fwd(m, d)
        for lo, hi in regions:                             # (all of it on the few-row path; the layers it reads on the other)
            diff = (kept[lo:hi] != buf[lo:hi]).nonzero()
            assert diff.numel() == 0, (f"{path}, after the {name}: {diff.shape[0]} bytes of the kept cache differ from a "
                                       f"fresh one, first at byte {lo + diff[0].item()}")
        _assert_planes_are_the_weights(m, buf, layers, f"{path}, after the {name}")
        _assert_fingerprints_mirror(m, buf, layers, f"{path}, after the {name}")


def _set_up_swap(m, layer=0, row=8):
    """W[row][1] = 2, W[row][8] = -2: swapping the two then changes the layer's output for sure."""
    w = _weight(m, layer)
    w.data[row, 1], w.data[row, 8] = 2.0, -2.0


def _swap(m, layer=0, row=8):
    w = _weight(m, layer)
    w.data[row, [1, 8]] = w.data[row, [8, 1]].clone()


@pytest.mark.parametrize("path", ["few", "many"])
def test_advisor_swap_is_seen_by_the_forward(path):
    m, params, d, layers = _case(path, 23)
    for l in layers[:2]:
        _set_up_swap(m, l)
    _assert_matches(m, params, d, f"{path}: before the swap")
    want, _ = _oracle(m, params, d)
    for l in layers[:2]:
        _swap(m, l)
    want2, _ = _oracle(m, params, d)
    assert (want2 - want).abs().max().item() > 1e-3                # (the swap matters)
    _assert_matches(m, params, d, f"{path}: after swapping W[8][1] and W[8][8]")


def test_captured_graph_sees_the_advisor_swap():
    m, params = _model(24)
    d = _graph()
    _set_up_swap(m)
    replay = m.capture(d)
    out, _ = replay()
    torch.cuda.synchronize()
    want, _ = _oracle(m, params, d)
    assert (out["classified_edges"][-1].cpu().double() - want).abs().max().item() <= TOL
    _swap(m)
    out, _ = replay()
    torch.cuda.synchronize()
    want2, _ = _oracle(m, params, d)
    assert (want2 - want).abs().max().item() > 1e-3
    assert (out["classified_edges"][-1].cpu().double() - want2).abs().max().item() <= TOL


def test_two_modules_of_one_configuration_alternate_on_one_stream():
    """EMA / teacher pattern: module B is module A with the swap; both share their configuration's engine and the stream's
    cache, so every call re-derives the chunk the other one left."""
    a, params = _model(25)
    _set_up_swap(a)
    b = copy.deepcopy(a)
    _swap(b)
    d = _graph()
    want_a, _ = _oracle(a, params, d)
    want_b, _ = _oracle(b, params, d)
    assert (want_b - want_a).abs().max().item() > 1e-3
    for i in range(3):
        _assert_matches(a, params, d, f"module A, call {i}")
        _assert_matches(b, params, d, f"module B, call {i}")


def test_unchanged_chunks_are_not_split_again():
    """Garbage planes under a matching fingerprint are KEPT (the verify-only path writes nothing, and the helper's offsets
    are the ones the kernels read: the logits move); one changed weight of the chunk brings the right planes back."""
    m, params = _model(26)
    d = _graph()
    got0, _ = _fwd(m, d)
    buf = wu.live_cache(m)
    lay = wu.model_layout(m)[0]
    K, O = lay["K"], lay["O"]
    planes = buf[lay["planes"]:lay["planes"] + 4 * O * K].view(torch.float16).view(2, K // 32, O, 32)
    garbage = (torch.rand(2, K // 32, 8, 32, generator=torch.Generator().manual_seed(1)) * 20000 - 10000).half().cuda()
    planes[:, :, 24:32] = garbage                          # all of chunk 3's rows, whatever the swizzle
    fp_before = buf[lay["fp"]:lay["fp"] + 8 * (O // 8)].clone()
    got1, _ = _fwd(m, d)
    assert torch.equal(planes[:, :, 24:32], garbage), "a chunk whose fingerprint matched was split again"
    assert torch.equal(buf[lay["fp"]:lay["fp"] + 8 * (O // 8)], fp_before)
    assert (got1 - got0).abs().max().item() > 1e-3, "garbage planes did not move the logits: the offsets are not the kernels'"
    _weight(m, 0).data[26, 5] += 0.125
    _assert_matches(m, params, d, "after one weight of the chunk changed")
    _assert_planes_are_the_weights(m, buf, (0,), "after one weight of the chunk changed")
    _assert_fingerprints_mirror(m, buf, FEW_LAYERS, "after one weight of the chunk changed")
