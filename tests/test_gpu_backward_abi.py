"""The three C entry points of the backward, called directly on ONE tape (include/mtmc_mpn.h):
  (a) mtmc_mpn_backward_flat  -- what the torch ops use: the library carves one flat buffer
  (b) mtmc_mpn_backward       -- one contiguous d_logits block, a `grads` struct of separately allocated tensors
  (c) mtmc_mpn_backward_steps -- grads_flat = NULL, a per-step pointer array with a NULL entry, its own tensors
(b) and (c) clear every receiving tensor themselves (one memset each), transpose x and the W_l in a launch of their own
and, for (b), turn the d_logits block into per-step pointers; no other test runs that code.

Reference: fp64 CPU autograd of the oracle with the loss sum_s <d_logits_s, logits_s> + <d_h, h>, at the bounds of
tests/test_gpu_training.py::check_against_cpu (grad_bounds.py).  Those bounds carry an absolute floor sized for the
gradients of a mean loss over the edges, so the incoming gradients here are scaled as such a loss's are: d_logits ~ 1/E,
d_h ~ 1/(32 N)."""
import copy
import ctypes as C

import pytest
import torch

import mtmc_mpn
from golden_util import ARCH
from grad_bounds import assert_input_grads_close, assert_param_grads_close
from mtmc_mpn import _lib, engine, graphs, torch_ops
from test_gpu_training import cpu_autograd, nodrop

pytestmark = pytest.mark.gpu

GARBAGE = 1e30          # what every receiving tensor of (b) and (c) holds before the call: the clearing is under test


def _grads_struct(model, tensors, slots):
    """A `grads` struct (mtmc_mpn_model layout) whose pointers name `tensors` (layer_slots order)."""
    g = _lib.Model.from_buffer_copy(model)
    it = iter(tensors)
    for slot, idx, layer in slots:
        dst = getattr(g, slot) if idx is None else getattr(g, slot)[idx]
        dst.weight, dst.bias = next(it).data_ptr(), next(it).data_ptr()
        if layer.bn_slot is not None:
            dst.gamma, dst.beta = next(it).data_ptr(), next(it).data_ptr()
    return g


@pytest.mark.parametrize("over", [
    dict(num_enc_steps=2, num_class_steps=2),
    dict(num_enc_steps=3, num_class_steps=2, node_agg_fn="max", reattach_initial_nodes=True, reattach_initial_edges=True),
    dict(num_enc_steps=0, num_class_steps=1),
])
def test_the_three_backward_entry_points_on_one_tape(over):
    d = graphs.camera_graph((14, 11, 9), seed=9)
    n, e = d.x.shape[0], d.edge_index.shape[1]
    assert (n, e) == (34, 758)
    params = nodrop(mtmc_mpn.default_params(**over))
    torch.manual_seed(0)
    m = mtmc_mpn.MOTMPNet(copy.deepcopy(params), None, ARCH)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.cuda().train()
    spec = m.spec
    slots = engine.layer_slots(spec)
    n_out, n_cls = engine.n_classified_steps(spec), spec.cls_edge[0].out_dim
    gen = torch.Generator().manual_seed(77)
    d_logits = torch.randn(n_out, e, n_cls, generator=gen) / e
    d_h = torch.randn(n, 32, generator=gen) / (32 * n)
    null_step = 0                                            # (c) hands the library NULL for this step

    def reference(skip):
        def loss_fn(out, h):
            return sum((d_logits[s].double() * o).sum() for s, o in enumerate(out["classified_edges"]) if s != skip) \
                + (d_h.double() * h).sum()
        _, grads, dx, dea, out = cpu_autograd(sd, copy.deepcopy(params), d, None, True, None, True, loss_fn=loss_fn)
        assert len(out["classified_edges"]) == n_out
        return grads, dx, dea
    ref_all, ref_dx, ref_dea = reference(None)
    ref_c, _, _ = reference(null_step)

    # ---- one training-mode forward; its workspace is the tape of the three backwards -----------------------------
    eng = engine.ForwardEngine(m)
    lib = eng.lib
    x, ea = d.x.cuda(), d.edge_attr.cuda()
    ei = d.edge_index.t().contiguous().cuda().t()
    prep = eng.prepare(x, ei, ea, training=True, tape=True)
    _lib.check(lib.mtmc_mpn_forward(C.byref(prep.model), C.byref(prep.call)))
    dl, dh = d_logits.cuda(), d_h.cuda()
    steps_all = (C.c_void_p * n_out)(*[dl[s].data_ptr() for s in range(n_out)])
    steps_c = (C.c_void_p * n_out)(*[None if s == null_step else dl[s].data_ptr() for s in range(n_out)])

    name_of = {id(p): k for k, p in m.named_parameters()}
    names = [name_of[id(p)] for p in engine.ordered_params(m)]
    shapes = [shp for _, _, shp in torch_ops.grad_layout(spec)[0]]
    assert len(names) == len(shapes) == 34
    unused = [spec.num_enc_steps == 0 and slot in ("upd_edge", "upd_node")
              for slot, _, layer in slots for _ in range(4 if layer.bn_slot is not None else 2)]

    def check(tensors, ref):
        named = []
        for k, t, dead in zip(names, tensors, unused):
            assert torch.isfinite(t).all().item(), k
            assert ref[k] is None or not dead, k
            if ref[k] is None:       # no path from the loss: the buffer comes back cleared (L == 0: the update MLPs' buffers)
                assert t.abs().max().item() == 0.0, k
            named.append((k, None if ref[k] is None else t))
        assert_param_grads_close(named, ref, e)

    def garbage_tensors():
        return [torch.full(shp, GARBAGE, device="cuda") for shp in shapes]

    # ---- (a) the flat form -------------------------------------------------------------------------------------------
    offsets, total = torch_ops.grad_layout(spec)
    flat = torch.full((total,), GARBAGE, device="cuda")
    _lib.check(lib.mtmc_mpn_backward_flat(C.byref(prep.model), C.byref(prep.call), steps_all, dh.data_ptr(), flat.data_ptr(),
                                          flat.numel(), None, None))
    check([flat[o:o + numel].view(shp) for o, numel, shp in offsets], ref_all)

    # ---- (b) one d_logits block, a struct of separately allocated tensors, input gradients --------------------------
    tb = garbage_tensors()
    gb = _grads_struct(prep.model, tb, slots)
    d_x = torch.full((n, spec.enc_node[0].in_dim), GARBAGE, device="cuda")
    d_ea = torch.full((e, spec.enc_edge[0].in_dim), GARBAGE, device="cuda")
    _lib.check(lib.mtmc_mpn_backward(C.byref(prep.model), C.byref(prep.call), dl.data_ptr(), dh.data_ptr(), C.byref(gb),
                                     d_x.data_ptr(), d_ea.data_ptr()))
    check(tb, ref_all)
    assert_input_grads_close(d_x, d_ea, ref_dx, ref_dea)

    # ---- (c) per-step pointers with a NULL entry, no flat buffer ------------------------------------------------------
    tc = garbage_tensors()
    gc = _grads_struct(prep.model, tc, slots)
    _lib.check(lib.mtmc_mpn_backward_steps(C.byref(prep.model), C.byref(prep.call), steps_c, dh.data_ptr(), C.byref(gc), None, 0,
                                           None, None))
    check(tc, ref_c)

    # ---- refusals: the return code only ------------------------------------------------------------------------------
    bad = _lib.Model.from_buffer_copy(gb)
    bad.upd_edge.gamma = None
    assert lib.mtmc_mpn_backward(C.byref(prep.model), C.byref(prep.call), dl.data_ptr(), dh.data_ptr(), C.byref(bad),
                                 None, None) == _lib.E_ARG
    bad = _lib.Model.from_buffer_copy(gb)
    bad.struct_bytes = C.sizeof(_lib.Model) - 8
    assert lib.mtmc_mpn_backward(C.byref(prep.model), C.byref(prep.call), dl.data_ptr(), dh.data_ptr(), C.byref(bad),
                                 None, None) == _lib.E_ARG
    torch.cuda.synchronize()
