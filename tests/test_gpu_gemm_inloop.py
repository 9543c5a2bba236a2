"""The in-loop encoder GEMMs (csrc/gemm_bn.hip) with an INPUT BatchNorm, in each operand format and tile configuration.

tests/test_gpu_gemm.py and test_gpu_gemm_knobs.py reach the three kernels through mtmc_linear_raw, which gives them no input
BatchNorm; here the node-encoder phases of an eval forward run through the engine's phase interface (the only route that
does), under the knobs that select the bf16x6 / fp32 kernels and keep the few-row, pre-split and staged kernels out of the
way.  `h0` is compared with an fp64 CPU recomputation of the encoder (Linear, batch-statistics BatchNorm, ReLU per layer).
The knobs are read once per process, so every case is a fresh child process.

What the plan tells: in-loop 64x64 / 128x128 tiles and the split-K factor of every layer -- asserted in the child.  It does not
name the operand format or BK; those follow from the knobs and from K (launch_gemm_bn): BK = 64 where the block's share of K
is a multiple of 64, else 32; bf16x6 exists for 128x128 tiles only, so MTMC_GEMM_NO_F16 puts 64x64-tile layers on the fp32
kernel (the n70 "bf16x6" case runs what its "fp32" case runs, and layers 2-3 of n8100 do too).

Bounds.  fp16 (default build): the forward-parity bound of tests/test_gpu_parity.py, 1e-4 * max(1, |h0|max).  bf16x6 and
fp32 have no project bound: 2 x the error of the commit BEFORE the shared staging functions, measured on these very cases
(profiles/gemm_inloop_refactor_ab.txt); the factor covers the fp64 statistics' atomics, which reorder from run to run.
The measured values stand in PARENT_ERR below.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FP16_BOUND = 1e-4                      # tests/test_gpu_parity.py: |h - ref| <= 1e-4 * max(1, |ref|max)
# max |h0 - fp64| / max(1, |h0|max) of the parent commit on these cases (profiles/gemm_inloop_refactor_ab.txt)
# (three runs each, the same to every digit; the fp16 cases gave n70 9.94e-7, n8100 1.15e-6, bk32 8.59e-7 there)
PARENT_ERR = {("n70", "bf16x6"): 7.447e-7, ("n70", "fp32"): 7.447e-7, ("n8100", "bf16x6"): 1.397e-6, ("bk32", "fp32"): 7.074e-7}
FORMAT_ENV = {"fp16": {}, "bf16x6": {"MTMC_GEMM_NO_F16": "1"}, "fp32": {"MTMC_GEMM_FP32": "1"}}
# shape -> (nodes, hidden widths of the encoder or None for 2048 -> 1024 -> 512 -> 128 -> 32, knobs,
#           the plan's kernel per layer ("64" / "128" tiles), its split-K factor per layer)
SHAPES = {
    # 64x64 tiles: layers 0-2 split four ways + combine (layer 1: K = 1024, two refills of the fp16 kernel's affine chunk),
    # layer 3 (K = 128) un-split, with the edge encoder's job as its passenger (fp16) or behind it (the one-call forward)
    "n70": (70, None, {"MTMC_GEMM_NO_FEW": "1"}, ["64"] * 4, [4, 4, 4, 1]),
    # 128x128 tiles with an input BatchNorm: layer 1 (N = 512: 4 column tiles) needs 64 row tiles, i.e. > 8064 rows; ragged last tile
    "n8100": (8100, None, {"MTMC_GEMM_NO_PRESPLIT": "1", "MTMC_GEMM_NO_STAGED": "1"}, ["128", "128", "64", "64"], [1, 1, 4, 1]),
    # BK = 32 with an input BatchNorm: layer 1 has K = 96
    "bk32": (70, [96, 128], {"MTMC_GEMM_NO_FEW": "1"}, ["64"] * 3, [4, 1, 1]),
}
CASES = [("n70", "fp16"), ("n70", "fp32"), ("n70", "bf16x6"), ("n8100", "fp16"), ("n8100", "bf16x6"), ("bk32", "fp16"),
         ("bk32", "fp32")]

CHILD = r"""
import ctypes as C, json, sys, types
import torch
sys.path.insert(0, sys.argv[1])
import mtmc_mpn
from mtmc_mpn import _lib, engine
n, widths, want_kernel, want_split, one_call = json.loads(sys.argv[2])
params = mtmc_mpn.default_params(num_enc_steps=1, num_class_steps=1)
if widths:
    params["encoder_feats_dict"]["nodes"]["resnet101"]["node_fc_dims"] = widths
torch.manual_seed(n)
model = mtmc_mpn.MOTMPNet(params, None, "resnet101").eval()
spec = model.spec
g = torch.Generator().manual_seed(7)
with torch.no_grad():                                   # BatchNorm affines that do something
    for l in spec.enc_node:
        bn = model.encoder.node_mlp.fc_layers[l.bn_slot]
        bn.weight.copy_(0.5 + torch.rand(l.out_dim, generator=g))
        bn.bias.copy_(0.2 * torch.randn(l.out_dim, generator=g))
x = torch.randn(n, spec.enc_node[0].in_dim, generator=g)
idx = torch.arange(n)
edge_index = torch.stack([idx.repeat_interleave(2), torch.stack([(idx + 1) % n, (idx + 2) % n], 1).reshape(-1)])
edge_attr = torch.rand(2 * n, spec.enc_edge[0].in_dim, generator=g)

# fp64 recomputation of the encoder: Linear, BatchNorm on the batch's statistics, ReLU
a = x.double()
for l in spec.enc_node:
    fc = model.encoder.node_mlp.fc_layers
    y = a @ fc[l.lin_slot].weight.double().t() + fc[l.lin_slot].bias.double()
    mean, var = y.mean(0), y.var(0, unbiased=False)
    a = torch.relu((y - mean) / torch.sqrt(var + 1e-5) * fc[l.bn_slot].weight.double() + fc[l.bn_slot].bias.double())
ref = a

model = model.cuda()
eng = engine.ForwardEngine(model)
plan = eng.plan(n, 2 * n)
names = {_lib.GEMM_INLOOP_64: "64", _lib.GEMM_INLOOP_128: "128"}
got_kernel = [names.get(k, str(k)) for k in plan.enc_kernel]
for l, (wk, ws) in enumerate(zip(want_kernel, want_split)):
    assert got_kernel[l] == wk and plan.enc_split_k[l] == ws, ("plan of layer", l, got_kernel, plan.enc_split_k)
with torch.no_grad():
    prep = eng.prepare(x.cuda(), edge_index.cuda(), edge_attr.cuda())
    pairs = eng.phase_list()
    stop = pairs.index((_lib.PH_NODE_H0, 0)) + 1
    for ph, arg in pairs[:stop]:
        eng.run_phase(prep, ph, arg)
    torch.cuda.synchronize()
    h0 = eng.region(prep, "h0").cpu().double()
    err = float((h0 - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    out = {"err": err, "kernel": got_kernel, "split_k": list(plan.enc_split_k), "passenger": plan.enc2_passenger}
    if one_call:      # the rest of the phases, then the one-call forward, where the edge encoder's job rides with / behind the last layer
        for ph, arg in pairs[stop:]:
            eng.run_phase(prep, ph, arg)
        torch.cuda.synchronize()
        by_phase = eng.outputs(prep)[0][0].clone()
        _lib.check(eng.lib.mtmc_mpn_forward(C.byref(prep.model), C.byref(prep.call)))
        torch.cuda.synchronize()
        out["one_call"] = float((eng.outputs(prep)[0][0] - by_phase).abs().max())
print("RESULT " + json.dumps(out))
"""


def run_case(shape, fmt):
    n, widths, knobs, kernels, splits = SHAPES[shape]
    env = dict(os.environ, **knobs, **FORMAT_ENV[fmt])
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps([n, widths, kernels, splits, shape == "n70"])], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.parametrize("shape, fmt", CASES)
def test_encoder_h0_against_fp64(shape, fmt):
    res = run_case(shape, fmt)
    bound = FP16_BOUND if fmt == "fp16" else 2 * PARENT_ERR[(shape, fmt)]
    print(f"{shape} {fmt}: max |h0 - fp64| / max(1, |h0|max) = {res['err']:.3e} (bound {bound:.3e}); plan {res['kernel']} "
          f"split-K {res['split_k']} passenger {res['passenger']} one-call vs phases {res.get('one_call')}")
    assert res["err"] <= bound, res
    if shape == "n70":
        # the edge encoder's second pass rides in (fp16) or behind (bf16x6, fp32) the un-split last layer of the one-call
        # forward; both routes of the same forward agree to the bound test_gpu_parity.py holds them to
        assert res["passenger"] == 1 and res["one_call"] <= 2e-6, res
