"""Inputs of the edge-loss and focal-loss GPU tests (tests/test_gpu_edge_loss.py, tests/test_gpu_focal_loss.py): the logits with
planted ties and +-80 rows, the weight modes of both classifier forms, and the model settings of the tests that run the loss
on a training forward.  The yardsticks are edge_loss_ref.py and focal_ref.py."""
import copy
import types

import torch

import mtmc_mpn
from golden_util import ARCH

DEV = "cuda:0"


def make_inputs(e, s, c, seed, labels="mixed"):
    """randn * 3 logits with exact ties (x0 == x1; x == 0) and rows at +-80 planted, nothing else within 1e-5 of a tie;
    about 2 % positives with -100 rows interleaved, or one class only."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(s, e, c, generator=g) * 3
    if c == 2:
        d = x[..., 1] - x[..., 0]
        x[..., 1] = torch.where((d.abs() < 1e-5), x[..., 0] + 1.0, x[..., 1])
        x[:, 5::29] = torch.tensor([80.0, -80.0])
        x[:, 7::31] = torch.tensor([-80.0, 80.0])
        x[:, ::17, 1] = x[:, ::17, 0]
    else:
        x[x.abs() < 1e-5] = 1.0
        x[:, 5::29] = 80.0
        x[:, 7::31] = -80.0
        x[:, ::17] = 0.0
    if labels == "mixed":
        y = (torch.rand(e, generator=g) < 0.02).long()
        y[[i for i in (0, 5, 7) if i < e]] = 1              # positives on a tie, on a +80 and on a -80 row as well
        y[3::41] = -100
    else:
        y = torch.full((e,), int(labels), dtype=torch.long)
    return x, y


def weight_modes(c):
    if c == 2:
        return [dict(), dict(weight=torch.tensor([0.7, 4.2], device=DEV)), dict(weight="balanced")]
    return [dict(), dict(pos_weight=torch.tensor([4.2], device=DEV)), dict(pos_weight="balanced")]


def to_gpu(d):
    return types.SimpleNamespace(x=d.x.cuda(), edge_index=d.edge_index.cuda(), edge_attr=d.edge_attr.cuda())


def nodrop(params):
    p = copy.deepcopy(params)
    p["encoder_feats_dict"]["nodes"][ARCH]["dropout_p"] = 0.0
    p["edge_model_feats_dict"]["dropout_p"] = 0.0
    p["node_model_feats_dict"]["dropout_p"] = 0.0
    return p


def one_logit_params():
    p = nodrop(mtmc_mpn.default_params(num_enc_steps=3, num_class_steps=3))
    p["classifier_feats_dict"]["edge_out_dim"] = 1
    return p
