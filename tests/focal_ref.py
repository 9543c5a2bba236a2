"""fp64 torch restatement of what mtmc_mpn.edge_loss(gamma > 0) and mtmc_mpn.focal_loss return -- TEST INFRASTRUCTURE: the
yardstick of tests/test_focal_loss.py and tests/test_gpu_focal_loss.py.  The row loss is written the textbook way, not by
the margin trick of the kernels: (1 - softmax(x)[y])^gamma * F.cross_entropy(reduction='none') for two logits and
(1 - exp(-bce))^gamma * bce for one (the reference's FocalLoss_binary, utils.py:715-720, per row).  Weights, the
denominator D, class means, probabilities, counts and the FPR term are those of edge_loss_ref.

1 - p_t is taken without the subtraction, as the probability of the other class: the other softmax output, resp.
sigmoid(-x) for target 1 and sigmoid(x) for target 0 (Lin et al.'s p_t).  The test inputs plant rows at +-80, where 1 - p_t
is 3e-70 resp. 2e-35: subtracted from 1 in fp64 (and as 1 - exp(-bce), where torch's bce is itself exactly 0) it is 0, and
autograd of 0^gamma is inf * 0 = NaN for gamma < 1, so the subtracting form has no gradient to compare against there.
tests/test_focal_loss.py holds this form to the reference's subtracting one at 1e-12 per row."""
import torch
import torch.nn.functional as F

from edge_loss_ref import Ref


def class_weights(c, n0, n1, weight, pos_weight):
    given = weight if c == 2 else pos_weight
    if given is None:
        return torch.ones(2, dtype=torch.float64)
    if isinstance(given, str):
        assert given == "balanced"
        return torch.tensor([1.0, n0 / n1 if n0 and n1 else 1.0], dtype=torch.float64)
    if c == 2:
        return torch.as_tensor(given).detach().cpu().double().view(2)
    return torch.cat([torch.ones(1, dtype=torch.float64), torch.as_tensor(given).detach().cpu().double().view(1)])


def focal_rows(x, y, gamma):
    """f [n] of x [n, C] (fp64, may require grad) against y [n] in {0, 1}."""
    if x.shape[1] == 2:
        ce = F.cross_entropy(x, y, reduction="none")
        return torch.softmax(x, 1).gather(1, (1 - y).view(-1, 1)).view(-1) ** gamma * ce
    bce = F.binary_cross_entropy_with_logits(x[:, 0], y.to(x.dtype), reduction="none")
    return torch.where(y == 1, torch.sigmoid(-x[:, 0]), torch.sigmoid(x[:, 0])) ** gamma * bce


def focal_ref(steps, labels, gamma, weight=None, pos_weight=None, fpr_alpha=0.0):
    """As edge_loss_ref: steps [E, C] fp64 tensors (C = 1 or 2), labels [E] int64, rows other than 0 / 1 left out; `loss`
    keeps its autograd graph."""
    keep = ((labels == 0) | (labels == 1)).nonzero().view(-1)
    y = labels[keep]
    n0, n1 = int((y == 0).sum()), int((y == 1).sum())
    c = steps[0].shape[1]
    w = class_weights(c, n0, n1, weight, pos_weight)
    d = float(w[0]) * n0 + float(w[1]) * n1 if c == 2 else float(n0 + n1)
    m0, m1 = y == 0, y == 1
    loss = 0.0
    class_loss, class_prob, confusion, fpr = [], [], [], []
    for x in steps:
        x = x[keep]
        f = focal_rows(x, y, gamma)
        loss = loss + (w[y] * f).sum() / d
        xd = x.detach()
        if c == 2:
            prob = torch.softmax(xd, 1).gather(1, y.view(-1, 1)).view(-1)
            pred = torch.argmax(xd, 1) == 1                              # first maximum on ties
        else:
            prob = torch.where(m1, torch.sigmoid(xd[:, 0]), torch.sigmoid(-xd[:, 0]))
            pred = xd[:, 0] >= 0
        tp, fp = int((pred & m1).sum()), int((pred & m0).sum())
        tn, fn = int((~pred & m0).sum()), int((~pred & m1).sum())
        per = f.detach()
        class_loss.append([float(per[m0].mean()) if n0 else 0.0, float(per[m1].mean()) if n1 else 0.0])
        class_prob.append([float(prob[m0].mean()) if n0 else 0.5, float(prob[m1].mean()) if n1 else 0.5])
        confusion.append([tp, fp, tn, fn])
        fpr.append(fp / (fp + tn) if n0 else 0.0)
    loss = loss + fpr_alpha * sum(fpr)
    return Ref(loss, torch.tensor(class_loss, dtype=torch.float64), torch.tensor(class_prob, dtype=torch.float64),
               torch.tensor(confusion, dtype=torch.int64), torch.tensor(fpr, dtype=torch.float64), w)


def focal_weighted_rows(x, labels, gamma, weight=None, pos_weight=None):
    """[E] = w[y] * f, 0 on rows labelled neither 0 nor 1: focal_loss(reduction="none"); differentiable in x."""
    keep = ((labels == 0) | (labels == 1)).nonzero().view(-1)
    y = labels[keep]
    w = class_weights(x.shape[1], int((y == 0).sum()), int((y == 1).sum()), weight, pos_weight)
    out = torch.zeros(x.shape[0], dtype=x.dtype)
    return out.index_add(0, keep, w[y] * focal_rows(x[keep], y, gamma))
