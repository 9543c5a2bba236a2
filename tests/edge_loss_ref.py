"""fp64 torch restatement of what mtmc_mpn.edge_loss returns -- TEST INFRASTRUCTURE: the yardstick of tests/test_edge_loss.py
and tests/test_gpu_edge_loss.py.  Every loss is torch's own F.cross_entropy(weight=...) / F.binary_cross_entropy_with_logits(
pos_weight=...); class means, probabilities and counts are taken with boolean masks (the reference's way, train.py:36-245)."""
import collections

import torch
import torch.nn.functional as F

Ref = collections.namedtuple("Ref", ["loss", "class_loss", "class_prob", "confusion", "fpr", "class_weight"])


def edge_loss_ref(steps, labels, weight=None, pos_weight=None, fpr_alpha=0.0):
    """steps: [E, C] fp64 tensors (C = 1 or 2, they may require grad); labels [E] int64, rows other than 0 / 1 are left out.
    weight (C = 2) / pos_weight (C = 1): None, "balanced", or numbers."""
    keep = ((labels == 0) | (labels == 1)).nonzero().view(-1)
    y = labels[keep]
    n0, n1 = int((y == 0).sum()), int((y == 1).sum())
    c = steps[0].shape[1]
    given = weight if c == 2 else pos_weight
    if given is None:
        w = torch.ones(2, dtype=torch.float64)
    elif isinstance(given, str):
        assert given == "balanced"
        w = torch.tensor([1.0, n0 / n1 if n0 and n1 else 1.0], dtype=torch.float64)     # reference train.py:127-130
    elif c == 2:
        w = torch.as_tensor(given).detach().cpu().double().view(2)
    else:
        w = torch.cat([torch.ones(1, dtype=torch.float64), torch.as_tensor(given).detach().cpu().double().view(1)])
    w = w.to(steps[0].device)
    loss = 0.0
    class_loss, class_prob, confusion, fpr = [], [], [], []
    for x in steps:
        x = x[keep]
        if c == 2:
            loss = loss + F.cross_entropy(x, y, weight=w)
            per = F.cross_entropy(x.detach(), y, reduction="none")
            prob = torch.softmax(x.detach(), 1).gather(1, y.view(-1, 1)).view(-1)
            pred = torch.argmax(x.detach(), 1) == 1                        # first maximum on ties
        else:
            t = y.to(x.dtype)
            loss = loss + F.binary_cross_entropy_with_logits(x[:, 0], t, pos_weight=w[1:])
            per = F.binary_cross_entropy_with_logits(x.detach()[:, 0], t, reduction="none")
            p1 = torch.sigmoid(x.detach()[:, 0])
            prob = torch.where(y == 1, p1, torch.sigmoid(-x.detach()[:, 0]))
            pred = x.detach()[:, 0] >= 0
        m0, m1 = y == 0, y == 1
        tp, fp = int((pred & m1).sum()), int((pred & m0).sum())
        tn, fn = int((~pred & m0).sum()), int((~pred & m1).sum())
        class_loss.append([float(per[m0].mean()) if n0 else 0.0, float(per[m1].mean()) if n1 else 0.0])
        class_prob.append([float(prob[m0].mean()) if n0 else 0.5, float(prob[m1].mean()) if n1 else 0.5])
        confusion.append([tp, fp, tn, fn])
        fpr.append(fp / (fp + tn) if n0 else 0.0)
    loss = loss + fpr_alpha * sum(fpr)
    return Ref(loss, torch.tensor(class_loss, dtype=torch.float64), torch.tensor(class_prob, dtype=torch.float64),
               torch.tensor(confusion, dtype=torch.int64), torch.tensor(fpr, dtype=torch.float64), w.cpu())
