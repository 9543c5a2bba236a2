"""The yardstick of the cluster-score tests: the five clustering scores of two label vectors from their definitions, in
numpy and Python numbers (integers for every count, `math.fsum` for every sum, `math.lgamma` for the factorials).

  ARI   from the pair confusion tp = sum n_ij^2 - n, fp = sum b^2 - sum n_ij^2, fn = sum a^2 - sum n_ij^2, tn = the rest
        of the n (n - 1) ordered pairs;
        1 if fn == fp == 0, else 2 (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn))
  H     -sum a/n (ln a - ln n), exactly 0 for one cluster;  MI = sum n_ij/n ln(n n_ij / (a b)), clamped at 0
  EMI   over pairs of distinct cluster sizes (a, b) with their multiplicities (`emi_full` is the same sum over all R x C
        cluster pairs, for the tests to hold the two against each other)
  homogeneity = 1 if H_true == 0 else MI / H_true; completeness likewise; V = harmonic mean (0 if both are 0)
  AMI   1 if R == C == 1, else (MI - EMI) / den, den = (H_true + H_pred) / 2 - EMI kept eps away from 0 with its sign

`edge_prf_ref` is compute_P_R_F of the reference's inference loop, written out on Python integers.
"""
import collections
import math
import sys

import numpy as np

NAMES = ("ari", "ami", "homogeneity", "completeness", "v_measure", "entropy_true", "entropy_pred", "mi", "emi")


def contingency(labels_true, labels_pred):
    """(a [R], b [C], cells {(i, j): n_ij}) as Python integers"""
    t = np.asarray(labels_true).reshape(-1)
    p = np.asarray(labels_pred).reshape(-1)
    assert t.shape == p.shape and t.size >= 1
    _, ti = np.unique(t, return_inverse=True)
    _, pi = np.unique(p, return_inverse=True)
    a = [int(v) for v in np.bincount(ti.reshape(-1))]
    b = [int(v) for v in np.bincount(pi.reshape(-1))]
    flat, cnt = np.unique(ti.reshape(-1).astype(np.int64) * len(b) + pi.reshape(-1), return_counts=True)
    cells = {(int(f) // len(b), int(f) % len(b)): int(c) for f, c in zip(flat, cnt)}
    return a, b, cells


def _pair_term(a, b, n):
    """sum over n_ij of n_ij/n ln(n n_ij/(a b)) P(n_ij), P hypergeometric"""
    lo, hi = max(1, a + b - n), min(a, b)
    base = math.lgamma(a + 1) + math.lgamma(b + 1) + math.lgamma(n - a + 1) + math.lgamma(n - b + 1) - math.lgamma(n + 1)
    terms = []
    for nij in range(lo, hi + 1):
        g = base - math.lgamma(nij + 1) - math.lgamma(a - nij + 1) - math.lgamma(b - nij + 1) \
            - math.lgamma(n - a - b + nij + 1)
        terms.append(nij / n * math.log(n * nij / (a * b)) * math.exp(g))
    return math.fsum(terms)


def emi_sizes(a, b, n):
    ca, cb = collections.Counter(a), collections.Counter(b)
    return math.fsum(ca[x] * cb[y] * _pair_term(x, y, n) for x in ca for y in cb)


def emi_full(a, b, n):
    return math.fsum(_pair_term(x, y, n) for x in a for y in b)


def entropy(sizes, n):
    if len(sizes) == 1:
        return 0.0
    return -math.fsum(s / n * (math.log(s) - math.log(n)) for s in sizes)


def cluster_scores_ref(labels_true, labels_pred):
    """-> (scores: dict of the nine floats in NAMES order, counts: [R, C, cells, tp, fp, fn, tn])"""
    a, b, cells = contingency(labels_true, labels_pred)
    n = sum(a)
    sa, sb, sn = sum(x * x for x in a), sum(x * x for x in b), sum(x * x for x in cells.values())
    tp, fp, fn = sn - n, sb - sn, sa - sn
    tn = n * (n - 1) - tp - fp - fn
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    h_true, h_pred = entropy(a, n), entropy(b, n)
    mi = max(0.0, math.fsum(c / n * math.log(n * c / (a[i] * b[j])) for (i, j), c in cells.items()))
    emi = emi_sizes(a, b, n)
    hom = 1.0 if h_true == 0.0 else mi / h_true
    com = 1.0 if h_pred == 0.0 else mi / h_pred
    v = 0.0 if hom + com == 0.0 else 2.0 * hom * com / (hom + com)
    if len(a) == 1 and len(b) == 1:
        ami = 1.0
    else:
        den = (h_true + h_pred) / 2.0 - emi
        eps = sys.float_info.epsilon
        den = min(den, -eps) if den < 0 else max(den, eps)
        ami = (mi - emi) / den
    scores = dict(zip(NAMES, (ari, ami, hom, com, v, h_true, h_pred, mi, emi)))
    return scores, [len(a), len(b), len(cells), tp, fp, fn, tn]


def edge_prf_ref(predictions, labels):
    """-> ([TP, FP, TN, FN], [P, R, F, precision_class0, precision_class1]); zero denominators give 0"""
    p = np.asarray(predictions).reshape(-1).astype(np.int64)
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    tp, fp = int(((y == 1) & (p == 1)).sum()), int(((y == 0) & (p == 1)).sum())
    tn, fn = int(((y == 0) & (p == 0)).sum()), int(((y == 1) & (p == 0)).sum())
    pr = tp / (tp + fp) if tp + fp else 0.0
    rc = tp / (tp + fn) if tp + fn else 0.0
    f = 2 * (pr * rc) / (pr + rc) if pr + rc else 0.0
    c0 = tn / (tn + fp) * 100.0 if tn else 0.0
    c1 = tp / (tp + fn) * 100.0 if tp else 0.0
    return [tp, fp, tn, fn], [pr, rc, f, c0, c1]
