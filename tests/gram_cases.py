"""Inputs, references and the error yardstick for `build_graph` in every regime of its Gram product and on near-duplicate
tracklets (tests/test_gram_cases.py on the CPU, tests/test_gpu_graph_build_regimes.py on the GPU).  No GPU in here.

G = X X^T goes through launch_gemm_bn(plain_gemm(...)) without |.|max words, so gemm_plan / launch_gemm_bn
(csrc/gemm_bn.hip, the last two functions) choose, with M = Nout = N and K = F:
    exact fp32 MFMA, 64 x 64 tiles, split-K 4     F % 256 == 0, N <= 960
    the same, split-K 2                           F % 128 == 0, F % 256 != 0, N <= 960
    the same, unsplit, BK = 64                    F <= 128 or F % 128 != 0, with F % 64 == 0; any such F at 961 <= N <= 1920
    the same, unsplit, BK = 32                    F % 64 != 0
    gemm_bn_bf16x6_kernel<2,2,32>, 128 x 128      N >= 1921: ceil(N / 128)^2 >= 256 tiles (gemm_plan: big_tiles)
    linear_generic_kernel (scalar)                F > 6144 (mfma_shape, which both call); refused at N > 2048 (launch_gemm_bn)
The split shows in mtmc_graph_workspace_bytes (slab term split * N^2 * 4 bytes); the last two rules do not: they are
restated above from the lines named and a change there has to be followed here by hand.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-6                                   # F.pairwise_distance's eps, added to the difference
NEAR = 1e-3                                  # gb_near (csrc/graph_backward.hip): d^2 < NEAR (rho_r^2 + rho_c^2)
FLOAT_EDGE_CAP = 200_000                     # floating outputs are compared on every edge up to here, on a sample above

# (N, F, cameras, l2norm, expected split, regime / what the case is for); l2norm=False runs on feats.abs()
FORWARD_CASES = (
    (9, 32, 3, True, 1, "fp32 BK32: smallest F, one tile"),
    (63, 96, 3, True, 1, "fp32 BK32: tile edge 63"),
    (64, 96, 3, True, 1, "fp32 BK32: tile edge 64"),
    (65, 96, 3, True, 1, "fp32 BK32: tile edge 65"),
    (65, 160, 3, True, 1, "fp32 BK32: K > 128 unsplit"),
    (65, 160, 3, False, 1, "fp32 BK32: K > 128 unsplit, no l2norm"),
    (65, 192, 3, True, 1, "fp32 BK64: K > 128 unsplit"),
    (130, 128, 3, True, 1, "fp32 BK64: K <= 128 rule"),
    (130, 384, 3, True, 2, "fp32 split-K 2"),
    (130, 256, 3, True, 4, "fp32 split-K 4, slice 64"),
    (130, 256, 3, False, 4, "fp32 split-K 4, slice 64, no l2norm"),
    (961, 96, 4, True, 1, "fp32 BK32: 256 tiles unsplit, last tile one row"),
    (961, 2048, 4, True, 1, "fp32 BK64: 256 tiles unsplit, last tile one row"),
    (1921, 64, 4, True, 1, "bf16x6 128x128: last tile one row, 3 grid-stride trips"),
    (1921, 2048, 4, True, 1, "bf16x6 128x128: last tile one row, 3 grid-stride trips"),
    (40, 6176, 3, True, 1, "scalar generic path"),
)
FORWARD_NOISE = 0.01

# (N, F, cameras, noise, l2norm, flagged edges in fp64); l2norm=False runs on feats.abs()
BACKWARD_CASES = (
    (31, 32, 3, 0.01, True, 60),
    (33, 96, 3, 0.01, True, 66),
    (64, 160, 4, 0.01, True, 192),
    (65, 256, 4, 0.01, True, 192),
    (65, 256, 4, 0.01, False, 192),
    (72, 2048, 3, 0.01, True, 144),
    (300, 64, 4, 0.02, True, 898),
)


def case_seed(n, f):
    return 1000 * n + f


def case_id(case):
    return "-".join(str(v) for v in case[:-1] if not isinstance(v, str)).replace("True", "l2").replace("False", "raw")


def near_case(n, f, n_cams, noise, seed, equal_pairs=1):
    """Training-order nodes (identity by identity, cameras interleave): (feats [n, f] f32, cams, ids).  Every identity's
    siblings sit in different cameras; the first `equal_pairs` identities have two exactly equal rows."""
    gen = torch.Generator().manual_seed(seed)
    ids = np.arange(n) // n_cams
    cams = np.arange(n) % n_cams
    base = torch.randn(int(ids[-1]) + 1, f, generator=gen)
    feats = base[torch.from_numpy(ids)] + noise * torch.randn(n, f, generator=gen)
    for p in range(equal_pairs):
        feats[n_cams * p + 1] = feats[n_cams * p]
    return feats, cams, ids


def forward_inputs(case):
    n, f, n_cams, l2norm = case[:4]
    feats, cams, ids = near_case(n, f, n_cams, FORWARD_NOISE, case_seed(n, f))
    return (feats if l2norm else feats.abs()), cams, ids


def backward_inputs(case):
    n, f, n_cams, noise, l2norm = case[:5]
    feats, cams, ids = near_case(n, f, n_cams, noise, case_seed(n, f))
    return (feats if l2norm else feats.abs()), cams, ids


def topology(cams):
    """edge_index [2, E] by the oracle's own statements (oracle/graph_oracle.py)."""
    from oracle import graph_oracle
    return graph_oracle.topology(cams)


def reference_attr(feats, cams, l2norm, edges):
    """fp64 reference of the floating outputs for the edges `edges` [2, K] (any subset, any order): the normalised rows x64
    and [ ||x_r - x_c + 1e-6||, 1 - cos(x_r, x_c) ] formed from the F-dimensional rows themselves, never from a Gram matrix.
    Chunked: three [chunk, F] fp64 temporaries of 128 MB at the most."""
    x = feats.double()
    if l2norm:
        x = F.normalize(x, p=2, dim=0)
    row, col = edges[0], edges[1]
    attr = torch.empty(row.numel(), 2, dtype=torch.float64)
    chunk = max(1, (1 << 24) // x.shape[1])
    for s in range(0, row.numel(), chunk):
        a, b = x[row[s:s + chunk]], x[col[s:s + chunk]]
        attr[s:s + chunk, 0] = (a - b + EPS).square().sum(1).sqrt()
        na, nb = a.square().sum(1).sqrt().clamp_min(1e-8), b.square().sum(1).sqrt().clamp_min(1e-8)
        attr[s:s + chunk, 1] = 1 - ((a / na[:, None]) * (b / nb[:, None])).sum(1)
    return x, attr


def rho2(x64):
    return x64.square().sum(1)


def flagged(d, rho2_nodes, edges):
    """gb_near's rule on any precision's d and rho^2."""
    return d.square() < NEAR * (rho2_nodes[edges[0]] + rho2_nodes[edges[1]])


def float_sample(cams, ids, edges, seed=0):
    """Edges whose floating outputs are compared: all of them up to FLOAT_EDGE_CAP, else every same-identity edge, the first and
    last 256 of every camera block and 20 000 seeded random ones (sorted, unique)."""
    e = edges.shape[1]
    if e <= FLOAT_EDGE_CAP:
        return torch.arange(e)
    lab = torch.from_numpy(np.asarray(ids))
    same = torch.nonzero(lab[edges[0]] == lab[edges[1]]).flatten()
    cams = np.asarray(cams)
    parts, off = [same], 0
    for c in np.unique(cams):
        size = int((cams == c).sum()) * int((cams != c).sum())
        parts += [torch.arange(off, off + min(256, size)), torch.arange(off + max(size - 256, 0), off + size)]
        off += size
    assert off == e
    parts.append(torch.randint(0, e, (20_000,), generator=torch.Generator().manual_seed(seed)))
    return torch.unique(torch.cat(parts))


@functools.lru_cache(maxsize=None)
def gram_model(f, noise, l2norm, seed=0):
    """The yardstick of the forward's error: the kernels' formulas on near_case(150, f, 3, noise, seed) with G accumulated in
    fp32 one k at a time, unsplit -- the longest chain any Gram path may have (the scalar path has exactly this one; the
    MFMA paths add blocks of 2 to 4 k and split-K shortens the chain).  Returns (max |d^2 - d_ref^2| / (rho_r^2 + rho_c^2),
    max |cos - cos_ref|) over the cross-camera pairs, against fp64.  The constants grow with K, not with N."""
    feats, cams, _ = near_case(150, f, 3, noise, seed)
    if not l2norm:
        feats = feats.abs()
    x = feats.clone()
    if l2norm:                                 # gb_normalize_kernel: v / max((float)sqrt(colsq), 1e-12), colsq in fp64
        nrm = feats.double().square().sum(0).sqrt().float().clamp_min(1e-12)
        x = feats / nrm
    xd = x.double()
    g = torch.zeros(150, 150, dtype=torch.float32)
    for k in range(f):                         # fused multiply-add: the fp32 x fp32 product is exact in fp64, one rounding
        g = (g.double() + xd[:, k, None] * xd[None, :, k]).float()
    row_sq = xd.square().sum(1).float()        # fp64 sum, rounded to fp32, as the kernel documents
    row_sum = xd.sum(1).float()
    eps = torch.tensor(EPS, dtype=torch.float32)
    nr, nc = row_sq[:, None], row_sq[None, :]
    d2 = nr + nc - 2 * g + 2 * eps * (row_sum[:, None] - row_sum[None, :]) + torch.tensor(float(f)) * eps * eps
    cos = g / (nr.sqrt().clamp_min(1e-8) * nc.sqrt().clamp_min(1e-8))
    assert d2.dtype == torch.float32 and cos.dtype == torch.float32
    x64 = F.normalize(feats.double(), p=2, dim=0) if l2norm else feats.double()
    d2_ref = (x64[:, None, :] - x64[None, :, :] + EPS).square().sum(2)
    r2 = rho2(x64)
    rho = r2.sqrt().clamp_min(1e-8)
    cos_ref = (x64 @ x64.T) / (rho[:, None] * rho[None, :])
    cross = torch.from_numpy(cams[:, None] != cams[None, :])
    c_d2 = ((d2.double() - d2_ref).abs() / (r2[:, None] + r2[None, :]))[cross].max().item()
    c_cos = (cos.double() - cos_ref).abs()[cross].max().item()
    return c_d2, c_cos


def workspace_split(n, f, total):
    """The split-K factor behind a value of mtmc_graph_workspace_bytes(n, f): graph_layout's list (csrc/graph_build.hip)
    restated, every block rounded up to 256 bytes, the slab term being split * n^2 * 4 bytes (absent when unsplit)."""
    up = lambda b: (b + 255) // 256 * 256
    base = up(f * 8) + 2 * up(n * 4) + up(n * n * 4) + up(n * 4)
    for split in (1, 2, 4, 8):
        if base + (up(split * n * n * 4) if split > 1 else 0) == total:
            return split
    raise AssertionError(f"workspace of ({n}, {f}) = {total} bytes matches no split of the layout")


def oracle_grad(feats, cams, l2norm, g_x, g_attr, dtype=torch.float64):
    """CPU autograd of the oracle in `dtype`, contracted with g_x / g_attr (tests/test_gpu_graph_build_backward.py's, with the
    precision as a parameter)."""
    from oracle import graph_oracle
    leaf = feats.detach().to(dtype).clone().requires_grad_()
    x, _, attr, _ = graph_oracle.build(leaf, cams, None, l2norm)
    loss = 0
    if g_x is not None:
        loss = loss + (x * g_x.to(dtype)).sum()
    if g_attr is not None and attr.shape[0]:
        loss = loss + (attr * g_attr.to(dtype)).sum()
    loss.backward()
    return leaf.grad


def seeded_grads(n, f, e, seed=11):
    """g_x, g_attr as tests/test_gpu_graph_build_backward.py's run() draws them."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, f, generator=gen), torch.randn(e, 2, generator=gen)


def grad_bar(want):
    return 1e-6 + 2e-4 * want.abs().max().item()


def edge_trips(e, block=256, max_blocks=4096):
    """grid-stride trips of gb_edges_kernel over e edges"""
    return math.ceil(e / (block * max_blocks))
