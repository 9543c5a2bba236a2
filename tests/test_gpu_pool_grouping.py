"""GPU tests of `pool_tracklets(grouping=)` and of the capturable `index=` form: a `Grouping` made beforehand pools with the
bits of the `index=` call (forward and both gradients, weighted or not), and `index=` with check=False can be captured and
replayed on new contents of `index`."""
import numpy as np
import pytest
import torch

import pool_ref

pytestmark = pytest.mark.gpu

D, N, F = 700, 23, 68


def _case(seed=0):
    rng = np.random.default_rng(seed)
    index = rng.integers(0, N, D)
    index[rng.random(D) < 0.05] = N + 3                  # detections of no tracklet
    index[index == 5] = 6                                # an empty tracklet
    embeds = pool_ref.gaussian_embeds(D, F, seed + 1)
    grad = pool_ref.gaussian_embeds(N, F, seed + 2)
    weights = rng.random(D).astype(np.float32)
    return (torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).cuda(), torch.from_numpy(np.array(embeds)).cuda(),
            torch.from_numpy(np.array(grad)).cuda(), torch.from_numpy(weights).cuda())


def _run(embeds, grad, weights, **how):
    from mtmc_mpn import pool_tracklets
    e = embeds.clone().requires_grad_()
    w = None if weights is None else weights.clone().requires_grad_()
    out = pool_tracklets(e, weights=w, check=False, **how)
    out.backward(grad)
    return out.detach(), e.grad, None if w is None else w.grad


@pytest.mark.parametrize("weighted", (False, True))
def test_a_grouping_pools_with_the_bits_of_the_index_call(weighted):
    import mtmc_mpn
    index, embeds, grad, weights = _case()
    weights = weights if weighted else None
    g = mtmc_mpn.group_by_index(index, N)
    want = _run(embeds, grad, weights, index=index, num_tracklets=N)
    for _ in range(2):                                   # group once, pool many times
        got = _run(embeds, grad, weights, grouping=g)
        for a, b in zip(got, want):
            assert (a is None and b is None) or torch.equal(a, b)
    assert bool((want[0][5] == 0).all()) and want[0].shape == (N, F)


def test_grouping_is_checked():
    import mtmc_mpn
    from mtmc_mpn import pool_tracklets
    index, embeds, _, _ = _case()
    g = mtmc_mpn.group_by_index(index, N)
    with pytest.raises(RuntimeError, match="outside"):   # check=True reads the status words, as with index=
        pool_tracklets(embeds, grouping=g)
    with pytest.raises(ValueError):
        pool_tracklets(embeds, grouping=g, index=index, num_tracklets=N)
    with pytest.raises(RuntimeError, match="Grouping"):
        pool_tracklets(embeds[:-1], grouping=g)
    with pytest.raises(RuntimeError, match="Grouping"):
        pool_tracklets(embeds, grouping=(g.perm, g.offsets))


@pytest.mark.parametrize("weighted", (False, True))
def test_the_index_form_can_be_captured(weighted):
    from mtmc_mpn import pool_tracklets
    index, embeds, _, weights = _case()
    other = _case(seed=9)[0]
    weights = weights if weighted else None
    want = [pool_tracklets(embeds, index=i, num_tracklets=N, weights=weights, check=False) for i in (index, other)]
    assert not torch.equal(want[0], want[1])
    static = index.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pool_tracklets(embeds, index=static, num_tracklets=N, weights=weights, check=False)
    for i, w in zip((other, index), reversed(want)):
        static.copy_(i)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, w)
