"""mtmc_postprocess_workspace_bytes (host-only): the workspace keeps its size.

The values are those of the buffer list as first written (offsets rounded to 256 bytes); callers size and cache their
workspaces by this query, and the kernels index the same list, so a changed total means a changed layout."""
import pytest

from mtmc_mpn import _lib


@pytest.mark.parametrize("n_nodes, n_edges, max_active, want", [
    (3, 4, 0, 4_864),
    (1, 0, 0, 4_864),
    (478, 171_000, 0, 8_580_608),
    (478, 171_000, 4_096, 235_008),
    (2_048, 1, 0, 127_488),
    (2_049, 100_000, 0, 5_126_144),
    (100_000, 10_000_000, 200_000, 16_040_448),
])
def test_workspace_bytes(n_nodes, n_edges, max_active, want):
    assert _lib.load().mtmc_postprocess_workspace_bytes(n_nodes, n_edges, max_active) == want


@pytest.mark.parametrize("n_nodes, n_edges", [(0, 5), (5, -1), (2 ** 31, 5)])
def test_unsupported_sizes_return_zero(n_nodes, n_edges):
    assert _lib.load().mtmc_postprocess_workspace_bytes(n_nodes, n_edges, 0) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """MTMC_E_ARG / MTMC_E_WORKSPACE of mtmc_postprocess with host values only (no pointer is read, nothing is launched); each
    refusal names the entry point in mtmc_mpn_last_error()."""
    from abi_refusal import refused
    lib = _lib.load()
    need = lib.mtmc_postprocess_workspace_bytes(10, 20, 0)

    def pp(logits=0x10000, row=0x20000, col=0x30000, stride=1, n=10, e=20, cams=3, prob1=0x40000, pred=0x50000, ids=0x60000,
           info=0x70000, ws=0x100000, nbytes=need):
        return lib.mtmc_postprocess(logits, row, col, stride, n, e, cams, 7, 0, prob1, pred, ids, info, ws, nbytes, None)
    for bad in (dict(n=0), dict(e=-1), dict(n=2 ** 31), dict(e=2 ** 31), dict(cams=0), dict(prob1=None), dict(pred=None),
                dict(ids=None), dict(info=None), dict(ws=None), dict(stride=0), dict(row=None), dict(col=None),
                dict(ws=0x100080), dict(logits=0x10004)):
        assert refused(lib, lambda: pp(**bad), _lib.E_ARG, "postprocess"), bad
    for bad in (dict(nbytes=need - 1), dict(nbytes=0)):
        assert refused(lib, lambda: pp(**bad), _lib.E_WORKSPACE, "postprocess"), bad
