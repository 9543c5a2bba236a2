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
