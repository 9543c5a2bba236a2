"""CPU: the three workspace queries of the build_graph family, pinned byte for byte.  Callers size their buffers by these
numbers and the layouts behind them (csrc/graph_build.hip, graph_knn.hip, graph_backward.hip) share one carving rule, so a
change of that rule shows here before it shows as a too-short workspace.  The literals were read from the library as built
before the three layouts were put on that rule."""
import pytest

# (n_nodes, feat_dim, mtmc_graph_workspace_bytes, mtmc_graph_knn_workspace_bytes, mtmc_graph_backward_workspace_bytes):
# N at 1, around a wave / a tile, S02's 450, the Gram regime edges 960 | 961 and 1920 | 1921, and the largest; the scalar
# Gram path (F = 6176); then the refused sizes -- the forward queries answer for any F >= 32, the backward's wants F % 32 == 0.
TABLE = (
    (1, 32, 1280, 1792, 2048),
    (1, 64, 1536, 2048, 2560),
    (1, 256, 3328, 3840, 5632),
    (1, 2048, 17664, 18176, 34304),
    (31, 32, 5120, 5632, 5888),
    (31, 64, 5376, 5888, 6400),
    (31, 256, 22528, 23040, 9472),
    (31, 2048, 36864, 37376, 38144),
    (62, 32, 16640, 17664, 17664),
    (62, 64, 16896, 17920, 18176),
    (62, 256, 80128, 81152, 21248),
    (62, 2048, 94464, 95488, 49920),
    (450, 32, 816640, 845824, 874752),
    (450, 64, 816896, 846080, 875264),
    (450, 256, 4058624, 4087808, 878336),
    (450, 2048, 4072960, 4102144, 907008),
    (960, 32, 3698176, 3821056, 3706112),
    (960, 64, 3698432, 3821312, 3706624),
    (960, 256, 18445568, 18568448, 3709696),
    (960, 2048, 18459904, 18582784, 3738368),
    (961, 32, 3706880, 3830272, 3834368),
    (961, 64, 3707136, 3830528, 3834880),
    (961, 256, 3708672, 3832064, 3837952),
    (961, 2048, 3723008, 3846400, 3866624),
    (1921, 32, 14785280, 15262208, 15039488),
    (1921, 64, 14785536, 15262464, 15040000),
    (1921, 256, 14787072, 15264000, 15043072),
    (1921, 2048, 14801408, 15278336, 15071744),
    (8000, 32, 256096256, 264160256, 256160512),
    (8000, 64, 256096512, 264160512, 256161024),
    (8000, 256, 256098048, 264162048, 256164096),
    (8000, 2048, 256112384, 264176384, 256192768),
    (46000, 32, 8464552448, 8729420800, 8467864832),
    (46000, 64, 8464552704, 8729421056, 8467865344),
    (46000, 256, 8464554240, 8729422592, 8467868416),
    (46000, 2048, 8464568576, 8729436928, 8467897088),
    (2048, 6176, 16851200, 17391872, 16916992),
    (0, 32, 0, 0, 0),
    (0, 2048, 0, 0, 0),
    (46001, 32, 0, 0, 0),
    (46001, 2048, 0, 0, 0),
    (450, 0, 0, 0, 0),
    (450, 2040, 832768, 861952, 0),
    (46000, 0, 0, 0, 0),
    (46000, 2040, 8464568576, 8729436928, 0),
)


@pytest.mark.parametrize("n,f,dense,knn,backward", TABLE)
def test_workspace_bytes_are_pinned(n, f, dense, knn, backward):
    from mtmc_mpn import _lib
    lib = _lib.load()
    got = (lib.mtmc_graph_workspace_bytes(n, f), lib.mtmc_graph_knn_workspace_bytes(n, f),
           lib.mtmc_graph_backward_workspace_bytes(n, f))
    assert got == (dense, knn, backward)


def test_the_table_covers_what_it_says():
    sizes = {(n, f) for n, f, *_ in TABLE}
    assert {(n, f) for n in (1, 31, 62, 450, 960, 961, 1921, 8000, 46000) for f in (32, 64, 256, 2048)} <= sizes
    assert (2048, 6176) in sizes
    zero = {(n, f) for n, f, d, k, b in TABLE if (d, k, b) == (0, 0, 0)}
    assert {n for n, _ in zero} >= {0, 46001} and {f for _, f in zero} >= {0}
    assert all(b == 0 and d > 0 and k > 0 for n, f, d, k, b in TABLE if f == 2040)
