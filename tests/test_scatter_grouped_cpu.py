"""CPU: the stable grouping and the repeatable scatter forwards are registered, trace on meta tensors, refuse CPU tensors
with the package's text, and their two size queries answer without a GPU."""
import pytest
import torch

import mtmc_mpn
from mtmc_mpn import _lib, ops, torch_ops  # noqa: F401  (registers torch.ops.mtmc_mpn.*)

GROUPED = ("scatter_add_grouped", "scatter_mean_grouped", "scatter_max_grouped")


def test_the_new_ops_are_registered_with_their_schemas():
    args = "(Tensor src, Tensor index, Tensor perm, Tensor offsets)"
    want = {"group_by_index": "mtmc_mpn::group_by_index(Tensor index, int num_groups) -> (Tensor, Tensor)",
            "scatter_add_grouped": f"mtmc_mpn::scatter_add_grouped{args} -> Tensor",
            "scatter_mean_grouped": f"mtmc_mpn::scatter_mean_grouped{args} -> Tensor",
            "scatter_max_grouped": f"mtmc_mpn::scatter_max_grouped{args} -> (Tensor, Tensor)"}
    for name, schema in want.items():
        assert str(getattr(torch.ops.mtmc_mpn, name).default._schema) == schema
        assert torch._C._dispatch_has_kernel_for_dispatch_key("mtmc_mpn::" + name, "CUDA")
        assert torch._C._dispatch_has_kernel_for_dispatch_key("mtmc_mpn::" + name, "Meta")
    for name in GROUPED:
        assert torch._C._dispatch_has_kernel_for_dispatch_key("mtmc_mpn::" + name, "Autograd")
    # the six schemas from before are what they were
    assert str(torch.ops.mtmc_mpn.scatter_add.default._schema) == \
        "mtmc_mpn::scatter_add(Tensor src, Tensor index, int dim, int? dim_size) -> Tensor"
    assert str(torch.ops.mtmc_mpn.scatter_max_backward.default._schema) == \
        "mtmc_mpn::scatter_max_backward(Tensor grad, Tensor arg, Tensor index, int n_src) -> Tensor"


def test_the_public_names_are_exported():
    assert mtmc_mpn.Grouping._fields == ("index", "perm", "offsets", "num_groups")
    assert "Grouping" in mtmc_mpn.__all__ and "group_by_index" in mtmc_mpn.__all__
    assert callable(mtmc_mpn.group_by_index)


@pytest.mark.parametrize("shape,dtype", [((700, 32), torch.float32), ((700,), torch.float16), ((700, 2, 3), torch.float32)])
def test_fakes_give_shapes_and_dtypes_on_meta_tensors(shape, dtype):
    index = torch.empty(700, dtype=torch.int64, device="meta")
    perm, offsets = torch.ops.mtmc_mpn.group_by_index(index, 50)
    assert perm.shape == (700,) and offsets.shape == (51,) and perm.dtype == offsets.dtype == torch.int64
    src = torch.empty(shape, dtype=dtype, device="meta")
    for name in GROUPED:
        out = getattr(torch.ops.mtmc_mpn, name)(src, index, perm, offsets)
        if name == "scatter_max_grouped":
            out, arg = out
            assert arg.shape == out.shape and arg.dtype == torch.int64
        assert out.shape == (50,) + shape[1:] and out.dtype == torch.float32


@pytest.mark.parametrize("name", GROUPED)
def test_backward_under_fake_tensors_leaves_a_gradient_like_src(name):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        src = torch.empty((700, 4), dtype=torch.float16, requires_grad=True)
        index = torch.empty(700, dtype=torch.int64)
        perm, offsets = torch.ops.mtmc_mpn.group_by_index(index, 50)
        out = getattr(torch.ops.mtmc_mpn, name)(src, index, perm, offsets)
        out = out[0] if isinstance(out, tuple) else out
        assert out.requires_grad
        out.sum().backward()
        assert src.grad.shape == src.shape and src.grad.dtype == torch.float16


def test_cpu_tensors_are_refused_with_the_usual_text():
    src, index = torch.ones(5, 4), torch.zeros(5, dtype=torch.int64)
    text = "tensors must be on a ROCm GPU"
    with pytest.raises(RuntimeError, match=text):
        mtmc_mpn.group_by_index(index, 3)
    for fn in (ops.scatter_add, ops.scatter_mean, ops.scatter_max):
        with pytest.raises(RuntimeError, match=text):
            fn(src, index, dim_size=3, deterministic=True)
        with pytest.raises(RuntimeError, match=text):
            fn(src, index, deterministic=mtmc_mpn.Grouping(index, index, torch.zeros(4, dtype=torch.int64), 3))
    with pytest.raises(RuntimeError, match=text):
        mtmc_mpn.pool_tracklets(torch.ones(5, 4), grouping=mtmc_mpn.Grouping(index, index, torch.zeros(4, dtype=torch.int64), 3))
    with pytest.raises((NotImplementedError, RuntimeError)):               # no CPU kernel behind the registered ops
        torch.ops.mtmc_mpn.scatter_add_grouped(src, index, index, torch.zeros(4, dtype=torch.int64))


def test_deterministic_needs_dim_size_and_says_why():
    src, index = torch.ones(5, 4), torch.zeros(5, dtype=torch.int64)
    for fn in (ops.scatter_add, ops.scatter_mean, ops.scatter_max):
        with pytest.raises(ValueError, match="dim_size.*host read"):
            fn(src, index, deterministic=True)
        with pytest.raises(NotImplementedError):
            fn(src, index, out=src, dim_size=3, deterministic=True)
        with pytest.raises(TypeError):
            fn(src, index, dim_size=3, deterministic="yes")
    g = mtmc_mpn.Grouping(index, index, torch.zeros(4, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="3 groups"):
        ops.scatter_add(src, index, dim_size=4, deterministic=g)
    with pytest.raises(ValueError):
        mtmc_mpn.group_by_index(index, -1)
    with pytest.raises(ValueError):
        mtmc_mpn.pool_tracklets(torch.ones(5, 4), [5], grouping=g)


def test_size_queries_need_no_gpu():
    lib = _lib.load()
    assert lib.mtmc_group_tile_rows() >= 64 and lib.mtmc_group_tile_rows() % 64 == 0
    group, scat = lib.mtmc_group_by_index_workspace_bytes, lib.mtmc_scatter_grouped_workspace_bytes
    for bits in (0, 1, 8, 11):
        sizes = [group(n, 450, bits) for n in (1, 1000, 37844, 10 ** 6, 10 ** 8)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (bits, sizes)
    assert group(37844, 70000, 8) > group(37844, 200, 8)            # more than one pass: the (key, row) pairs
    assert group(2 ** 31, 450, 0) == 0 and group(-1, 450, 0) == 0 and group(100, 2 ** 31, 0) == 0 and group(100, -1, 0) == 0
    assert group(100, 450, 12) == 0 and group(100, 450, -1) == 0
    assert group(2 ** 31 - 1, 2 ** 31 - 1, 0) > 0
    sizes = [scat(n, 32) for n in (0, 1, 1000, 150454, 10 ** 7)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert scat(1000, 0) == 0 and scat(1000, -4) == 0 and scat(2 ** 31, 4) == 0 and scat(-1, 4) == 0
    assert scat(10 ** 7, 32) < 10 ** 7 * 32 * 4                   # the partials are a fraction of src


def test_refusals_name_their_entry_point():
    from abi_refusal import refused
    lib = _lib.load()
    p = 0x10000

    def group(index=p, n_rows=10, n_groups=5, bits=0, perm=p, offsets=p, info=p, ws=p, ws_bytes=1 << 20):
        return lib.mtmc_group_by_index(index, n_rows, n_groups, bits, perm, offsets, info, ws, ws_bytes, None)

    def scat(src=p, n_src=10, n_cols=4, perm=p, offsets=p, dim_size=5, mode=0, out=p, arg=None, ws=p, ws_bytes=1 << 20):
        return lib.mtmc_scatter_grouped(src, n_src, n_cols, perm, offsets, dim_size, mode, out, arg, ws, ws_bytes, None)
    for bad in (dict(index=None), dict(perm=None), dict(offsets=None), dict(n_rows=-1), dict(n_groups=-1), dict(bits=12),
                dict(n_rows=2 ** 31), dict(perm=p + 4), dict(info=p + 2), dict(ws=None), dict(ws_bytes=16)):
        assert refused(lib, lambda: group(**bad), _lib.E_ARG, "group_by_index"), bad
    for bad in (dict(src=None), dict(perm=None), dict(offsets=None), dict(out=None), dict(n_src=-1), dict(n_cols=0),
                dict(dim_size=-1), dict(mode=3), dict(perm=p + 4), dict(out=p + 2), dict(ws=None), dict(ws_bytes=16)):
        assert refused(lib, lambda: scat(**bad), _lib.E_ARG, "scatter_grouped"), bad
    assert scat(src=None, perm=None, offsets=None, out=None, ws=None, dim_size=0) == 0      # nothing to do
