"""CPU: scatter_add / scatter_mean / scatter_max are differentiable with respect to `src`.  The three forward ops have an
autograd kernel, the three backward ops exist with their schemas, a backward under FakeTensorMode leaves a gradient of src's
shape and dtype, and the three C entry points refuse bad arguments by name before any launch."""
import pytest
import torch

from abi_refusal import refused
from mtmc_mpn import _lib, torch_ops  # noqa: F401  (registers torch.ops.mtmc_mpn.*)

FORWARD = ("scatter_add", "scatter_mean", "scatter_max")
P = 0x10000                                  # an aligned address that is never read


@pytest.mark.parametrize("name", FORWARD)
def test_forward_ops_have_an_autograd_kernel(name):
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mtmc_mpn::" + name, "Autograd")


def test_backward_ops_are_registered_with_their_schemas():
    want = {"scatter_add_backward": "mtmc_mpn::scatter_add_backward(Tensor grad, Tensor index, int n_src) -> Tensor",
            "scatter_mean_backward": "mtmc_mpn::scatter_mean_backward(Tensor grad, Tensor index, int n_src) -> Tensor",
            "scatter_max_backward": "mtmc_mpn::scatter_max_backward(Tensor grad, Tensor arg, Tensor index, int n_src) -> Tensor"}
    for name, schema in want.items():
        assert str(getattr(torch.ops.mtmc_mpn, name).default._schema) == schema
        assert torch._C._dispatch_has_kernel_for_dispatch_key("mtmc_mpn::" + name, "CUDA")
        assert torch._C._dispatch_has_kernel_for_dispatch_key("mtmc_mpn::" + name, "Meta")
    # the forward schemas are what they were
    assert str(torch.ops.mtmc_mpn.scatter_max.default._schema) == \
        "mtmc_mpn::scatter_max(Tensor src, Tensor index, int dim, int? dim_size) -> (Tensor, Tensor)"
    for name in ("scatter_add", "scatter_mean"):
        assert str(getattr(torch.ops.mtmc_mpn, name).default._schema) == \
            f"mtmc_mpn::{name}(Tensor src, Tensor index, int dim, int? dim_size) -> Tensor"


@pytest.mark.parametrize("shape,dtype", [((700, 32), torch.float32), ((700,), torch.float16)])
@pytest.mark.parametrize("name", FORWARD)
def test_backward_under_fake_tensors_leaves_a_gradient_like_src(name, shape, dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        src = torch.empty(shape, dtype=dtype, requires_grad=True)
        index = torch.empty(700, dtype=torch.int64)
        out = getattr(torch.ops.mtmc_mpn, name)(src, index, 0, 50)
        if name == "scatter_max":
            out, arg = out
            assert arg.dtype == torch.int64 and not arg.requires_grad and arg.shape == out.shape
        assert out.shape == (50,) + shape[1:] and out.dtype == torch.float32
        assert out.requires_grad and out.grad_fn is not None
        out.sum().backward()
        assert src.grad is not None and src.grad.shape == src.shape and src.grad.dtype == dtype


def test_the_int64_form_needs_no_gradient():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = torch.ops.mtmc_mpn.scatter_add(torch.empty(700, dtype=torch.int64), torch.empty(700, dtype=torch.int64), 0, 50)
        assert out.shape == (50,) and out.dtype == torch.int64 and out.grad_fn is None and not out.requires_grad


def test_backward_ops_infer_shapes_without_a_gpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        g, index = torch.empty(50, 2, 4), torch.empty(700, dtype=torch.int32)
        for d in (torch.ops.mtmc_mpn.scatter_add_backward(g, index, 700), torch.ops.mtmc_mpn.scatter_mean_backward(g, index, 700),
                  torch.ops.mtmc_mpn.scatter_max_backward(g, torch.empty(50, 2, 4, dtype=torch.int64), index, 700)):
            assert d.shape == (700, 2, 4) and d.dtype == torch.float32
    with pytest.raises((NotImplementedError, RuntimeError)):           # no CPU kernel behind them
        torch.ops.mtmc_mpn.scatter_add_backward(torch.ones(3, 4), torch.zeros(5, dtype=torch.int64), 5)


def test_backward_refusals_name_their_entry_point():
    lib = _lib.load()

    def add(g=P, index=P, n_src=10, n_cols=4, dim_size=5, d=P):
        return lib.mtmc_scatter_add_backward(g, index, n_src, n_cols, dim_size, d, None)

    def mean(g=P, index=P, n_src=10, n_cols=4, dim_size=5, count=P, d=P):
        return lib.mtmc_scatter_mean_backward(g, index, n_src, n_cols, dim_size, count, d, None)

    def mx(g=P, arg=P, index=P, n_src=10, n_cols=4, dim_size=5, d=P):
        return lib.mtmc_scatter_max_backward(g, arg, index, n_src, n_cols, dim_size, d, None)
    bads = (dict(g=None), dict(index=None), dict(d=None), dict(n_src=-1), dict(n_cols=-1), dict(dim_size=-1),
            dict(g=P + 2), dict(d=P + 1), dict(index=P + 4))
    for bad in bads:
        assert refused(lib, lambda: add(**bad), _lib.E_ARG, "scatter_add_backward"), bad
        assert refused(lib, lambda: mean(**bad), _lib.E_ARG, "scatter_mean_backward"), bad
        assert refused(lib, lambda: mx(**bad), _lib.E_ARG, "scatter_max_backward"), bad
    assert refused(lib, lambda: mean(count=None), _lib.E_ARG, "scatter_mean_backward")      # no count scratch
    assert refused(lib, lambda: mx(arg=None), _lib.E_ARG, "scatter_max_backward")
    assert refused(lib, lambda: mx(arg=P + 4), _lib.E_ARG, "scatter_max_backward")
    # nothing to do: success with nothing enqueued, whatever the pointers
    for empty in (dict(n_src=0), dict(n_cols=0)):
        assert add(g=None, index=None, d=None, **empty) == 0
        assert mean(g=None, index=None, count=None, d=None, **empty) == 0
        assert mx(g=None, arg=None, index=None, d=None, **empty) == 0
