"""Stand-in for the two `torch_scatter` functions the reference's Python programs use, over index_add_ (see
tests/refshim/lietorch/__init__.py for where it is visible).  `index` is one-dimensional along `dim`."""
import torch


def scatter_sum(src, index, dim=-1, out=None, dim_size=None):
    assert out is None and index.dim() == 1, "the stand-in serves a 1-d index and no `out`"
    dim = dim % src.dim()
    if dim_size is None:
        dim_size = int(index.max()) + 1 if index.numel() else 0
    shape = list(src.shape)
    shape[dim] = dim_size
    return torch.zeros(shape, dtype=src.dtype, device=src.device).index_add_(dim, index, src)


def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    total = scatter_sum(src, index, dim, out, dim_size)
    dim = dim % src.dim()
    count = torch.zeros(total.shape[dim], dtype=src.dtype, device=src.device)
    count.index_add_(0, index, torch.ones(index.shape[0], dtype=src.dtype, device=src.device))
    shape = [1] * total.dim()
    shape[dim] = -1
    return total / count.clamp(min=1).view(shape)


scatter_add = scatter_sum
