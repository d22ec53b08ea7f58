"""What every embedding op (neighbors, clusters, latent_gaussian, fingerprints) does to its arguments before it calls the library, once: the
matrix and per-row checks, the row pitch, the scratch of an entry and the placeholder for a pointer that is never followed.
`who` is the public function that was called: every ValueError starts with its name."""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import check, lib


def matrix(t, name: str, who: str) -> None:
    if not torch.is_tensor(t) or t.dim() != 2:
        raise ValueError(f"{who}: `{name}` must be a matrix [rows, H] (got {type(t).__name__}"
                         + (f" of shape {tuple(t.shape)})" if torch.is_tensor(t) else ")"))
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: `{name}` must be float32 (got {t.dtype})")


def rows(t, name: str, who: str, min_width: int = 0) -> torch.Tensor:
    """a float32 GPU matrix whose rows are contiguous (any row pitch is taken as it is)"""
    matrix(t, name, who)
    if t.shape[1] < min_width:
        raise ValueError(f"{who}: `{name}` has rows of width {t.shape[1]}")
    if not t.is_cuda:
        raise ValueError(f"{who}: `{name}` must live on the GPU (got {t.device}); there is no CPU path")
    t = t.detach()
    if t.shape[1] > 1 and t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def word_matrix(t, name: str, who: str, min_width: int = 1, max_width: int = None) -> None:
    if not torch.is_tensor(t) or t.dim() != 2:
        raise ValueError(f"{who}: `{name}` must be a matrix of words [rows, W] (got {type(t).__name__}"
                         + (f" of shape {tuple(t.shape)})" if torch.is_tensor(t) else ")"))
    if t.dtype != torch.int32:
        raise ValueError(f"{who}: `{name}` must be int32 words (got {t.dtype})")
    if t.shape[1] < min_width or (max_width is not None and t.shape[1] > max_width):
        raise ValueError(f"{who}: `{name}` has rows of {t.shape[1]} words"
                         + (f" (at most {max_width})" if max_width is not None and t.shape[1] > max_width else ""))


def word_rows(t, name: str, who: str, min_width: int = 1, max_width: int = None) -> torch.Tensor:
    """an int32 GPU matrix of bit words [rows, W] whose rows are contiguous (any row pitch is taken as it is)"""
    word_matrix(t, name, who, min_width, max_width)
    if not t.is_cuda:
        raise ValueError(f"{who}: `{name}` must live on the GPU (got {t.device}); there is no CPU path")
    t = t.detach()
    if t.shape[1] > 1 and t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def pitch(x: torch.Tensor) -> int:
    """the row pitch the C entries take (a single row has no stride to speak of: its width)"""
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


def group(g, n: int, dev, name: str, who: str) -> torch.Tensor:
    """one integer per row -> int32 [n] on `dev`"""
    g = torch.as_tensor(g)
    if g.numel() != n:
        raise ValueError(f"{who}: `{name}` has {g.numel()} entries for {n} rows")
    if g.is_floating_point():
        raise ValueError(f"{who}: `{name}` must hold integers")
    return g.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()


def per_row(t, n: int, dev, name: str, who: str, dtype=torch.float32) -> torch.Tensor:
    """one float32 (or `dtype`) per row -> contiguous [n].  dev: the matrix's device, which a tensor has to be on; None
    (bank_sqnorm, bank_popcount): anything torch.as_tensor takes that ends up on a GPU"""
    if dev is None:
        t = torch.as_tensor(t)
    if not torch.is_tensor(t) or t.dtype != dtype or t.numel() != n or (t.device != dev if dev is not None else not t.is_cuda):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        kind = str(dtype).replace("torch.", "")
        raise ValueError(f"{who}: `{name}` must be {n} {kind} values on {'the GPU' if dev is None else dev} (got {got})")
    return t.detach().reshape(-1).contiguous()


def scratch(sizer: str, dev, *shape):
    """(uint8 tensor, its size as a c_size_t) as lib().<sizer>(*shape, &bytes) asks: an entry's workspace, from torch's allocator
    on the current stream"""
    nbytes = C.c_size_t()
    check(getattr(lib(), sizer)(*shape, C.byref(nbytes)), sizer)
    return torch.empty(nbytes.value, dtype=torch.uint8, device=dev), C.c_size_t(nbytes.value)


def empty_bank(H: int, dev, grouped: bool, dtype=torch.float32):
    """(bank, b_group) to pass for a bank without rows: the C entries want a bank pointer (and, with groups, a group pointer) even
    then; one zero row in a group of its own that no kernel reads"""
    return (torch.zeros(1, H, dtype=dtype, device=dev),
            torch.full((1,), -1, dtype=torch.int32, device=dev) if grouped else None)


def placeholder(dev, dtype=torch.float32) -> torch.Tensor:
    """one element that is never read or written: the C entries want non-null pointers for empty arrays too"""
    return torch.empty(1, dtype=dtype, device=dev)
