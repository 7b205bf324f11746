"""Strided (non-contiguous) operands for the kernel tests: a logical tensor placed inside a larger backing buffer whose every
other element holds a known bit pattern, and the check that a kernel left those elements alone.

Two fills are used (bit patterns, so that a NaN compares equal to itself):
  * NaN poison (``nan_bits``) around INPUTS: a kernel that reads an element outside the logical rows computes NaN;
  * a sentinel (``sentinel_bits``) around OUTPUTS: 0x7B7B for 16-bit (bf16 1.3e36, fp16 61280: no attention output equals
    it), a fixed odd float for fp32 -- a store outside the logical rows is seen even where it lands inside the allocation.
"""
import torch

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _signed(bits: int, size: int) -> int:
    if size == 1:
        return bits & 0xFF
    top = 1 << (8 * size)
    bits &= top - 1
    return bits - top if bits >= top >> 1 else bits


def nan_bits(dtype) -> int:
    """A quiet NaN of `dtype` as a bit pattern (fp8 e4m3fn: 0x7F; integer byte pools: 0xA5, no NaN exists)."""
    return {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01, torch.float32: 0x7FC00001, torch.float8_e4m3fn: 0x7F,
            torch.uint8: 0xA5}[dtype]


def sentinel_bits(dtype) -> int:
    return {torch.bfloat16: 0x7B7B, torch.float16: 0x7B7B, torch.float32: 0x4B7B7B7B, torch.float8_e4m3fn: 0x7B,
            torch.uint8: 0x7B}[dtype]


def carve_strided(t, strides, offset, fill, tail=0):
    """`t`'s values as a view with the given element `strides` and storage `offset` of a fresh 1-D backing buffer (on t's
    device) whose other elements hold the bit pattern `fill`; `tail` more fill elements follow the last row.  The view
    carries the buffer as ``.backing``."""
    size = t.element_size()
    n = offset + sum((s - 1) * st for s, st in zip(t.shape, strides) if s > 0) + 1 + tail
    raw = torch.full((n,), _signed(fill, size), dtype=_INT[size], device=t.device)
    backing = raw.view(t.dtype)
    view = backing.as_strided(tuple(t.shape), tuple(strides), offset)
    view.copy_(t)
    view.backing = backing
    return view


def carve(t, pad_t=0, pad_h=0, offset=0, fill=None, tail=0):
    """A logical [N, H, D] tensor inside a larger backing buffer: stride(2) == 1, stride(1) == D + pad_h,
    stride(0) == H * (D + pad_h) + pad_t, storage offset `offset` (elements).  2-D [N, C] likewise with one element per
    "head": stride(1) == 1 + pad_h, stride(0) == C * (1 + pad_h) + pad_t.  Every element of the backing buffer outside the
    view holds the bit pattern `fill` (default: NaN poison)."""
    if fill is None:
        fill = nan_bits(t.dtype)
    if t.dim() == 3:
        sh = t.shape[2] + pad_h
        strides = (t.shape[1] * sh + pad_t, sh, 1)
    elif t.dim() == 2:
        sh = 1 + pad_h
        strides = (t.shape[1] * sh + pad_t, sh)
    else:
        raise ValueError(f"carve: 2-D or 3-D tensors, got {tuple(t.shape)}")
    return carve_strided(t, strides, offset, fill, tail)


def gap_mask(view):
    """bool[backing.numel()]: True at every element of view.backing that is NOT an element of the view."""
    backing = view.backing
    idx = torch.arange(backing.numel(), device=backing.device).as_strided(tuple(view.shape), view.stride(), view.storage_offset())
    mask = torch.ones(backing.numel(), dtype=torch.bool, device=backing.device)
    mask[idx.reshape(-1)] = False
    return mask


def gaps_untouched(view, fill) -> bool:
    """True iff every element of view.backing outside the logical view still holds `fill`, compared as bits."""
    backing = view.backing
    size = backing.element_size()
    raw = backing.view(_INT[size])
    return bool((raw[gap_mask(view)] == _signed(fill, size)).all().item())


def bits_equal(a, b) -> bool:
    """Two tensors of one dtype and shape hold the same bits (NaN == NaN, -0 != +0)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = _INT[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))
