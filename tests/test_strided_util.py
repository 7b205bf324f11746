"""strided_util (the carved operands of test_gpu_strided_operands.py) on the CPU: the view has the strides and offset
asked for, a single planted write into a gap is seen, a write inside the view is not."""
import pytest
import torch

import strided_util as su

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.uint8]


def _logical(shape, dtype):
    g = torch.Generator().manual_seed(len(shape) * 100 + shape[0])
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return torch.randn(shape, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad_t,pad_h,offset", [(0, 0, 0), (8, 0, 0), (0, 8, 16), (24, 16, 8), (4, 0, 4), (3, 1, 5)])
def test_carve_3d_strides_offset_and_values(dtype, pad_t, pad_h, offset):
    t = _logical((5, 3, 16), dtype)
    v = su.carve(t, pad_t, pad_h, offset, su.nan_bits(dtype))
    assert v.stride(2) == 1 and v.stride(1) == 16 + pad_h and v.stride(0) == 3 * (16 + pad_h) + pad_t
    assert v.storage_offset() == offset and v.shape == t.shape
    assert su.bits_equal(v, t)
    assert v.backing.numel() == offset + 4 * v.stride(0) + 2 * v.stride(1) + 15 + 1
    assert int(su.gap_mask(v).sum()) == v.backing.numel() - t.numel()
    assert su.gaps_untouched(v, su.nan_bits(dtype))
    if dtype.is_floating_point and (pad_t or pad_h or offset):  # the poison is a NaN of the dtype
        assert torch.isnan(v.backing[su.gap_mask(v)].float()).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pad_t,pad_h,offset", [(0, 0, 0), (8, 0, 8), (8, 8, 5), (4, 0, 4)])
def test_carve_2d(dtype, pad_t, pad_h, offset):
    t = _logical((7, 6), dtype)
    v = su.carve(t, pad_t, pad_h, offset, su.sentinel_bits(dtype))
    assert v.stride(1) == 1 + pad_h and v.stride(0) == 6 * (1 + pad_h) + pad_t and v.storage_offset() == offset
    assert su.bits_equal(v, t)
    assert su.gaps_untouched(v, su.sentinel_bits(dtype))
    if v.backing.numel() > t.numel():  # (held to the fill that was asked for, not to any fill)
        assert not su.gaps_untouched(v, su.nan_bits(dtype))


def test_carve_strided_4d_and_tail():
    t = _logical((3, 2, 4, 8), torch.bfloat16)  # an HND pool [pages, H, page, D] with two pad tokens per (page, head) and a padded page
    v = su.carve_strided(t, (2 * 6 * 8 + 16, 6 * 8, 8, 1), 8, su.nan_bits(t.dtype), tail=32)
    assert v.stride() == (112, 48, 8, 1) and v.storage_offset() == 8
    assert v.backing.numel() == 8 + 2 * 112 + 48 + 3 * 8 + 7 + 1 + 32
    assert su.bits_equal(v, t) and su.gaps_untouched(v, su.nan_bits(t.dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_write_into_any_gap_is_detected(dtype):
    fill = su.sentinel_bits(dtype)
    t = _logical((4, 2, 8), dtype)
    ref = su.carve(t, 8, 8, 8, fill, tail=3)
    gaps = torch.nonzero(su.gap_mask(ref)).reshape(-1).tolist()
    # before the first row, inside a head pad, inside a token pad, the tail -- and every other gap element
    assert {0, 7, 8 + 8, 8 + 2 * 16, ref.backing.numel() - 1} <= set(gaps)
    for i in gaps:
        v = su.carve(t, 8, 8, 8, fill, tail=3)
        v.backing[i] = 1 if dtype == torch.uint8 else 0.5
        assert not su.gaps_untouched(v, fill), i


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_gap_comparison_is_by_bits(dtype):
    """Another NaN, or the fill's value with one mantissa bit changed, is a touched gap."""
    t = _logical((3, 2, 8), dtype)
    v = su.carve(t, 8, 0, 0, su.nan_bits(dtype))
    v.backing[16] = float("nan")  # torch's NaN: not the poison's payload
    assert torch.isnan(v.backing[16]) and not su.gaps_untouched(v, su.nan_bits(dtype))
    w = su.carve(t, 8, 0, 0, su.nan_bits(dtype))
    assert su.gaps_untouched(w, su.nan_bits(dtype))  # NaN poison equals itself


@pytest.mark.parametrize("dtype", DTYPES)
def test_writes_inside_the_view_are_not_flagged(dtype):
    fill = su.sentinel_bits(dtype)
    t = _logical((4, 2, 8), dtype)
    v = su.carve(t, 8, 8, 8, fill)
    v.copy_(torch.zeros_like(t))
    v[3, 1, 7] = 1
    v[0, 0, 0] = 1
    assert su.gaps_untouched(v, fill)
    # ... not even a write of the fill's own bits
    v[1, 1, 1] = v.backing[0]
    assert su.gaps_untouched(v, fill)


def test_bits_equal_tells_signed_zero_and_nan():
    a = torch.tensor([0.0, float("nan")], dtype=torch.float16)
    assert su.bits_equal(a, a.clone())
    assert not su.bits_equal(a, torch.tensor([-0.0, float("nan")], dtype=torch.float16))
