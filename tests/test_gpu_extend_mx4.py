"""Extend attention straight over the 4-bit (MXFP4 block-16) pool, rx_extend_attn_mx4 / rx::extend_mx4_kernel: every instance
against the fp64 oracle fed the exactly dequantised bytes (the bound of every 16-bit extend instance: the unpack is exact and
the output is rounded once), the prefix-only form with its LSE, the refusals, and the backend's two routes."""
import numpy as np
import pytest
import torch

import parity_util as parity
from oracle import radix_oracle as orc
from test_gpu_kv_mx4 import DT, PS, _canon, _dev, _random_pool, mx4_dequant

DEV = "cuda"
PRE, EXT = [0, 70, 200, 33], [130, 40, 9, 1]   # no prefix; inside one tile; ending inside a tile; rows crossing a 64-row block; one token
# dtype, D, index width, pool, (Hq, Hkv), logit cap + scales + not causal.  Pools: "nhd1" page 1 with scattered slots, "nhd16" /
# "hnd" pages of 16 with shuffled page ids.  NHD pages are slot-major, so the eight non-LINEAR instances are the HND pools
# with more than one kv head; one kv head makes HND pages slot-major too.
CASES = [
    ("bf16", 128, "int", "nhd1", (4, 4), False), ("bf16", 128, "int", "hnd", (4, 2), True),
    ("bf16", 128, "long", "nhd16", (8, 2), False), ("bf16", 128, "long", "hnd", (4, 4), False),
    ("bf16", 64, "int", "hnd", (8, 1), False), ("bf16", 64, "int", "hnd", (8, 2), False),
    ("bf16", 64, "long", "nhd1", (16, 1), False), ("bf16", 64, "long", "hnd", (4, 2), False),
    ("f16", 128, "int", "nhd16", (16, 1), False), ("f16", 128, "int", "hnd", (8, 2), False),
    ("f16", 128, "long", "hnd", (16, 1), False), ("f16", 128, "long", "hnd", (4, 4), False),
    ("f16", 64, "int", "nhd1", (4, 2), True), ("f16", 64, "int", "hnd", (4, 4), False),
    ("f16", 64, "long", "nhd16", (8, 1), False), ("f16", 64, "long", "hnd", (8, 2), False),
]


def _np(t):
    return t.view(torch.uint16).numpy() if t.dtype == torch.bfloat16 else t.numpy()


def _batch(dt, d, ix, lay, heads, seed):
    """A random packed pool, the batch's index arrays and operands; host arrays for the oracle, device tensors for the call."""
    (hq, hkv), dtype, ps = heads, DT[dt], 1 if lay == "nhd1" else PS
    rng = np.random.default_rng(seed)
    n_pages = sum(-(-n // PS) for n in PRE) + 3
    if ps == 1:
        slots = rng.permutation(np.arange(1, n_pages * PS))[: sum(PRE)]
    else:
        ids = rng.permutation(np.arange(1, n_pages))
        first = np.cumsum([0] + [-(-n // PS) for n in PRE])
        slots = np.concatenate([(ids[first[i]: first[i + 1], None] * PS + np.arange(PS)).reshape(-1)[:n] for i, n in enumerate(PRE)])
    pool = _random_pool(rng, n_pages * PS, hkv, d)
    T = sum(EXT)
    q, k, v = (torch.from_numpy(rng.standard_normal((T, h, d)).astype(np.float32)).to(dtype) for h in (hq, hkv, hkv))
    host = dict(q=_np(q), k=_np(k), v=_np(v), kb=mx4_dequant(pool[0], pool[1]), vb=mx4_dequant(pool[2], pool[3]),
                qo=np.concatenate([[0], np.cumsum(EXT)]).astype(np.int64), ip=np.concatenate([[0], np.cumsum(PRE)]).astype(np.int32),
                ii=slots.astype(np.int64))
    wide = torch.int64 if ix == "long" else torch.int32
    kd, ksd, vd, vsd = (_dev(a, lay == "hnd", flat=i % 2 == 1) for i, a in enumerate(pool))
    dev = dict(q=q.to(DEV), k=k.to(DEV), v=v.to(DEV), kd=kd, vd=vd, qo=torch.from_numpy(host["qo"]).to(DEV).to(wide),
               ip=torch.from_numpy(host["ip"]).to(DEV), ii=torch.from_numpy(host["ii"]).to(DEV).to(wide),
               kw=dict(page_size=ps, k_scale_buffer=ksd, v_scale_buffer=vsd))
    return host, dev


def _dispatch(dt, d, ix, lay, heads):
    linear = "false" if lay == "hnd" and heads[1] > 1 else "true"
    return f"extend_mx4_kernel<rx::{dt.upper()}, {d}, {ix}, {linear}>|g{heads[0] // heads[1]}"


@pytest.mark.gpu
@pytest.mark.parametrize("dt,d,ix,lay,heads,extras", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_every_instance_matches_the_oracle(dt, d, ix, lay, heads, extras):
    from sglang_amd import lib as rxlib
    from sglang_amd import ops

    h, g = _batch(dt, d, ix, lay, heads, d + heads[0] + len(ix + lay))
    kw = dict(logit_cap=30.0, k_scale=0.9, v_scale=1.25, is_causal=False) if extras else dict(is_causal=True)
    want, absw = orc.extend_attention(h["q"], h["k"], h["v"], h["kb"], h["vb"], h["qo"], h["ip"], h["ii"], sm_scale=d ** -0.5,
                                      return_absw=True, **kw)
    o = torch.full_like(g["q"], float("nan"))
    ops.extend_attention_fwd(g["q"], g["k"], g["v"], o, g["kd"], g["vd"], g["qo"], g["ip"], g["ii"], None, kw["is_causal"], None,
                             max(EXT), kw.get("k_scale", 1.0), kw.get("v_scale", 1.0), sm_scale=d ** -0.5,
                             logit_cap=kw.get("logit_cap", 0.0), **g["kw"])
    torch.cuda.synchronize()
    assert rxlib.last_dispatch() == _dispatch(dt, d, ix, lay, heads)
    parity.check_out(o.float().cpu().numpy(), want, DT[dt], ("extend_mx4", dt, d, ix, lay, heads, extras), ulps=1, absw=absw)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,d,lay,heads", [("bf16", 128, "hnd", (8, 2)), ("f16", 64, "nhd1", (4, 4))], ids=lambda v: str(v).replace(" ", ""))
def test_prefix_only_form_and_its_lse(dt, d, lay, heads):
    """skip_extend: the keys are the prefix, every query sees all of it; the request without a prefix gets zeros and lse = -inf.
    The LSE is an fp32 log-sum of fp32 scores: 1e-4 absolute (tests/test_gpu_parity.py holds its 16-bit-score LSEs to 2e-3)."""
    from sglang_amd import ops

    h, g = _batch(dt, d, "long", lay, heads, d)
    want, want_lse = orc.extend_attention(h["q"], h["k"], h["v"], h["kb"], h["vb"], h["qo"], h["ip"], h["ii"], sm_scale=d ** -0.5,
                                          is_causal=True, skip_extend=True, return_lse=True)
    _, absw = orc.extend_attention(h["q"], h["k"], h["v"], h["kb"], h["vb"], h["qo"], h["ip"], h["ii"], sm_scale=d ** -0.5,
                                   is_causal=True, skip_extend=True, return_absw=True)
    o = torch.full_like(g["q"], float("nan"))
    lse = torch.full(o.shape[:2], float("nan"), dtype=torch.float32, device=DEV)
    ops.extend_attention_fwd(g["q"], g["k"], g["v"], o, g["kd"], g["vd"], g["qo"], g["ip"], g["ii"], None, True, None, max(EXT),
                             1.0, 1.0, sm_scale=d ** -0.5, skip_extend=True, lse_extend=lse, **g["kw"])
    got, got_lse = o.float().cpu().numpy(), lse.cpu().numpy()
    assert not got[: EXT[0]].any() and np.all(np.isneginf(got_lse[: EXT[0]])) and np.all(np.isneginf(want_lse[: EXT[0]]))
    parity.check_out(got, want, DT[dt], ("extend_mx4 prefix only", dt, d), ulps=1, absw=absw)
    np.testing.assert_allclose(got_lse, want_lse, atol=1e-4, rtol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["skip_prefix", "empty_kv_indices"])
def test_a_call_without_a_prefix_is_the_16_bit_entrys(how):
    """skip_prefix, and the empty index list that ops turns into it: nothing is read from the pool, rx_extend_attn serves it."""
    from sglang_amd import lib as rxlib
    from sglang_amd import ops

    h, g = _batch("bf16", 128, "long", "hnd", (8, 2), 7)
    ip, ii = (g["ip"], g["ii"]) if how == "skip_prefix" else (torch.zeros_like(g["ip"]), g["ii"][:0])
    want, absw = orc.extend_attention(h["q"], h["k"], h["v"], h["kb"], h["vb"], h["qo"], h["ip"], h["ii"], sm_scale=128 ** -0.5,
                                      is_causal=True, skip_prefix=True, return_absw=True)
    o = torch.full_like(g["q"], float("nan"))
    ops.extend_attention_fwd(g["q"], g["k"], g["v"], o, g["kd"], g["vd"], g["qo"], ip, ii, None, True, None, max(EXT), 1.0, 1.0,
                             sm_scale=128 ** -0.5, skip_prefix=how == "skip_prefix", **g["kw"])
    torch.cuda.synchronize()
    assert "extend_mx4_kernel" not in rxlib.last_dispatch() and rxlib.last_dispatch().startswith("extend_")
    parity.check_out(o.float().cpu().numpy(), want, torch.bfloat16, ("extend_mx4 no prefix", how), ulps=1, absw=absw)


def test_the_default_route_is_the_measured_regime():
    """option extend_mx4_native = -1: one 64-row block at most, and a grid of at least half the CUs."""
    from sglang_amd import lib as rxlib
    from sglang_amd.attention.backend import mx4_extend_native_rule as rule

    assert rxlib.get_option("extend_mx4_native") == -1
    assert rule(16, 4, 64, 8, 256) and not rule(17, 4, 64, 8, 256)      # 64 rows / 68 rows
    assert rule(16, 4, 16, 8, 256) and not rule(16, 4, 15, 8, 256)      # 128 workgroups / 120 on 256 CUs
    assert rule(64, 1, 32, 8, 256) and not rule(16, 4, 1, 8, 256) and not rule(512, 4, 32, 8, 256)


def test_refused_options_raise_and_null_params_fail_on_the_host():
    from sglang_amd import lib as rxlib
    from sglang_amd import ops

    assert rxlib.load().rx_extend_attn_mx4(None, None, None) == -1 and b"null" in rxlib.load().rx_last_error()
    q = torch.zeros(2, 4, 128, dtype=torch.bfloat16)
    kb, sb, x = torch.zeros(32, 4, 64, dtype=torch.uint8), torch.zeros(32, 32, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)
    fwd = (q, q, q, q, kb, kb, x, x, x)
    base = dict(custom_mask=None, is_causal=True, mask_indptr=None, max_len_extend=2, k_scale=1.0, v_scale=1.0)
    for name, val in (("custom_mask", x), ("sliding_window_size", 8), ("sinks", q), ("xai_temperature_len", 4),
                      ("score_mod", ops.relative_bias_score_mod), ("unified_prefix_lens", x), ("q_pack", 2), ("window_kv_offsets", x)):
        with pytest.raises(NotImplementedError, match=name):
            ops.extend_attention_fwd(*fwd, **dict(base, **{name: val}), k_scale_buffer=sb, v_scale_buffer=sb)
    with pytest.raises(ValueError, match="together"):
        ops.extend_attention_fwd(*fwd, **base, k_scale_buffer=sb)


@pytest.mark.gpu
@pytest.mark.parametrize("hnd", [False, True], ids=["nhd", "hnd"])
def test_backend_routes_an_fp4_pool_extend_natively_or_through_the_gather(hnd):
    from sglang_amd import lib as rxlib
    from sglang_amd import ops
    from sglang_amd.attention.backend import HipRadixAttnBackend
    from sglang_amd.attention.radix_attention import RadixAttention
    from sglang_amd.forward_batch import ForwardBatch
    from sglang_amd.mem_cache.allocator import PagedTokenToKVPoolAllocator
    from sglang_amd.mem_cache.memory_pool import MHATokenToKVPoolFP4, ReqToTokenPool

    hq, hkv, d, dtype, size, pre, ext = 8, 2, 128, torch.bfloat16, 1024, [0, 70, 33], [40, 9, 20]
    pool = MHATokenToKVPoolFP4(size, PS, dtype, hkv, d, 1, DEV, use_hnd=hnd)
    r2t = ReqToTokenPool(8, 512, DEV)
    alloc = PagedTokenToKVPoolAllocator(size, PS, dtype, DEV, pool, debug_mode=True)
    MC = type("MC", (), dict(num_attention_heads=hq, num_key_value_heads=hkv, context_len=512))
    MR = type("MR", (), dict(device=DEV, req_to_token_pool=r2t, token_to_kv_pool=pool, token_to_kv_pool_allocator=alloc, model_config=MC,
                             page_size=PS, dtype=dtype, server_args=type("SA", (), dict(triton_attention_num_kv_splits=8))))
    backend, layer = HipRadixAttnBackend(MR), RadixAttention(hq, d, d ** -0.5, hkv, 0)
    gen = torch.Generator().manual_seed(5)
    rand = lambda *shape: torch.randn(*shape, generator=gen).to(dtype).to(DEV)  # noqa: E731
    rows = r2t.alloc(3)
    rpi = torch.tensor(rows, dtype=torch.int64, device=DEV)

    def grow(old, new):   # alloc_for_extend: slots + req_to_token rows
        o_, n_ = torch.tensor(old, dtype=torch.int64), torch.tensor(new, dtype=torch.int64)
        last = torch.tensor([int(r2t.req_to_token[r, p - 1]) if p > 0 else -1 for r, p in zip(rows, old)], dtype=torch.int64, device=DEV)
        out = alloc.alloc_extend(o_.to(DEV), o_, n_.to(DEV), n_, last, int((n_ - o_).sum()))
        ops.write_req_to_token(r2t.req_to_token, rpi, None, o_.to(DEV), n_.to(DEV), (n_ - o_).to(DEV), out)
        return out

    pool.set_kv_buffer(layer, grow([0, 0, 0], pre), rand(sum(pre), hkv, d), rand(sum(pre), hkv, d))
    seq, T = [p + e for p, e in zip(pre, ext)], sum(ext)
    loc = grow(pre, seq)
    q, k, v = rand(T, hq * d), rand(T, hkv * d), rand(T, hkv * d)
    slots = pool.num_pages * PS
    kbo, vbo = (mx4_dequant(_canon(a, hnd, np.empty((slots, hkv, d // 2))), _canon(s, hnd, np.empty((slots, hkv, d // 16))))
                for a, s in zip(pool.get_mx4_buffers(0)[:2], pool.get_mx4_buffers(0)[2:]))
    fb = ForwardBatch.for_extend(rpi, torch.tensor(seq, device=DEV), loc, pre, ext)
    ip, ii = orc.build_kv_indices(r2t.req_to_token.cpu().numpy(), np.array(rows), np.array(pre))
    bits = lambda t, *shape: t.view(*shape).cpu().view(torch.uint16).numpy()  # noqa: E731
    want, absw = orc.extend_attention(bits(q, T, hq, d), bits(k, T, hkv, d), bits(v, T, hkv, d), kbo, vbo,
                                      np.concatenate([[0], np.cumsum(ext)]).astype(np.int64), ip, ii, is_causal=True,
                                      sm_scale=d ** -0.5, return_absw=True)
    dense = sum(pre) * hkv * d * 2 * 2   # the gather route's 16-bit copy of the prefix rows, K and V
    for native in (1, 0):
        with rxlib.option("extend_mx4_native", native):
            backend.init_forward_metadata(fb)   # (the option is read with the forward's metadata)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            held = torch.cuda.memory_allocated()
            o = layer(q, k, v, fb, backend)   # (stores the same new rows again on the second pass)
            torch.cuda.synchronize()
            grew = torch.cuda.max_memory_allocated() - held - o.nbytes
        name = rxlib.last_dispatch()
        assert ("extend_mx4_kernel" in name) == bool(native) and name.startswith("extend_"), name
        if native:
            assert grew < dense, (grew, dense)
        parity.check_out(o.view(T, hq, d).float().cpu().numpy(), want, dtype, ("mx4 backend extend", hnd, native), ulps=1, absw=absw)
    assert pool.check_errors() == 0
