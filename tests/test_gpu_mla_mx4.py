"""The 4-bit (MXFP4 block-16) latent pool, MLATokenToKVPoolFP4: the quantising store bit for bit against the format's numpy
restatement (test_gpu_kv_mx4), decode_mla_mx4_kernel and the backend route against the fp64 oracle fed the exactly dequantised
rows (k = the 576-wide row, v = its first 512 columns), the row gather bit for bit."""
import numpy as np
import pytest
import torch

import parity_util as parity
from oracle import radix_oracle as orc
from test_gpu_kv_mx4 import BOUNDS, _step, mx4_dequant, mx4_quant

DEV = "cuda"
PS = 16
RANK, ROPE, D = 512, 64, 576
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


class _Layer:
    layer_id = 0


def _pool(dtype, size):
    from sglang_amd.mem_cache.memory_pool import MLATokenToKVPoolFP4

    return MLATokenToKVPoolFP4(size, PS, dtype, RANK, ROPE, 1, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True], ids=["row", "nope_rope"])
@pytest.mark.parametrize("dt", DT)
def test_store_is_bit_exact(dt, pair):
    dtype, n = DT[dt], 70
    pool = _pool(dtype, 5 * PS)
    slots = pool.kv_buffer[0].shape[0]
    g = torch.Generator().manual_seed(len(dt) + pair)
    x = torch.randn(n, D // 16, 16, generator=g) * torch.exp2(torch.randint(-6, 7, (n, D // 16, 1), generator=g).float())
    x = x.to(dtype)
    for b0, kk in ((0, -3), (33, 4)):   # a block of the nope part and one of the rope part
        ties = torch.tensor(BOUNDS) * 2.0 ** kk
        x[0, b0] = torch.cat([ties, -ties, torch.tensor([6 * 2.0 ** kk, 0.0])]).to(dtype)   # every tie, both signs
        x[1, b0 + 1] = 0                                                                     # an all-zero block
        top = torch.tensor([6 * 2.0 ** kk]).to(dtype)
        for blk, val in enumerate((top, _step(top, True), _step(top, False))):               # maxima at 6 * 2^k and a step off
            x[2, b0 + blk] = (x[2, b0 + blk].float().clamp(-2.0 ** kk, 2.0 ** kk)).to(dtype)
            x[2, b0 + blk, 5] = -val[0] if blk == 1 else val[0]
    x = x.view(n, 1, D)
    loc = torch.cat([torch.randperm(slots - 1, generator=g)[: n - 2] + 1, torch.tensor([0, slots + 5])])  # + reserved, + outside
    data, sb = np.full((slots, 1, D // 2), 0xAB, np.uint8), np.full((slots, D // 16), 0xAB, np.uint8)
    qd, qs = mx4_quant(x.float().numpy())
    data[loc[:-2].numpy()], sb[loc[:-2].numpy()] = qd[:-2], qs[:-2, 0]
    pool.kv_buffer[0].fill_(0xAB)
    pool.kv_scale_buffer[0].fill_(0xAB)
    xd = x.to(DEV)
    if pair:
        pool.set_mla_kv_buffer(_Layer, loc.to(DEV), xd[..., :RANK].contiguous(), xd[..., RANK:].contiguous())
    else:
        pool.set_kv_buffer(_Layer, loc.to(DEV), xd)
    assert pool.check_errors() == 1
    got_d, got_s = (t.cpu().numpy() for t in pool.get_mx4_buffers(0))
    assert np.array_equal(got_d, data), int((got_d != data).sum())
    assert np.array_equal(got_s, sb), int((got_s != sb).sum())
    assert sb[loc[1], 1] == 94 and sb[loc[1], 34] == 94


# dtype, lookup, linear layout, Hq, kv splits, extras (logit cap + sinks + scales), K scale bytes rising with position
DECODE_CASES = [
    ("bf16", "i64", True, 16, True, False, False), ("bf16", "i64", False, 5, False, False, False),
    ("bf16", "i32", True, 32, False, False, False), ("bf16", "i32", False, 16, True, False, False),
    ("bf16", "r2t", True, 5, True, False, False), ("bf16", "r2t", False, 32, False, False, False),
    ("f16", "i64", True, 5, False, False, False), ("f16", "i64", False, 32, True, False, False),
    ("f16", "i32", True, 16, True, False, False), ("f16", "i32", False, 5, False, False, False),
    ("f16", "r2t", True, 32, True, False, False), ("f16", "r2t", False, 16, False, False, False),
    ("bf16", "i64", True, 16, True, True, False), ("f16", "r2t", False, 5, False, True, False),
    ("bf16", "i32", True, 16, False, False, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,mode,lin,hq,split,extras,rising", DECODE_CASES, ids=lambda v: str(v))
def test_decode_matches_the_oracle(dt, mode, lin, hq, split, extras, rising):
    from sglang_amd import lib as rxlib
    from sglang_amd import ops

    dtype = DT[dt]
    lens = np.array([1, 31, 32, 33, 65, 257, 1100], dtype=np.int64)
    bs = len(lens)
    rng = np.random.default_rng(hq + len(dt + mode) + lin)
    pages = [-(-int(n) // PS) for n in lens]
    n_pages = sum(pages) + 3
    page_ids = rng.permutation(np.arange(1, n_pages))   # shuffled, page 0 unused
    r2t = np.zeros((bs + 1, int(lens.max()) + PS), dtype=np.int32)
    pi = 0
    for i, n in enumerate(lens):
        r2t[i + 1, : int(n)] = (page_ids[pi: pi + pages[i], None] * PS + np.arange(PS)[None]).reshape(-1)[: int(n)]
        pi += pages[i]
    # the pool straight from random nibbles and scale bytes 119..127 (every value exact in fp16 too): independent of the store
    data = rng.integers(0, 256, (n_pages * PS, 1, D // 2), dtype=np.uint8)
    sb = rng.integers(119, 128, (n_pages * PS, 1, D // 16)).astype(np.uint8)
    if rising:   # later scores beat earlier ones by far more than ln 4096: the max-based softmax step runs again and again
        for i, n in enumerate(lens):
            sb[r2t[i + 1, : int(n)]] = (119 + np.arange(int(n)) * 12 // int(n)).astype(np.uint8)[:, None, None]
    q = torch.from_numpy(rng.standard_normal((bs, hq, D)).astype(np.float32)).to(dtype)
    rpi = np.arange(1, bs + 1, dtype=np.int64)
    ip, ii = orc.build_kv_indices(r2t, rpi, lens)
    sm = D ** -0.5
    kw = dict(k_scale=0.8, v_scale=1.25, logit_cap=30.0, sinks=rng.standard_normal(hq).astype(np.float32)) if extras else {}
    qb = q.view(torch.uint16).numpy() if dtype == torch.bfloat16 else q.numpy()
    k = mx4_dequant(data, sb)
    want, absw = orc.decode_attention(qb, k, k[..., :RANK], ip, ii, sm, return_absw=True, **kw)
    if lin:   # the pool's own shapes: [slots, 1, 288] / [slots, 36]
        kd, ksd = torch.from_numpy(data).to(DEV), torch.from_numpy(sb[:, 0]).to(DEV)
    else:     # pages with two pad tokens: [pages, 1, page, 288] / [pages, 1, page, 36] views
        kd, ksd = (torch.zeros(n_pages, 1, PS + 2, a.shape[-1], dtype=torch.uint8) for a in (data, sb))
        kd[:, :, :PS], ksd[:, :, :PS] = (torch.from_numpy(a).view(n_pages, PS, 1, -1).permute(0, 2, 1, 3) for a in (data, sb))
        kd, ksd = kd.to(DEV)[:, :, :PS], ksd.to(DEV)[:, :, :PS]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    S = 8 if split else 1
    lens_d = T(lens)
    splits = al = ls = None
    if split:
        splits = torch.zeros(bs, dtype=torch.int32, device=DEV)
        ops.get_num_kv_splits_balanced(splits, lens_d, hq, 1, S, 64, 128)   # (a small budget: the long request is cut)
        assert int(splits.max()) > 1
        al = torch.zeros(bs, hq, S, RANK, dtype=torch.float32, device=DEV)
        ls = torch.zeros(bs, hq, S, dtype=torch.float32, device=DEV)
    o = torch.full((bs, hq, RANK), float("nan"), dtype=dtype, device=DEV)
    common = dict(page_size=PS, k_scale_buffer=ksd, v_scale_buffer=ksd if hq == 16 else None)
    if extras:
        common.update(logit_cap=kw["logit_cap"], sinks=T(kw["sinks"]))
    ksc, vsc = kw.get("k_scale", 1.0), kw.get("v_scale", 1.0)
    if mode == "r2t":
        ops.decode_attention_fwd_paged(q.to(DEV), kd, kd, o, T(r2t), T(rpi), lens_d, al, ls, splits, S, sm, ksc, vsc, **common)
    else:
        ops.decode_attention_fwd(q.to(DEV), kd, kd, o, T(ip), T(ii).to(torch.int64 if mode == "i64" else torch.int32), al, ls,
                                 splits, S, sm, ksc, vsc, **common)
    torch.cuda.synchronize()
    assert rxlib.last_dispatch() == (f"decode_mla_mx4_kernel<rx::{dt.upper()}, {'long' if mode == 'i64' else 'int'}, "
                                     f"{'true' if lin else 'false'}>|" + ("req_to_token" if mode == "r2t" else "indices"))
    # the unpack is exact, so the result carries the 16-bit latent kernel's roundings: the same bound as its cases
    parity.check_out(o.float().cpu().numpy(), want, dtype, ("mla mx4", dt, mode, lin, hq, split, extras, rising), ulps=1, absw=absw)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
def test_gather_is_bit_exact(dt):
    dtype = DT[dt]
    pool = _pool(dtype, 5 * PS)
    slots = pool.kv_buffer[0].shape[0]
    rng = np.random.default_rng(len(dt))
    data = rng.integers(0, 256, (slots, 1, D // 2), dtype=np.uint8)
    sb = rng.integers(119, 128, (slots, D // 16)).astype(np.uint8)
    pool.kv_buffer[0].copy_(torch.from_numpy(data))
    pool.kv_scale_buffer[0].copy_(torch.from_numpy(sb))
    loc = rng.integers(0, slots, 50)
    nope, rope = pool.get_mla_kv_buffer(_Layer, torch.from_numpy(loc).to(DEV))
    want = torch.from_numpy(mx4_dequant(data, sb[:, None])[loc]).to(dtype)
    assert tuple(nope.shape) == (50, 1, RANK) and tuple(rope.shape) == (50, 1, ROPE) and pool.check_errors() == 0
    assert torch.equal(torch.cat([nope, rope], -1).cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
def test_backend_extend_then_decode_on_the_latent_fp4_pool():
    """HipRadixAttnBackend on MLATokenToKVPoolFP4: extend over 4-bit prefixes (store, gather, extend_mla_kernel), then one
    decode step (decode_mla_mx4_kernel), both against the oracle fed the dequantised bytes the pool actually holds."""
    from sglang_amd import ops
    from sglang_amd.attention.backend import HipRadixAttnBackend
    from sglang_amd.attention.radix_attention import RadixAttention
    from sglang_amd.forward_batch import ForwardBatch
    from sglang_amd.mem_cache.allocator import PagedTokenToKVPoolAllocator
    from sglang_amd.mem_cache.memory_pool import ReqToTokenPool

    hq, dtype, size = 16, torch.bfloat16, 1024
    pool = _pool(dtype, size)
    r2t = ReqToTokenPool(8, 512, DEV)
    alloc = PagedTokenToKVPoolAllocator(size, PS, dtype, DEV, pool, debug_mode=True)

    class MC:
        num_attention_heads, num_key_value_heads, context_len = hq, 1, 512

    class MR:
        device, req_to_token_pool, token_to_kv_pool, token_to_kv_pool_allocator, model_config, page_size = DEV, r2t, pool, alloc, MC, PS
        dtype = torch.bfloat16

        class server_args:
            triton_attention_num_kv_splits = 8

    backend = HipRadixAttnBackend(MR)
    layer = RadixAttention(hq, D, D ** -0.5, 1, 0, v_head_dim=RANK)
    g = torch.Generator().manual_seed(5)
    rand = lambda *shape: torch.randn(*shape, generator=g).to(dtype).to(DEV)  # noqa: E731
    with pytest.raises(NotImplementedError, match="get_mx4_buffers"):
        pool.get_key_buffer(0)
    pre, ext = [0, 70, 33], [40, 9, 20]
    rows = r2t.alloc(3)
    rpi = torch.tensor(rows, dtype=torch.int64, device=DEV)

    def grow(old, new):   # alloc_for_extend: slots + req_to_token rows
        o_, n_ = torch.tensor(old, dtype=torch.int64), torch.tensor(new, dtype=torch.int64)
        last = torch.tensor([int(r2t.req_to_token[r, p - 1]) if p > 0 else -1 for r, p in zip(rows, old)], dtype=torch.int64, device=DEV)
        out = alloc.alloc_extend(o_.to(DEV), o_, n_.to(DEV), n_, last, int((n_ - o_).sum()))
        ops.write_req_to_token(r2t.req_to_token, rpi, None, o_.to(DEV), n_.to(DEV), (n_ - o_).to(DEV), out)
        return out

    def held():   # the pool's rows as the oracle's float buffer [slots, 1, 576]
        kb, ksb = pool.get_mx4_buffers(0)
        return mx4_dequant(kb.cpu().numpy(), ksb.cpu().numpy()[:, None])

    pool.set_kv_buffer(layer, grow([0, 0, 0], pre), rand(sum(pre), 1, D))
    seq = [p + e for p, e in zip(pre, ext)]
    loc = grow(pre, seq)
    T = sum(ext)
    q, k = rand(T, hq * D), rand(T, 1, D)
    kbo = held()   # (before the forward stores the new rows: the extend reads the prefix only)
    fb = ForwardBatch.for_extend(rpi, torch.tensor(seq, device=DEV), loc, pre, ext)
    backend.init_forward_metadata(fb)
    o = layer(q, k, k[..., :RANK], fb, backend)
    bits = lambda t, *shape: t.reshape(*shape).cpu().view(torch.uint16).numpy()  # noqa: E731
    ip, ii = orc.build_kv_indices(r2t.req_to_token.cpu().numpy(), np.array(rows), np.array(pre))
    qo = np.concatenate([[0], np.cumsum(ext)]).astype(np.int64)
    want, absw = orc.extend_attention(bits(q, T, hq, D), bits(k, T, 1, D), bits(k[..., :RANK].contiguous(), T, 1, RANK), kbo,
                                      kbo[..., :RANK], qo, ip, ii, is_causal=True, sm_scale=D ** -0.5, return_absw=True)
    parity.check_out(o.view(T, hq, RANK).float().cpu().numpy(), want, dtype, ("mla mx4 backend extend",), ulps=1, absw=absw)

    seq1 = [s + 1 for s in seq]
    loc = grow(seq, seq1)
    q, k = rand(3, hq * D), rand(3, 1, D)
    seq_t = torch.tensor(seq1, dtype=torch.int64)
    fb = ForwardBatch.for_decode(rpi, seq_t.to(DEV), loc, seq_t)
    backend.init_forward_metadata(fb)
    o = layer(q, k, k[..., :RANK], fb, backend)
    kbo = held()
    ip, ii = orc.build_kv_indices(r2t.req_to_token.cpu().numpy(), np.array(rows), np.array(seq1))
    want, absw = orc.decode_attention(bits(q, 3, hq, D), kbo, kbo[..., :RANK], ip, ii, D ** -0.5, return_absw=True)
    assert pool.check_errors() == 0
    parity.check_out(o.view(3, hq, RANK).float().cpu().numpy(), want, dtype, ("mla mx4 backend decode",), ulps=1, absw=absw)


def test_rejected_arguments_raise_and_null_params_fail_on_the_host():
    from sglang_amd import lib as rxlib
    from sglang_amd import ops
    from sglang_amd.mem_cache.memory_pool import MLATokenToKVPool

    assert rxlib.load().rx_decode_attn_mx4(None, None, None) == -1 and b"null" in rxlib.load().rx_last_error()
    q, o = torch.zeros(2, 16, D, dtype=torch.bfloat16), torch.zeros(2, 16, RANK, dtype=torch.bfloat16)
    kb, sb, x = torch.zeros(32, 1, D // 2, dtype=torch.uint8), torch.zeros(32, D // 16, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    fwd = (q, kb, kb, o, x, x, None, None, None, 1, 0.1, 1.0, 1.0)
    for name, val in (("score_mod", ops.relative_bias_score_mod), ("stages", 1), ("merge_counters", x), ("k_new", q),
                      ("split_items", object())):
        with pytest.raises(NotImplementedError, match=name):
            ops.decode_attention_fwd(*fwd, k_scale_buffer=sb, **{name: val})
    paged = (q, kb, kb, o, x, x, x, None, None, None, 1, 0.1)
    for name, val in (("kv_start", x), ("extra_o", q), ("extra_lse", q), ("stages", 2), ("merge_counters", x), ("k_new", q),
                      ("split_items", object()), ("score_mod", ops.relative_bias_score_mod), ("units", object())):
        with pytest.raises(NotImplementedError, match=name):
            ops.decode_attention_fwd_paged(*paged, k_scale_buffer=sb, **{name: val})
    with pytest.raises(NotImplementedError, match="MLATokenToKVPoolFP4"):   # fused RoPE decode
        ops.decode_attention_fwd_grouped_rope(q, kb, kb, o, x, x, None, RANK, ROPE, None, None, None, 1, 0.1)
    with pytest.raises(NotImplementedError, match="uint8"):
        MLATokenToKVPool(64, 1, torch.uint8, RANK, ROPE, 1, "cpu")
