"""Shared-prefix (cascade) decode over the 4-bit (MXFP4 block-16) pool: rx::cascade_mx4_kernel alone (the skip-extend, not-causal
form of rx_extend_attn_mx4), ops.CascadeDecode / ops.CascadeGroups on packed buffers and the backend route, each against the fp64
oracle fed the exactly dequantised bytes.  Bounds: 1 ulp for a single launch, 2 ulp for the cascade (its partials cross 16-bit
buffers, tests/test_gpu_cascade.py), LSE 1e-4 absolute (an fp32 log-sum of fp32 scores, tests/test_gpu_extend_mx4.py)."""
import numpy as np
import pytest
import torch

import parity_util as parity
from oracle import radix_oracle as orc
from test_gpu_cascade import _oracle_plan, _table
from test_gpu_kv_mx4 import DT, PS, _canon, _dev, _random_pool, mx4_dequant

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731


def _bits(t):
    return t.cpu().view(torch.uint16).numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def _pool(rng, slots, hkv, d, hnd):
    """a random packed pool: (dequantised K, V for the oracle), (k data, v data, k scales, v scales on the device)"""
    p = _random_pool(rng, slots, hkv, d)
    kd, ksd, vd, vsd = (_dev(a, hnd, flat=i % 2 == 1) for i, a in enumerate(p))
    return (mx4_dequant(p[0], p[1]), mx4_dequant(p[2], p[3])), (kd, vd, ksd, vsd)


KV = [0, 1, 63, 64, 65, 200]   # empty chunk; one token; a tile less one; one tile; a tile and one; three full tiles + a partial one
# members per pseudo-request by group size: times G under 16 rows / exactly 128 / 129 (132, 144) / few / few / about 300
EXT = {1: [5, 128, 129, 7, 40, 300], 4: [3, 32, 33, 2, 10, 75], 16: [0, 8, 9, 1, 2, 19]}
# dtype, D, index width, pool ("nhd1": page 1, scattered slots; "hnd": pages of 16, shuffled, not LINEAR with Hkv > 1), (Hq, Hkv), cap + k_scale
P1_CASES = [
    ("bf16", 128, "int", "nhd1", (4, 4), False), ("bf16", 128, "long", "hnd", (8, 2), True), ("bf16", 128, "int", "hnd", (16, 1), False),
    ("bf16", 128, "long", "nhd1", (16, 1), False), ("bf16", 64, "int", "hnd", (8, 2), False), ("bf16", 64, "long", "nhd1", (16, 1), False),
    ("bf16", 64, "long", "hnd", (4, 4), False), ("f16", 128, "int", "hnd", (8, 2), False), ("f16", 128, "long", "nhd1", (4, 4), False),
    ("f16", 128, "long", "hnd", (32, 2), False), ("f16", 64, "long", "hnd", (8, 2), True), ("f16", 64, "int", "nhd1", (4, 1), False),
]


@pytest.mark.parametrize("dt,d,ix,lay,heads,extras", P1_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_phase_one_kernel_matches_the_oracle(dt, d, ix, lay, heads, extras):
    from sglang_amd import lib as rxlib
    from sglang_amd import ops

    (hq, hkv), dtype, hnd = heads, DT[dt], lay == "hnd"
    ext = EXT[hq // hkv]
    rng = np.random.default_rng(d + hq + len(ix + lay))
    n_pages = sum(-(-n // PS) for n in KV) + 3
    if hnd:
        ids = rng.permutation(np.arange(1, n_pages))
        first = np.cumsum([0] + [-(-n // PS) for n in KV])
        slots = np.concatenate([(ids[first[i]: first[i + 1], None] * PS + np.arange(PS)).reshape(-1)[:n] for i, n in enumerate(KV)])
    else:
        slots = rng.permutation(np.arange(1, n_pages * PS))[: sum(KV)]
    (kb, vb), (kd, vd, ksd, vsd) = _pool(rng, n_pages * PS, hkv, d, hnd)
    rows = sum(ext)
    q = torch.from_numpy(rng.standard_normal((rows, hq, d)).astype(np.float32)).to(dtype)
    kx = torch.zeros(rows, hkv, d, dtype=dtype)   # (k_extend / v_extend give the call its kv head count; skip_extend reads neither)
    qo, ip = np.concatenate([[0], np.cumsum(ext)]).astype(np.int64), np.concatenate([[0], np.cumsum(KV)]).astype(np.int32)
    kw = dict(logit_cap=30.0, k_scale=0.9, v_scale=1.25) if extras else {}
    okw = dict(sm_scale=d ** -0.5, is_causal=False, skip_extend=True, **kw)
    want, want_lse = orc.extend_attention(_bits(q), _bits(kx), _bits(kx), kb, vb, qo, ip, slots.astype(np.int64), return_lse=True, **okw)
    _, absw = orc.extend_attention(_bits(q), _bits(kx), _bits(kx), kb, vb, qo, ip, slots.astype(np.int64), return_absw=True, **okw)
    wide = torch.int64 if ix == "long" else torch.int32
    args = (q.to(DEV), kx.to(DEV), kx.to(DEV), None, kd, vd, T(qo).to(wide), T(ip), T(slots).to(wide), None, False, None, max(ext),
            kw.get("k_scale", 1.0), kw.get("v_scale", 1.0))
    linear = "false" if hnd and hkv > 1 else "true"
    for opt, kernel in ((0, "extend_mx4_kernel"), (1, "cascade_mx4_kernel")):
        o = torch.full_like(args[0], float("nan"))
        lse = torch.full(o.shape[:2], float("nan"), dtype=torch.float32, device=DEV)
        with rxlib.option("cascade_mx4", opt):
            ops.extend_attention_fwd(*args[:3], o, *args[4:], sm_scale=d ** -0.5, logit_cap=kw.get("logit_cap", 0.0), skip_extend=True,
                                     lse_extend=lse, page_size=PS if hnd else 1, k_scale_buffer=ksd, v_scale_buffer=vsd)
        torch.cuda.synchronize()
        assert rxlib.last_dispatch() == f"{kernel}<rx::{dt.upper()}, {d}, {ix}, {linear}>|g{hq // hkv}"
    got, got_lse = o.float().cpu().numpy(), lse.cpu().numpy()
    assert not got[: ext[0]].any() and np.all(np.isneginf(got_lse[: ext[0]]))   # the empty chunk: zeros, lse = -inf
    parity.check_out(got, want, dtype, ("cascade_mx4 phase 1", dt, d, ix, lay, heads, extras), ulps=1, absw=absw)
    np.testing.assert_allclose(got_lse, want_lse, atol=1e-4, rtol=0)


CASES = [
    # bs, hq, hkv, d, page, shared(target), lens, min_shared -- the D 128 / 64 shapes of tests/test_gpu_cascade.py::CASES ...
    (8, 8, 2, 128, 16, 512, [600, 513, 700, 640, 1000, 512 + 17, 530, 800], 64),
    (5, 4, 4, 128, 1, 100, [101, 150, 333, 100, 129], 1),          # one request is the prefix itself (empty suffix)
    (3, 16, 2, 64, 16, 256, [300, 257, 512], 64),                  # D 64, logit cap
    (4, 8, 1, 128, 16, 0, [100, 200, 300, 64], 64),                # nothing shared -> plain decode
    (6, 8, 2, 128, 16, 48, [100, 200, 300, 64, 90, 77], 64),       # shared but below min_shared -> L = 0
    (1, 8, 2, 128, 16, 0, [777], 16),                              # bs 1: everything is "shared"
    (40, 8, 2, 128, 16, 600, None, 64),                            # ... and 160 rows per kv head (two row blocks), L ends inside a tile
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_cascade_decode_on_packed_buffers_matches_plain_decode(case):
    from sglang_amd import ops

    bs, hq, hkv, d, page, shared, lens, min_shared = CASES[case]
    dtype, hnd = (torch.bfloat16, torch.float16)[case % 2], page == PS and case % 2 == 0
    rng = np.random.default_rng(700 + case)
    lens = np.asarray(shared + rng.integers(1, 200, size=bs) if lens is None else lens, dtype=np.int64)
    ctx = int(lens.max()) + page
    r2t, slots = _table(rng, shared, lens, page, ctx)
    rpi = np.arange(1, bs + 1, dtype=np.int64)
    (kb, vb), (kd, vd, ksd, vsd) = _pool(rng, slots, hkv, d, hnd)
    q = torch.from_numpy(rng.standard_normal((bs, hq, d)).astype(np.float32)).to(dtype)
    sinks = rng.standard_normal(hq).astype(np.float32) if case % 2 else None
    cap, (ks, vs), sm = 30.0 if case == 2 else 0.0, (0.9, 1.1) if case % 3 == 0 else (1.0, 1.0), d ** -0.5
    ip, ii = orc.build_kv_indices(r2t, rpi, lens)
    want, absw = orc.decode_attention(_bits(q), kb, vb, ip, ii, sm, return_absw=True, k_scale=ks, v_scale=vs, logit_cap=cap, sinks=sinks)
    cd = ops.CascadeDecode(bs, hq, hkv, d, dtype, DEV, max_shared=ctx, min_shared=min_shared, num_chunks=[None, 1, 3][case % 3], mx4=True)
    cd.plan(T(r2t), T(rpi if case % 2 else rpi.astype(np.int32)), T(lens if case % 2 else lens.astype(np.int32)))
    L = _oracle_plan(r2t, rpi, lens, ctx, min_shared)
    assert cd.shared_len() == L and (case in (3, 4) or L >= shared) and (case != 6 or L % 64)
    assert np.array_equal(cd.kv_start[:bs].cpu().numpy(), np.full(bs, L))
    assert np.array_equal(cd.suffix_lens[:bs].cpu().numpy(), lens - L)
    o = torch.full((bs, hq, d), float("nan"), dtype=dtype, device=DEV)
    cd(q.to(DEV), kd, vd, o, sm, ks, vs, cap, None if sinks is None else T(sinks), page_size=page, k_scale_buffer=ksd, v_scale_buffer=vsd)
    parity.check_out(o.float().cpu().numpy(), want, dtype, ("cascade mx4", case), ulps=2, absw=absw)


@pytest.mark.parametrize("hnd", [False, True], ids=["nhd", "hnd"])
def test_cascade_groups_on_packed_buffers(hnd):
    """Two groups of different prefix length and one request in no group."""
    from sglang_amd import ops

    hq, hkv, d, dtype = 8, 2, 128, torch.bfloat16
    rng = np.random.default_rng(31 + hnd)
    shared, members = [300, 130], [[0, 2, 5], [1, 4]]
    lens = np.array([400, 131, 301, 90, 260, 777], dtype=np.int64)
    n_pages = sum(-(-int(n) // PS) for n in lens) + sum(-(-s // PS) for s in shared) + 2
    ids = list(rng.permutation(np.arange(1, n_pages)))
    take = lambda n: np.concatenate([np.arange(PS) + ids.pop() * PS for _ in range(-(-n // PS))])[:n]  # noqa: E731  (n slots on fresh pages)
    r2t = np.zeros((len(lens) + 1, int(lens.max()) + PS), dtype=np.int32)
    pre = [take(s) for s in shared]
    for b, n in enumerate(lens):
        g = next((i for i, m in enumerate(members) if b in m), None)
        head = pre[g] if g is not None else np.zeros(0, np.int64)
        r2t[b + 1, : int(n)] = np.concatenate([head, take(int(n) - len(head))])
    rpi = np.arange(1, len(lens) + 1, dtype=np.int64)
    (kb, vb), (kd, vd, ksd, vsd) = _pool(rng, n_pages * PS, hkv, d, hnd)
    q = torch.from_numpy(rng.standard_normal((len(lens), hq, d)).astype(np.float32)).to(dtype)
    ip, ii = orc.build_kv_indices(r2t, rpi, lens)
    want, absw = orc.decode_attention(_bits(q), kb, vb, ip, ii, d ** -0.5, return_absw=True)
    cg = ops.CascadeGroups(len(lens), hq, hkv, d, dtype, DEV, max_shared_total=1024, mx4=True)
    cg.plan(T(r2t), T(rpi), T(lens), list(zip(members, shared)))
    o = torch.full((len(lens), hq, d), float("nan"), dtype=dtype, device=DEV)
    cg(q.to(DEV), kd, vd, o, d ** -0.5, page_size=PS, k_scale_buffer=ksd, v_scale_buffer=vsd)
    parity.check_out(o.float().cpu().numpy(), want, dtype, ("cascade groups mx4", hnd), ulps=2, absw=absw)


@pytest.mark.parametrize("hnd", [False, True], ids=["nhd", "hnd"])
def test_backend_cascade_decode_on_an_fp4_pool(hnd):
    """A radix-hit batch driven as tests/test_gpu_cascade.py::test_backend_cascade_decode_on_radix_hit_batch drives it: one decode
    step (separate quantising store, then the cascade) against the oracle fed the bytes the pool holds."""
    from sglang_amd import ops
    from sglang_amd.attention.backend import HipRadixAttnBackend
    from sglang_amd.attention.radix_attention import RadixAttention
    from sglang_amd.forward_batch import ForwardBatch
    from sglang_amd.mem_cache.allocator import PagedTokenToKVPoolAllocator
    from sglang_amd.mem_cache.memory_pool import MHATokenToKVPoolFP4, MLATokenToKVPoolFP4, ReqToTokenPool

    hq, hkv, d, dtype, size, bs, shared = 8, 2, 128, torch.bfloat16, 4096, 9, 512
    pool = MHATokenToKVPoolFP4(size, PS, dtype, hkv, d, 1, DEV, use_hnd=hnd)
    r2t = ReqToTokenPool(16, 1200, DEV)
    alloc = PagedTokenToKVPoolAllocator(size, PS, dtype, DEV, pool, debug_mode=True)
    MC = type("MC", (), dict(num_attention_heads=hq, num_key_value_heads=hkv, context_len=1200))
    MR = type("MR", (), dict(device=DEV, req_to_token_pool=r2t, token_to_kv_pool=pool, token_to_kv_pool_allocator=alloc, model_config=MC,
                             page_size=PS, dtype=dtype, server_args=type("SA", (), dict(triton_attention_num_kv_splits=8))))
    backend = HipRadixAttnBackend(MR, cascade_decode=True, cascade_min_bs=2, cascade_min_shared=64)
    layer = RadixAttention(hq, d, d ** -0.5, hkv, 0)
    gen = torch.Generator().manual_seed(11)
    rand = lambda *shape: torch.randn(*shape, generator=gen).to(dtype).to(DEV)  # noqa: E731
    rows = r2t.alloc(bs)
    rpi = torch.tensor(rows, dtype=torch.int64, device=DEV)

    def grow(which, old, new):   # alloc_for_extend: slots + req_to_token rows
        o_, n_ = torch.tensor(old, dtype=torch.int64), torch.tensor(new, dtype=torch.int64)
        last = torch.tensor([int(r2t.req_to_token[r, p - 1]) if p > 0 else -1 for r, p in zip(which, old)], dtype=torch.int64, device=DEV)
        out = alloc.alloc_extend(o_.to(DEV), o_, n_.to(DEV), n_, last, int((n_ - o_).sum()))
        ops.write_req_to_token(r2t.req_to_token, torch.tensor(which, dtype=torch.int64, device=DEV), None, o_.to(DEV), n_.to(DEV),
                               (n_ - o_).to(DEV), out)
        return out

    pool.set_kv_buffer(layer, grow(rows[:1], [0], [shared]), rand(shared, hkv, d), rand(shared, hkv, d))
    for r in rows[1:]:   # radix hit: the cached prefix's slots are written into the new request's row
        r2t.req_to_token[r, :shared] = r2t.req_to_token[rows[0], :shared]
    priv = [1, 40, 129, 16, 300, 77, 5, 250, 64]
    lens = [shared + p for p in priv]
    pool.set_kv_buffer(layer, grow(rows, [shared] * bs, lens), rand(sum(priv), hkv, d), rand(sum(priv), hkv, d))
    seq = [n + 1 for n in lens]
    loc = grow(rows, lens, seq)
    q, k, v = rand(bs, hq * d), rand(bs, hkv * d), rand(bs, hkv * d)
    fb = ForwardBatch.for_decode(rpi, torch.tensor(seq, device=DEV), loc, torch.tensor(seq))
    backend.init_forward_metadata(fb)
    o = layer(q, k, v, fb, backend)
    assert backend._cascade is not None and backend._cascade.shared_len() == shared
    slots = pool.num_pages * PS
    kbo, vbo = (mx4_dequant(_canon(a, hnd, np.empty((slots, hkv, d // 2))), _canon(s, hnd, np.empty((slots, hkv, d // 16))))
                for a, s in zip(pool.get_mx4_buffers(0)[:2], pool.get_mx4_buffers(0)[2:]))
    ip, ii = orc.build_kv_indices(r2t.req_to_token.cpu().numpy(), np.array(rows), np.array(seq))
    want, absw = orc.decode_attention(_bits(q.view(bs, hq, d)), kbo, vbo, ip, ii, d ** -0.5, return_absw=True)
    assert pool.check_errors() == 0
    parity.check_out(o.view(bs, hq, d).float().cpu().numpy(), want, dtype, ("mx4 backend cascade", hnd), ulps=2, absw=absw)
    mla = MLATokenToKVPoolFP4(256, PS, dtype, 512, 64, 1, DEV)
    with pytest.raises(NotImplementedError):
        HipRadixAttnBackend(type("MR2", (MR,), dict(token_to_kv_pool=mla)), cascade_decode=True)
