"""Randomised differential test of the whole 4-bit chain, MHA rows and latent rows: quantising store -> the pool's bytes
(bit for bit against mx4_quant) -> decode attention (against the fp64 oracle on mx4_dequant of the bytes read back) -> row
gather (bit for bit), with the error flags at zero.  tests/test_gpu_random.py draws 16-bit pools only.

Seeds are fixed and no draw is filtered, skipped or retried: where a combination is not served, the draw lists say so.  A CPU
test builds every seed's configuration and runs the oracle alone on it; a failure carries the seed and what it drew."""
import types

import numpy as np
import pytest
import torch

import parity_util as parity
from oracle import radix_oracle as orc
from test_gpu_kv_mx4 import mx4_dequant, mx4_quant
from test_gpu_mx4_edges import DEV, DL, DT, RANK, ROPE, _T, _attend, _expect, _get, _oracle_kw, _put, _table
from test_gpu_random import LEN_POOL

LENS = LEN_POOL + [0, 1100]
GROUPS = [1, 2, 4, 5, 8, 16, 20, 32]
LATENT_HEADS = [1, 2, 4, 5, 8, 16, 20, 32]
PAGES = [1, 4, 16, 32, 48]
SEEDS = [("mha", s) for s in range(12)] + [("mla", s) for s in range(8)]


def _draw(kind, seed):
    rng = np.random.default_rng({"mha": 5000, "mla": 6000}[kind] + seed)

    def pick(xs):
        return xs[int(rng.integers(len(xs)))]

    c = dict(dt=pick(["bf16", "f16"]))
    if kind == "mha":
        c["d"] = pick([64, 128])
        group = pick(GROUPS)
        hkv = pick([h for h in (1, 2, 4, 8) if h * group <= 64])   # (the list follows the group: at most 64 q heads for the fp64 oracle)
        c.update(heads=(hkv * group, hkv), lay=pick(["nhd", "hnd"]))
    else:
        c.update(d=DL, heads=(pick(LATENT_HEADS), 1), lay=pick(["nhd", "pad"]))   # (pad: the padded-page view, never slot-major)
    # One-token pages go with the NHD layout only: every launcher here reads page_size 1 as slot-major rows a token stride
    # apart, which a 4-D [pages, H, 1, X] buffer is not (more than one head, or pad tokens), so those are not drawn.
    c["page"] = pick(PAGES if c["lay"] == "nhd" else PAGES[1:])
    c["lens"] = [pick(LENS) for _ in range(int(rng.integers(1, 9)))]
    c["mode"] = pick(["i32", "i64", "r2t"])
    c["S"] = pick([1, 2, 4, 8, 16])   # (1: single pass)
    c["kw"] = {k: v for k, v in (("k_scale", 0.7), ("v_scale", 1.3), ("logit_cap", 30.0), ("sinks", True), ("xai", 64)) if rng.integers(2)}
    return c, rng


def _chain_inputs(kind, seed):
    """everything a seed needs that the CPU can make: the rows, their slots, the bytes the pool must hold, q, the oracle's answer"""
    c, rng = _draw(kind, seed)
    dtype, d, (hq, hkv), ps = DT[c["dt"]], c["d"], c["heads"], c["page"]
    lens = np.asarray(c["lens"], dtype=np.int64)
    bs = len(lens)
    r2t, n_pages = _table(rng, lens, ps)
    slots = n_pages * ps
    loc = np.concatenate([r2t[i + 1, : int(n)] for i, n in enumerate(lens)]).astype(np.int64)
    loc = loc[rng.permutation(len(loc))]   # the rows arrive in shuffled order
    n = len(loc)
    g = torch.Generator().manual_seed(seed)
    ks, vs = c["kw"].get("k_scale", 1.0), c["kw"].get("v_scale", 1.0)
    rows, pool = [], []
    for sc in (ks,) if d == DL else (ks, vs):   # (latent rows: ONE tensor, stored with the k scale)
        x = torch.randn(n, hkv, d // 16, 16, generator=g) * torch.exp2(torch.randint(-6, 7, (n, hkv, d // 16, 1), generator=g).float())
        x = x.to(dtype).view(n, hkv * d)
        data, sb = np.full((slots, hkv, d // 2), 0x11, np.uint8), np.full((slots, hkv, d // 16), 120, np.uint8)
        xq = (x / sc if sc != 1.0 else x).float().numpy().reshape(n, hkv, d)   # the in-place div_ rounds to the 16-bit dtype
        data[loc], sb[loc] = mx4_quant(xq)
        rows.append(x)
        pool += [data, sb]
    q = torch.randn(bs, hq, d, generator=g).to(dtype)
    ip, ii = orc.build_kv_indices(r2t, np.arange(1, bs + 1, dtype=np.int64), lens)
    okw = _oracle_kw(c, rng)
    kf = mx4_dequant(pool[0], pool[1])
    vf = kf[..., :RANK] if d == DL else mx4_dequant(pool[2], pool[3])
    qb = q.view(torch.uint16).numpy() if dtype == torch.bfloat16 else q.numpy()
    want, absw = orc.decode_attention(qb, kf, vf, ip, ii, d ** -0.5, return_absw=True, **okw)
    return types.SimpleNamespace(c=c, rng=rng, dtype=dtype, lens=lens, r2t=r2t, slots=slots, loc=loc, rows=rows, pool=pool, q=q,
                                 ip=ip, ii=ii, okw=okw, kf=kf, vf=vf, want=want, absw=absw, ks=ks, vs=vs)


@pytest.mark.parametrize("kind,seed", SEEDS)
def test_random_mx4_chain_configurations_on_the_cpu(kind, seed):
    """every seed's configuration can be built, and the oracle alone gives finite values on it"""
    r = _chain_inputs(kind, seed)
    c = r.c
    assert r.lens.sum() > 0 and np.isfinite(r.want).all() and np.isfinite(r.absw).all(), (kind, seed, c)
    assert all(np.isfinite(a).all() for a in (r.kf, r.vf))
    for i, a in enumerate(r.pool):   # the device layout of every buffer, and the instance the case must run
        t = _put(a, c["lay"], c["page"], flat=i % 2 == 1, dev="cpu")
        assert np.array_equal(_get(t, c["lay"], a), a)
    assert _expect(c)[0].startswith("decode_mla_mx4_kernel" if kind == "mla" else "decode_mx4_kernel")


def _run_chain(r, seed):
    from sglang_amd import ops

    c, dtype = r.c, r.dtype
    d, lay, ps, mla = c["d"], c["lay"], c["page"], c["d"] == DL
    # 1. the store, into buffers that hold a recognisable filler
    bufs = [_put(np.full_like(a, 0x11 if i % 2 == 0 else 120), lay, ps, flat=i % 2 == 1) for i, a in enumerate(r.pool)]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    loc = _T(r.loc if seed % 2 else r.loc.astype(np.int32))
    if mla:
        row = r.rows[0].to(DEV)
        if seed % 2:   # the [nope | rope] pair from two tensors
            ops.store_cache_mla_mx4(row[:, :RANK].contiguous(), row[:, RANK:].contiguous(), bufs[0], bufs[1], loc, page_size=ps,
                                    scale=r.ks, err_flag=err)
        else:
            ops.store_cache_mla_mx4(row, None, bufs[0], bufs[1], loc, page_size=ps, scale=r.ks, err_flag=err)
    else:
        ops.store_cache_mx4(r.rows[0].to(DEV), r.rows[1].to(DEV), bufs[0], bufs[2], bufs[1], bufs[3], loc, page_size=ps,
                            k_scale=r.ks, v_scale=r.vs, err_flag=err)
    # 2. the bytes the pool holds
    for i, (buf, w) in enumerate(zip(bufs, r.pool)):
        got = _get(buf, lay, w)
        assert np.array_equal(got, w), ("stored bytes, buffer", i, int((got != w).sum()))
    # 3. decode over them
    four = (bufs[0], bufs[1], bufs[0], None) if mla else tuple(bufs)
    o, name, _ = _attend(c, r.q.to(DEV), four, r.r2t, r.lens, r.ip, r.ii, r.okw)
    assert name == "|".join(_expect(c)), (name, _expect(c))
    got, live = o.float().cpu().numpy(), r.lens > 0
    assert not np.isnan(got[live]).any()
    parity.check_out(got[live], r.want[live], dtype, ("mx4 chain", "mla" if mla else "mha", seed), ulps=1, absw=r.absw[live])
    if c["S"] == 1:
        assert np.all(got[~live] == 0)   # (split-KV leaves an empty request's row to stage 2: test_gpu_mx4_edges holds it)
    # 4. gather a random subset of the slots
    pick = r.rng.integers(0, r.slots, 40)
    if mla:
        nope, rope = ops.get_mla_kv_mx4(bufs[0], bufs[1], _T(pick), RANK, ROPE, dtype, page_size=ps, err_flag=err)
        pairs = [(torch.cat([nope, rope], -1), r.kf)]
    else:
        k, v = ops.gather_kv_mx4(bufs[0], bufs[2], bufs[1], bufs[3], _T(pick), dtype, page_size=ps, err_flag=err)
        pairs = [(k, r.kf), (v, r.vf)]
    for out, f in pairs:
        want = torch.from_numpy(f[pick]).to(dtype)
        assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16)), "gathered rows"
    # 5. nothing was flagged
    assert int(err.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seed", SEEDS)
def test_random_mx4_chain(kind, seed):
    r = _chain_inputs(kind, seed)
    try:
        _run_chain(r, seed)
    except Exception as e:
        raise AssertionError(f"{kind} seed {seed}, drew {r.c}: {e!r}") from e
