"""Pool-addressing kernels on KV pools larger than 4 GiB: is the slot -> offset arithmetic 64-bit from end to end?

Every pool here is a typed view of ONE uint8 storage of big_pool_util.NBYTES (8 GiB + 128 MiB, never initialised as a
whole), K and V views one window apart, and a case touches only slots of the pool's high window: offsets >= 2^32
elements from the view's base, chosen (big_pool_util, held to brute force by test_big_pool_util.py) so that any 32-bit
truncation lands on sentinel bytes INSIDE the storage.  A wrong kernel fails a comparison; it cannot leave the buffer.

Three checks per case.  (1) oracle: the window's rows are gathered into a compact pool, the slot ids remapped (slot -
window base), and the output held to oracle/radix_oracle.py through parity_util.check_out at the bound of that
kernel's dispatch-coverage case (ulps = 1, absw); stores and gathers are bit-exact copies / conversions and are held
to torch's own.  (2) twin: the same call on the compact pool -- same options, same explicit num_kv_splits; only
addresses differ -- must give the same BITS; the twin runs twice first, so a family that is not bit-stable run to run
fails there and not in the comparison (none was: every family below is held to all three checks).  (3) canaries
(writing kernels): the alias ranges are filled with 0xFF before the call and must be unchanged after it, and the
window's rows equal the twin's.  For reading kernels the same 0xFF bytes are NaNs (bf16 / e4m3fn): a truncated read
poisons the output.

4-bit (MXFP4) pools: the DATA bytes are a view with a high window like any other; the scale bytes sit 8x lower (near
2^29: no truncation moves them) in a second view at big_pool_util.SCALE_BASES, with guard rows around their window.
The cascade decode is held to ulps = 2, the bound of test_gpu_cascade.py (its chunk partials cross 16-bit buffers).
extend_mfma64_kernel exists in development builds only (option ext64 has no effect in the product library), so no
call can reach it.

Measured on an MI355X: the allocation takes 0.5 ms (torch.empty only reserves the range; the cases touch a few MiB of
it), the module's 96 cases 4 to 5 s in all, the slowest one 0.4 s."""
import time
import zlib

import numpy as np
import pytest
import torch

import big_pool_util as bp
import parity_util as parity
from oracle import radix_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn
PS = 16   # slots are handed out in pages of 16 in every case, as the dispatch-coverage matrix does


@pytest.fixture(scope="module")
def ops():
    from sglang_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def rxlib():
    from sglang_amd import lib

    return lib


@pytest.fixture(scope="module")
def storage():
    free, _ = torch.cuda.mem_get_info()
    need = bp.NBYTES + (1 << 30)   # the storage, and a GiB for the twins and torch's own pools
    if free < need:
        pytest.skip(f"big-pool tests need {need} bytes of free device memory, mem_get_info() shows {free}")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = torch.empty(bp.NBYTES, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    print(f"\nbig pool: {bp.NBYTES} bytes allocated in {(time.perf_counter() - t0) * 1e3:.1f} ms")
    yield s
    del s
    torch.cuda.empty_cache()


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == BF16:
        return t.view(torch.uint16).numpy()
    return t.view(torch.uint8).numpy() if t.dtype == FP8 else t.numpy()


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Pools:
    """K and V views of one geometry with their window, twins and canaries.  mla: V is K's first 512 columns."""

    def __init__(self, storage, name, dtype, mid=False, mla=False):
        h, d, es, page, layout = bp.GEOMETRIES[name]
        self.storage, self.name, self.dtype, self.mla, self.hnd, self.h, self.d = storage, name, dtype, mla, layout == "hnd", h, d
        self.win = bp.mid_window(h * d, es, page, layout) if mid else bp.geometry_window(name)
        base = bp.MID_BASE if mid else 0
        self.bases = (base,) if mla else (base, base + bp.V_OFFSET)
        self.k = bp.pool_view(storage, self.bases[0], dtype, name, self.win)
        self.v = self.k[..., :512] if mla else bp.pool_view(storage, self.bases[1], dtype, name, self.win)
        self.n = self.win.hi - self.win.lo
        self.page = page

    def layout(self, ops, k=None, v=None):
        """(page_size, kv_layout) arguments of the attention calls for the big pool or a twin"""
        return (self.page, ops.kv_layout_hnd(self.k if k is None else k, self.v if v is None else v)) if self.hnd else (1, None)

    def windows(self):
        return [bp.window_rows(p, self.win) for p in ((self.k,) if self.mla else (self.k, self.v))]

    def fill(self, seed):
        """sentinels into the alias ranges, random rows into the windows"""
        g = torch.Generator().manual_seed(seed)
        for base, rows in zip(self.bases, self.windows()):
            bp.fill_alias(self.storage, base, self.win)
            if self.dtype == torch.uint8:
                rows.copy_(torch.randint(0, 256, rows.shape, generator=g, dtype=torch.uint8).to(DEV))
            else:
                rows.copy_(torch.randn(rows.shape, generator=g).to(self.dtype).to(DEV))

    def poison(self, byte=0x5A):
        """sentinels into the alias ranges, one other byte into the windows (stores)"""
        for base, rows in zip(self.bases, self.windows()):
            bp.fill_alias(self.storage, base, self.win)
            rows.view(torch.uint8).fill_(byte)

    def twins(self):
        k = self.windows()[0].clone()
        return (k, k[..., :512]) if self.mla else (k, self.windows()[1].clone())

    def intact(self):
        return all(bp.alias_intact(self.storage, b, self.win) for b in self.bases)

    def canon(self, t):
        """a twin (or window) -> [slots, H, D] on the CPU, slot 0 = the window's first slot"""
        t = t.cpu()
        if t.dtype == FP8:   # (bytes: torch indexes uint8 everywhere)
            t = t.view(torch.uint8)
        return t.permute(0, 2, 1, 3).reshape(self.n, self.h, t.shape[-1]) if self.hnd else t

    def oracle_rows(self, t):
        c = self.canon(t)
        return orc.fp8_e4m3fn_decode(c.contiguous().numpy()) if self.dtype == FP8 else _bits(c)


def _set_rows(pools, rows, rel, value):
    """rows (a window or a twin) at the relative slots `rel` := value"""
    if pools.hnd:
        rows[rel // PS, :, rel % PS] = value
    else:
        rows[rel] = value


def _dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dt is None else t.to(dt)


def _loc(pools, n, seed, dtype):
    """n distinct window slots, relative to the window, its second and last among them (not its first: relative slot 0
    is the twin's reserved slot, which the stores skip)"""
    g = torch.Generator().manual_seed(seed)
    rel = torch.randperm(pools.n - 3, generator=g)[: n - 2] + 2
    return torch.cat([rel, torch.tensor([1, pools.n - 1])]).to(dtype)


def _paged_lists(lens, n_slots, seed):
    """req_to_token rows (relative slots, shuffled pages of 16) for requests of `lens` tokens"""
    rng = np.random.default_rng(seed)
    pages = [-(-int(n) // PS) for n in lens]
    assert sum(pages) <= n_slots // PS
    ids = rng.permutation(n_slots // PS)
    r2t = np.zeros((len(lens) + 1, int(max(lens)) + PS), dtype=np.int64)
    pi = 0
    for i, n in enumerate(lens):
        r2t[i + 1, : int(n)] = (ids[pi: pi + pages[i], None] * PS + np.arange(PS)[None]).reshape(-1)[: int(n)]
        pi += pages[i]
    return r2t


# ======================================================================================================================
# stores
# ======================================================================================================================
STORES = [("store_cache", "bf16_h8_d128", BF16, False), ("store_cache", "bf16_h8_d128", BF16, True),   # (True: offsets in [2^31, 2^32))
          ("store_cache_layout", "bf16_h8_d128_hnd", BF16, False), ("store_cache_layout", "bf16_h2_d64_hnd", BF16, False),
          ("store_cache_fp8", "fp8_h2_d128", FP8, False), ("store_cache_fp8", "fp8_h2_d128_hnd", FP8, False),
          ("fused_fp8_qkv_kv_cache", "fp8_h2_d128", FP8, False), ("fused_fp8_qkv_kv_cache", "fp8_h2_d128_hnd", FP8, False)]


def _store(ops, op, P, k, v, kb, vb, loc, slots):
    """one store of rows k / v at `loc` into the pools kb / vb (the big views or the twins)"""
    h, d = P.h, P.d
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    if op == "store_cache":
        ops.store_cache(k, v, kb, vb, loc, err_flag=err)
    else:
        lay = ops.kv_layout_hnd(kb, vb) if P.hnd else ops._kv_layout(kb, vb, 1)
        if op == "store_cache_layout":
            ops.store_cache_layout(k, v, lay, loc, h, d, d, size_limit=slots, err_flag=err)
        elif op == "store_cache_fp8":
            ops.store_cache_fp8(k, v, lay, loc, h, d, d, size_limit=slots, k_scale=0.5, v_scale=2.0, err_flag=err)
        else:
            sc = torch.tensor([0.5], device=DEV), torch.tensor([2.0], device=DEV)
            ops.fused_fp8_qkv_kv_cache(None, k.view(-1, h, d), v.view(-1, h, d), kb, vb, loc, *sc, kv_layout=lay if P.hnd else None, err_flag=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 0


@pytest.mark.parametrize("op,name,dtype,mid", STORES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_store_reaches_the_high_window(storage, ops, op, name, dtype, mid, idt):
    P = Pools(storage, name, dtype, mid=mid)
    n = 70
    g = torch.Generator().manual_seed(zlib.crc32((op + name).encode()))
    k = torch.randn(n, P.h * P.d, generator=g).to(BF16).to(DEV)
    v = torch.randn(n, P.h * P.d, generator=g).to(BF16).to(DEV)
    rel = _loc(P, n, 5, idt).to(DEV)
    P.poison()
    kt, vt = P.twins()
    _store(ops, op, P, k, v, kt, vt, rel, P.n)
    kt2, vt2 = P.twins()
    _store(ops, op, P, k, v, kt2, vt2, rel, P.n)
    assert _same(kt, kt2) and _same(vt, vt2)
    _store(ops, op, P, k, v, P.k, P.v, rel + P.win.lo, P.win.hi)
    assert P.intact(), "a store went to an alias of its slot (a truncated offset)"
    kw, vw = P.windows()
    assert _same(kw, kt) and _same(vw, vt)                     # the window holds what the twin holds ...
    for rows, src, scale in ((P.canon(kt), k, 0.5), (P.canon(vt), v, 2.0)):   # ... and that is the stored rows
        want = src.view(n, P.h, P.d).cpu()
        if dtype == FP8:   # (scales are powers of two: the in-place div_ of one op and the fp32 multiply of the other agree)
            want = (want.float() / scale).to(FP8).view(torch.uint8)
        assert _same(rows[rel.cpu().long()], want), op
        untouched = torch.ones(P.n, dtype=torch.bool)
        untouched[rel.cpu().long()] = False
        assert bool((rows[untouched].contiguous().view(torch.uint8) == 0x5A).all())


# ======================================================================================================================
# gathers and moves
# ======================================================================================================================
@pytest.mark.parametrize("name,dtype", [("bf16_mla", BF16), ("fp8_mla", FP8)], ids=["bf16", "fp8"])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_get_mla_kv_reads_the_high_window(storage, ops, name, dtype, idt):
    P = Pools(storage, name, dtype, mla=True)
    P.fill(7)
    kt, _ = P.twins()
    rel = _loc(P, 50, 9, idt).to(DEV)
    a = ops.get_mla_kv(kt, rel, 512, 64, BF16, size_limit=P.n)
    b = ops.get_mla_kv(kt, rel, 512, 64, BF16, size_limit=P.n)
    c = ops.get_mla_kv(P.k, rel + P.win.lo, 512, 64, BF16, size_limit=P.win.hi)
    torch.cuda.synchronize()
    want = kt[rel.long()] if dtype == BF16 else kt.view(torch.uint8)[rel.long()].view(FP8).float().to(BF16)
    for x, y, z, w in zip(a, b, c, (want[..., :512], want[..., 512:])):
        assert _same(x, y) and _same(z, x) and _same(x, w)


@pytest.mark.parametrize("direction", ["high_to_high", "high_to_low", "low_to_high"])
def test_move_kv_between_low_and_high_slots(storage, ops, direction):
    """rx_move_kv on both buffers of a linear pool.  The low slots are taken ABOVE the alias slots, so that a move that
    truncates lands on a canary and not on its own source or target."""
    P = Pools(storage, "bf16_h8_d128", BF16)
    P.fill(11)
    low0 = max(P.win.alias_slots) + 1
    low = [p[low0: low0 + P.n] for p in (P.k, P.v)]
    g = torch.Generator().manual_seed(13)
    for rows in low:
        rows.copy_(torch.randn(rows.shape, generator=g).to(BF16).to(DEV))
    n = 40
    perm = torch.randperm(P.n, generator=g)
    src_rel, tgt_rel = perm[:n].to(DEV), perm[n: 2 * n].to(DEV)
    src_hi, tgt_hi = direction != "low_to_high", direction != "high_to_low"
    # the twin: the compact copies of [low rows | window rows] of each buffer
    twins = [torch.cat([lo_, hi_]) for lo_, hi_ in zip(low, P.windows())]
    ts, tt = src_rel + (P.n if src_hi else 0), tgt_rel + (P.n if tgt_hi else 0)
    want = [t.clone() for t in twins]
    for w in want:
        w[tt] = w[ts]
    rb = torch.tensor([P.win.row_bytes] * 2, dtype=torch.int64, device=DEV)
    for rep in range(2):
        tw = [t.clone() for t in twins]
        ops.move_kv(torch.tensor([t.data_ptr() for t in tw], dtype=torch.int64, device=DEV), rb, tt, ts)
        torch.cuda.synchronize()
        assert all(_same(a, b) for a, b in zip(tw, want))
    ops.move_kv(torch.tensor([P.k.data_ptr(), P.v.data_ptr()], dtype=torch.int64, device=DEV), rb,
                tgt_rel + (P.win.lo if tgt_hi else low0), src_rel + (P.win.lo if src_hi else low0))
    torch.cuda.synchronize()
    assert P.intact(), "a move read or wrote an alias of its slot"
    for lo_, hi_, w in zip(low, P.windows(), want):
        assert _same(torch.cat([lo_, hi_]), w)


# ======================================================================================================================
# decode
# ======================================================================================================================
# family, geometry, pool dtype, Hq, lookup, kv splits, extras
DECODES = [
    ("decode_mfma_kernel", "bf16_h8_d128", BF16, 32, "i64", True, {}),
    ("decode_mfma_kernel", "bf16_h8_d128_hnd", BF16, 32, "r2t", True, {}),
    ("decode_mfma_kernel", "bf16_h2_d64_hnd", BF16, 8, "i32", False, {}),
    ("decode_mfma_kernel", "bf16_h2_d128", BF16, 8, "units", False, {}),
    ("decode_mfma_kernel", "bf16_h2_d128", BF16, 8, "r2t", False, {"fuse": True}),
    ("decode_mfma_kernel", "bf16_h2_d128_hnd", BF16, 4, "i64", False, {"fuse": True}),
    ("decode_mfma_kernel", "fp8_h2_d128", FP8, 8, "i32", True, {}),
    ("decode_mfma_kernel", "fp8_h2_d128_hnd", FP8, 8, "r2t", False, {}),
    ("decode_mfma_kernel", "bf16_h8_d128", BF16, 32, "i64", True, {"mid": True}),
    ("decode_mfma_bias_kernel", "bf16_h2_d128", BF16, 8, "i64", True, {"bias": True}),
    ("decode_mfma_bias_kernel", "bf16_h2_d64_hnd", BF16, 4, "r2t", False, {"bias": True}),
    ("decode_generic_kernel", "bf16_h2_d80", BF16, 4, "i64", True, {}),
    ("decode_generic_kernel", "bf16_h2_d80", BF16, 8, "i32", False, {}),
    ("decode_mla_kernel", "bf16_mla", BF16, 16, "i64", True, {}),
    ("decode_mla_kernel", "bf16_mla", BF16, 5, "r2t", False, {}),
    ("decode_mla_kernel", "fp8_mla", FP8, 16, "i64", True, {"opts": {"decode_mla8_dma": 0}}),
    ("decode_mla8_dma_kernel", "fp8_mla", FP8, 16, "i64", True, {}),
    ("decode_mla8_dma_kernel", "fp8_mla", FP8, 128, "r2t", False, {}),
    ("decode_mla8_t64_kernel", "fp8_mla", FP8, 16, "i32", True, {"opts": {"decode_mla8_t64": 1}}),
]


@pytest.mark.parametrize("fam,name,pdt,hq,mode,split,extra", DECODES, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_decode_reads_the_high_window(storage, ops, rxlib, fam, name, pdt, hq, mode, split, extra):
    mla = name.endswith("mla")
    P = Pools(storage, name, pdt, mid=extra.get("mid", False), mla=mla)
    dk, dv, hkv = P.d, (512 if mla else P.d), P.h
    lens = np.array([1, 33, 257, 300], dtype=np.int64)
    bs = len(lens)
    seed = zlib.crc32(repr((fam, name, hq, mode, split)).encode())
    P.fill(seed)
    g = torch.Generator().manual_seed(seed)
    r2t = _paged_lists(lens, P.n, seed)
    rpi = np.arange(1, bs + 1, dtype=np.int64)
    ip, ii = orc.build_kv_indices(r2t, rpi, lens)
    q = torch.randn(bs, hq, dk, generator=g).to(BF16)
    sm = dk ** -0.5
    ks, vs = (0.8, 1.25) if (pdt == FP8 and not mla) else (1.0, 1.0)
    kn = vn = last = None
    if extra.get("fuse"):   # the launch stores the step's new row itself: the row is poisoned first, in the pool and in the twin
        kn, vn = (torch.randn(bs, hkv, dk, generator=g).to(BF16).to(DEV) for _ in range(2))
        last = torch.from_numpy(r2t[rpi, lens - 1])
        for rows in P.windows():
            _set_rows(P, rows, last.to(DEV), 7.0)
    aux = (1.5 * torch.randn(bs, hq, 70, generator=g)).to(DEV) if extra.get("bias") else None
    S = 8 if split else 1
    splits = torch.tensor([1, 2, 2, 3], dtype=torch.int32, device=DEV) if split else None
    qd = q.to(DEV)
    T = _dev

    def run(kb, vb, base):
        o = torch.full((bs, hq, dv), float("nan"), dtype=BF16, device=DEV)
        al = torch.zeros(bs, hq, S, dv, dtype=torch.float32, device=DEV) if split else None
        ls = torch.zeros(bs, hq, S, dtype=torch.float32, device=DEV) if split else None
        page, lay = P.layout(ops, kb, vb)
        kw = dict(page_size=page, kv_layout=lay)
        if split and fam not in ("decode_generic_kernel", "decode_mfma_bias_kernel"):   # stage 2 inside the stage-1 kernel
            kw["merge_counters"] = torch.zeros(bs * hq, dtype=torch.int32, device=DEV)
        if kn is not None:
            kw.update(k_new=kn, v_new=vn)
        if aux is not None:
            kw.update(score_mod=ops.relative_bias_score_mod, aux_tensors=[aux])
        opts = [rxlib.option(k_, v_) for k_, v_ in extra.get("opts", {}).items()]
        for cm in opts:
            cm.__enter__()
        try:
            if mode in ("i32", "i64"):
                ops.decode_attention_fwd(qd, kb, vb, o, T(ip), T(ii + base, torch.int32 if mode == "i32" else torch.int64), al, ls,
                                         splits, S, sm, ks, vs, **kw)
            else:
                table, rp, ln = T(r2t + base, torch.int32), T(rpi), T(lens)
                if mode == "units":
                    kw["units"] = ops.DecodeUnits(bs, DEV).build(table, rp, ln)
                ops.decode_attention_fwd_paged(qd, kb, vb, o, table, rp, ln, al, ls, splits, S, sm, ks, vs, **kw)
            torch.cuda.synchronize()
            return o, rxlib.last_dispatch()
        finally:
            for cm in reversed(opts):
                cm.__exit__(None, None, None)

    kt, vt = P.twins()
    o1, _ = run(kt, vt, 0)
    if kn is not None:   # (the first twin run stored the new rows: the second starts from a fresh twin)
        kt, vt = P.twins()
    o2, _ = run(kt, vt, 0)
    assert _same(o1, o2), "the twin is not bit-stable run to run"
    o, got = run(P.k, P.v, P.win.lo)
    assert got.startswith(fam + "<"), got
    assert ("req_to_token" if mode in ("r2t", "units") else "indices") in got or not fam.startswith("decode_mfma"), got
    assert P.intact()
    assert _same(o, o1), "the high window and its low twin differ: an offset was truncated"
    if kn is not None:
        assert all(_same(w, t) for w, t in zip(P.windows(), (kt, vt)))
        assert _same(P.canon(kt)[last], kn.cpu()) and _same(P.canon(vt)[last], vn.cpu())
    kbo = P.oracle_rows(kt)
    vbo = kbo[..., :512] if mla else P.oracle_rows(vt)
    want, absw = orc.decode_attention(_bits(q), kbo, vbo, ip, ii, sm, return_absw=True, k_scale=ks, v_scale=vs,
                                      score_bias=None if aux is None else aux.double().cpu().numpy())
    parity.check_out(o.float().cpu().numpy(), want, BF16, ("big pool", fam, name, mode), ulps=1, absw=absw)


# ======================================================================================================================
# extend
# ======================================================================================================================
# family, geometry, pool dtype, (Hq), index dtype, options, keyword arguments, new-token counts
EXTENDS = [
    ("extend_mfma32_kernel", "bf16_h2_d128", BF16, 4, "i64", {"ext32_autopack": 0}, {}, [300, 40, 257, 129]),
    ("extend_mfma32_kernel", "bf16_h2_d128_hnd", BF16, 8, "i32", {"ext32_pack_min_wgs": 0}, {}, [300, 40, 257, 129]),
    ("extend_mfma32_kernel", "bf16_h8_d128", BF16, 8, "i64", {}, {"mid": True}, [300, 40, 257, 129]),
    ("extend_mfma32_kernel", "fp8_h2_d128", FP8, 4, "i64", {"ext32_autopack": 0}, {"k_scale": 0.9, "v_scale": 1.25}, [300, 40, 257, 129]),
    ("extend_mfma32_kernel", "fp8_h2_d128_hnd", FP8, 8, "i32", {"ext32_autopack": 0}, {"k_scale": 0.9}, [300, 40, 257, 129]),
    ("extend_mfma_kernel", "bf16_h2_d64", BF16, 4, "i64", {"extend_d256_at64": 0}, {}, [100, 40, 57, 129]),
    ("extend_mfma_kernel", "bf16_h2_d64_hnd", BF16, 8, "i32", {"extend_d256_at64": 0}, {"sliding_window_size": 90}, [100, 40, 57, 129]),
    ("extend_mfma_kernel", "bf16_h2_d128_hnd", BF16, 4, "i64", {"extend_16x16_d128": 1}, {}, [100, 40, 57, 129]),
    ("extend_generic_kernel", "bf16_h2_d80", BF16, 4, "i64", {}, {}, [60, 9, 33, 20]),
    ("extend_d256_kernel", "bf16_h2_d64", BF16, 8, "i32", {}, {}, [300, 40, 257, 140]),
    ("extend_d256_kernel", "bf16_h2_d256_hnd", BF16, 4, "i64", {}, {"logit_cap": 30.0}, [300, 40, 257, 140]),
    ("extend_d256_kernel", "bf16_h2_d128_hnd", BF16, 16, "i64", {"extend_d256_at128": 1}, {}, [300, 40, 257, 140]),
    ("extend_nd_kernel", "bf16_h2_d96", BF16, 4, "i64", {"extend_d256": 0, "extend_d256_at96": 0}, {}, [20, 9, 57, 30]),
    ("extend_nd_kernel", "bf16_h2_d256_hnd", BF16, 8, "i64", {"extend_d256": 0}, {"sliding_window_size": 90}, [300, 40, 257, 140]),
    ("extend_mla_kernel", "bf16_mla", BF16, 16, "i64", {}, {}, [30, 9, 57, 12]),
    ("extend_mla_kernel", "bf16_mla", BF16, 5, "i64", {}, {"own_v": True}, [30, 9, 57, 12]),
]
PRE = [0, 70, 200, 33]


@pytest.mark.parametrize("fam,name,pdt,hq,idx,opts,kwargs,ext", EXTENDS, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_extend_reads_its_prefix_from_the_high_window(storage, ops, rxlib, fam, name, pdt, hq, idx, opts, kwargs, ext):
    kwargs = dict(kwargs)
    mla, own_v = name.endswith("mla"), kwargs.pop("own_v", False)
    P = Pools(storage, name, pdt, mid=kwargs.pop("mid", False), mla=mla)
    dk, dv, hkv = P.d, (512 if mla else P.d), P.h
    pre, ext = np.asarray(PRE, np.int64), np.asarray(ext, np.int64)
    T_ = int(ext.sum())
    seed = zlib.crc32(repr((fam, name, hq, idx)).encode())
    P.fill(seed)
    g = torch.Generator().manual_seed(seed)
    r2t = _paged_lists(pre, P.n, seed)
    kvp, kvi = orc.build_kv_indices(r2t, np.arange(1, len(pre) + 1), pre)
    q = torch.randn(T_, hq, dk, generator=g).to(BF16)
    ke = torch.randn(T_, hkv, dk, generator=g).to(BF16)
    ve = ke[..., :dv] if mla else torch.randn(T_, hkv, dv, generator=g).to(BF16)
    qo = np.concatenate([[0], np.cumsum(ext)]).astype(np.int64)
    ks, vs = kwargs.pop("k_scale", 1.0), kwargs.pop("v_scale", 1.0)
    qd, ked = q.to(DEV), ke.to(DEV)
    ved = (ked[..., :dv].contiguous() if own_v else ked[..., :dv]) if mla else ve.to(DEV)
    idt = torch.int32 if idx == "i32" else torch.int64

    def run(kb, vb, base):
        o = torch.full((T_, hq, dv), float("nan"), dtype=BF16, device=DEV)
        page, lay = P.layout(ops, kb, vb)
        cms = [rxlib.option(k_, v_) for k_, v_ in opts.items()]
        for cm in cms:
            cm.__enter__()
        try:
            ops.extend_attention_fwd(qd, ked, ved, o, kb, vb, torch.from_numpy(qo).to(DEV), torch.from_numpy(kvp).to(DEV).to(torch.int32),
                                     torch.from_numpy(kvi + base).to(DEV).to(idt), None, True, None, int(ext.max()), ks, vs,
                                     sm_scale=dk ** -0.5, page_size=page, kv_layout=lay, **kwargs)
            torch.cuda.synchronize()
            return o, rxlib.last_dispatch()
        finally:
            for cm in reversed(cms):
                cm.__exit__(None, None, None)

    kt, vt = P.twins()
    o1, _ = run(kt, vt, 0)
    o2, _ = run(kt, vt, 0)
    assert _same(o1, o2), "the twin is not bit-stable run to run"
    o, got = run(P.k, P.v, P.win.lo)
    assert got.startswith(fam + "<"), got
    assert P.intact()
    assert _same(o, o1), "the high window and its low twin differ: an offset was truncated"
    kbo = P.oracle_rows(kt)
    vbo = kbo[..., :512] if mla else P.oracle_rows(vt)
    want, absw = orc.extend_attention(_bits(q), _bits(ke), _bits(ve.contiguous()), kbo, vbo, qo, kvp.astype(np.int32), kvi,
                                      is_causal=True, sm_scale=dk ** -0.5, return_absw=True, k_scale=ks, v_scale=vs, **kwargs)
    parity.check_out(o.float().cpu().numpy(), want, BF16, ("big pool", fam, name, idx), ulps=1, absw=absw)


@pytest.mark.parametrize("name,hq,idx,small", [("bf16_h2_d128", 8, "i64", 1), ("bf16_h2_d128_hnd", 4, "i32", 0)], ids=lambda v: str(v))
def test_unified_extend_with_every_row_in_the_high_window(storage, ops, rxlib, name, hq, idx, small):
    """extend_attention_fwd_unified reads the new tokens from the pool too: they are stored into the window first
    (store_cache / store_cache_layout, whose own case is above)."""
    P = Pools(storage, name, BF16)
    d, hkv = P.d, P.h
    pre, ext = np.asarray(PRE, np.int64), np.asarray([120, 40, 57, 129], np.int64)
    T_ = int(ext.sum())
    seed = zlib.crc32(repr(("unified", name)).encode())
    P.fill(seed)
    g = torch.Generator().manual_seed(seed)
    r2t = _paged_lists(pre + ext, P.n, seed)
    kvp, kvi = orc.build_kv_indices(r2t, np.arange(1, len(pre) + 1), pre + ext)
    new = np.concatenate([r2t[i + 1, p: p + e] for i, (p, e) in enumerate(zip(pre, ext))])
    q = torch.randn(T_, hq, d, generator=g).to(BF16)
    ke, ve = (torch.randn(T_, hkv * d, generator=g).to(BF16).to(DEV) for _ in range(2))
    loc = torch.from_numpy(new + P.win.lo).to(DEV)
    if P.hnd:
        ops.store_cache_layout(ke, ve, ops.kv_layout_hnd(P.k, P.v), loc, hkv, d, d, size_limit=P.win.hi)
    else:
        ops.store_cache(ke, ve, P.k, P.v, loc)
    torch.cuda.synchronize()
    qo = np.concatenate([[0], np.cumsum(ext)]).astype(np.int64)
    qd = q.to(DEV)
    idt = torch.int32 if idx == "i32" else torch.int64

    def run(kb, vb, base):
        o = torch.full((T_, hq, d), float("nan"), dtype=BF16, device=DEV)
        page, lay = P.layout(ops, kb, vb)
        with rxlib.option("ext32_small_wg", small):
            ops.extend_attention_fwd_unified(qd, o, kb, vb, 1.0, 1.0, torch.from_numpy(qo).to(DEV), torch.from_numpy(kvp).to(DEV).to(torch.int32),
                                             torch.from_numpy(kvi + base).to(DEV).to(idt), torch.from_numpy(pre.astype(np.int32)).to(DEV),
                                             int(ext.max()), sm_scale=d ** -0.5, is_causal=True, page_size=page, kv_layout=lay)
            torch.cuda.synchronize()
            return o, rxlib.last_dispatch()

    kt, vt = P.twins()
    o1, _ = run(kt, vt, 0)
    o2, _ = run(kt, vt, 0)
    assert _same(o1, o2), "the twin is not bit-stable run to run"
    o, got = run(P.k, P.v, P.win.lo)
    assert got.startswith("extend_mfma32_uni_kernel<"), got
    assert P.intact() and _same(o, o1)
    assert _same(P.canon(kt)[new], ke.view(T_, hkv, d).cpu())   # (the stored rows are where the lists say)
    want, absw = orc.extend_attention_unified(_bits(q), P.oracle_rows(kt), P.oracle_rows(vt), qo, kvp.astype(np.int32), kvi, pre,
                                              sm_scale=d ** -0.5, return_absw=True)
    parity.check_out(o.float().cpu().numpy(), want, BF16, ("big pool", "unified", name), ulps=1, absw=absw)


# ======================================================================================================================
# RoPE with the fused store
# ======================================================================================================================
@pytest.mark.parametrize("op", ["rope_store_kv", "fused_qk_norm_rope"])
@pytest.mark.parametrize("name,dtype", [("bf16_h2_d128", BF16), ("bf16_h2_d128_hnd", BF16), ("fp8_h2_d128", FP8), ("fp8_h2_d128_hnd", FP8)],
                         ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_rope_with_fused_store_reaches_the_high_window(storage, ops, op, name, dtype, idt):
    """The pool rows must be the k rows the op leaves behind (rotated, and normalised by fused_qk_norm_rope) and the v
    rows, divided by the scales (powers of two) and rounded to e4m3fn on an fp8 pool."""
    P = Pools(storage, name, dtype)
    n, hq, hkv, d = 50, 4, P.h, P.d
    g = torch.Generator().manual_seed(zlib.crc32((op + name).encode()))
    qkv0 = torch.randn(n, (hq + 2 * hkv) * d, generator=g).to(BF16).to(DEV)
    pos = torch.randint(0, 500, (n,), generator=g).to(DEV)
    ang = torch.arange(512)[:, None] * (10000.0 ** (-torch.arange(0, d, 2) / d))[None]
    cache = torch.cat([ang.cos(), ang.sin()], -1).float().to(DEV)
    w = [(1.0 + 0.1 * torch.randn(d, generator=g)).to(BF16).to(DEV) for _ in range(2)]
    ks, vs = (0.5, 2.0) if dtype == FP8 else (1.0, 1.0)
    rel = _loc(P, n, 17, idt).to(DEV)

    def run(kb, vb, loc, slots):
        qkv = qkv0.clone()
        lay = ops.kv_layout_hnd(kb, vb) if P.hnd else ops._kv_layout(kb, vb, 1)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        kw = dict(layout=lay, loc=loc, size_limit=slots, k_scale=ks, v_scale=vs, err_flag=err)
        if op == "rope_store_kv":
            q, k, v = (qkv[:, a * d: b * d].view(n, -1, d) for a, b in ((0, hq), (hq, hq + hkv), (hq + hkv, hq + 2 * hkv)))
            ops.rope_store_kv(q, k, v, pos, cache, True, **kw)
        else:
            ops.fused_qk_norm_rope(qkv, hq, hkv, hkv, d, 1e-6, w[0], w[1], 10000.0, True, pos, **kw)
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        return qkv

    P.poison()
    kt, vt = P.twins()
    r1 = run(kt, vt, rel, P.n)
    kt2, vt2 = P.twins()
    r2 = run(kt2, vt2, rel, P.n)
    assert _same(r1, r2) and _same(kt, kt2) and _same(vt, vt2) and not _same(r1, qkv0)
    r = run(P.k, P.v, rel + P.win.lo, P.win.hi)
    assert P.intact(), "the fused store went to an alias of its slot (a truncated offset)"
    assert _same(r, r1) and all(_same(a, b) for a, b in zip(P.windows(), (kt, vt)))
    for rows, cols, scale in ((P.canon(kt), (hq, hq + hkv), ks), (P.canon(vt), (hq + hkv, hq + 2 * hkv), vs)):
        want = r1[:, cols[0] * d: cols[1] * d].reshape(n, hkv, d).cpu()
        if dtype == FP8:
            want = (want.float() / scale).to(FP8).view(torch.uint8)
        assert _same(rows[rel.cpu().long()], want), op
        untouched = torch.ones(P.n, dtype=torch.bool)
        untouched[rel.cpu().long()] = False
        assert bool((rows[untouched].contiguous().view(torch.uint8) == 0x5A).all())


# ======================================================================================================================
# move_kv_layout
# ======================================================================================================================
@pytest.mark.parametrize("direction", ["high_to_high", "high_to_low", "low_to_high"])
@pytest.mark.parametrize("name", ["bf16_h8_d128_hnd", "bf16_h2_d64_hnd"])
def test_move_kv_layout_between_low_and_high_slots(storage, ops, name, direction):
    """rx_move_kv_layout on both buffers of an HND page-16 pool; low pages above the alias pages, as for move_kv."""
    P = Pools(storage, name, BF16)
    P.fill(21)
    low0 = max(P.win.alias_slots) + 1
    assert low0 % PS == 0
    low = [p[low0 // PS: (low0 + P.n) // PS] for p in (P.k, P.v)]
    g = torch.Generator().manual_seed(23)
    for rows in low:
        rows.copy_(torch.randn(rows.shape, generator=g).to(P.dtype).to(DEV))
    n = 40
    perm = torch.randperm(P.n, generator=g)
    src_rel, tgt_rel = perm[:n].to(DEV), perm[n: 2 * n].to(DEV)
    src_hi, tgt_hi = direction != "low_to_high", direction != "high_to_low"
    twins = [torch.cat([lo_, hi_]) for lo_, hi_ in zip(low, P.windows())]   # [low pages | window pages] of each buffer
    ts, tt = src_rel + (P.n if src_hi else 0), tgt_rel + (P.n if tgt_hi else 0)
    es = P.k.element_size()
    geom = torch.tensor([[P.h * PS * P.d * es, PS * P.d * es, P.d * es, P.d * es]] * 2, dtype=torch.int64, device=DEV)

    def canon(t):   # [pages, H, page, D] -> bytes [slots, H, D * es]
        return t.contiguous().view(torch.uint8).view(t.shape[0], P.h, PS, -1).permute(0, 2, 1, 3).reshape(t.shape[0] * PS, P.h, -1)

    want = [canon(t).clone() for t in twins]
    for w in want:
        w[tt] = w[ts]
    for rep in range(2):
        tw = [t.clone() for t in twins]
        ops.move_kv_layout(torch.tensor([t.data_ptr() for t in tw], dtype=torch.int64, device=DEV), geom, PS, P.h, tt, ts)
        torch.cuda.synchronize()
        assert all(_same(canon(a), b) for a, b in zip(tw, want))
    ops.move_kv_layout(torch.tensor([P.k.data_ptr(), P.v.data_ptr()], dtype=torch.int64, device=DEV), geom, PS, P.h,
                       tgt_rel + (P.win.lo if tgt_hi else low0), src_rel + (P.win.lo if src_hi else low0))
    torch.cuda.synchronize()
    assert P.intact(), "a move read or wrote an alias of its slot"
    for lo_, hi_, w in zip(low, P.windows(), want):
        assert _same(canon(torch.cat([lo_, hi_])), w)


# ======================================================================================================================
# cascade (shared-prefix) decode
# ======================================================================================================================
@pytest.mark.parametrize("name,hq", [("bf16_h8_d128", 32), ("bf16_h2_d128_hnd", 8)], ids=lambda v: str(v))
def test_cascade_decode_with_its_shared_prefix_in_the_high_window(storage, ops, rxlib, name, hq):
    P = Pools(storage, name, BF16)
    d, hkv, shared = P.d, P.h, 192
    priv = np.array([1, 40, 92, 17], dtype=np.int64)
    lens, bs = shared + priv, len(priv)
    seed = zlib.crc32(("cascade" + name).encode())
    P.fill(seed)
    g = torch.Generator().manual_seed(seed)
    lists = _paged_lists([shared] + list(priv), P.n, seed)   # row 1: the shared pages, rows 2..: the private ones
    r2t = np.zeros((bs + 1, int(lens.max()) + PS), dtype=np.int64)
    for i, p_ in enumerate(priv):
        r2t[i + 1, :shared], r2t[i + 1, shared: shared + p_] = lists[1, :shared], lists[i + 2, :p_]
    rpi = np.arange(1, bs + 1, dtype=np.int64)
    ip, ii = orc.build_kv_indices(r2t, rpi, lens)
    q = torch.randn(bs, hq, d, generator=g).to(BF16)
    qd, sm = q.to(DEV), d ** -0.5

    def run(kb, vb, base):
        o = torch.full((bs, hq, d), float("nan"), dtype=BF16, device=DEV)
        page, lay = P.layout(ops, kb, vb)
        cd = ops.CascadeDecode(bs, hq, hkv, d, BF16, DEV, max_shared=512, min_shared=64)
        cd.plan(_dev(r2t + base, torch.int32), _dev(rpi), _dev(lens))
        assert cd.shared_len() == shared
        cd(qd, kb, vb, o, sm, page_size=page, kv_layout=lay)
        torch.cuda.synchronize()
        return o, rxlib.last_dispatch()

    kt, vt = P.twins()
    o1, _ = run(kt, vt, 0)
    o2, _ = run(kt, vt, 0)
    assert _same(o1, o2), "the twin is not bit-stable run to run"
    o, got = run(P.k, P.v, P.win.lo)
    assert got.startswith("decode_mfma_kernel<") and "req_to_token" in got, got   # (the suffix launch; the shared rows went through the extend kernel)
    assert P.intact() and _same(o, o1)
    want, absw = orc.decode_attention(_bits(q), P.oracle_rows(kt), P.oracle_rows(vt), ip, ii, sm, return_absw=True)
    # (two 16-bit roundings: the chunk partials cross 16-bit buffers before the merge -- 2 ulp, as test_gpu_cascade.py)
    parity.check_out(o.float().cpu().numpy(), want, BF16, ("big pool", "cascade", name), ulps=2, absw=absw)


# ======================================================================================================================
# 4-bit (MXFP4 block-16) pools
# ======================================================================================================================
class Mx4(Pools):
    """Data views as Pools (bytes), plus the scale-byte views [slots, Hkv * D / 16] and their guard rows.  mla: one buffer."""

    def __init__(self, storage, name, mla=False):
        super().__init__(storage, name, torch.uint8)
        self.latent = mla
        if mla:
            self.bases, self.v = self.bases[:1], self.k
        self.srow = self.h * self.d // 8
        self.scales = [bp.scale_view(storage, i, self.srow, self.win) for i in range(len(self.bases))]

    def windows(self):
        return [bp.window_rows(p, self.win) for p in ((self.k,) if self.latent else (self.k, self.v))]

    def scale_windows(self):
        return [s[self.win.lo: self.win.hi] for s in self.scales]

    def _guards(self):
        return [r for i in range(len(self.scales)) for r in bp.scale_ranges(i, self.srow, self.win)[2]]

    def prepare(self, seed=None):
        """seed: random data bytes and scale bytes 119..127 (K) / 121..129 (V); None: 0x5A everywhere (stores)"""
        if seed is None:
            self.poison()
        else:
            self.fill(seed)
        g = torch.Generator().manual_seed(seed or 0)
        for i, sw in enumerate(self.scale_windows()):
            sw.copy_(torch.full(sw.shape, 0x5A, dtype=torch.uint8) if seed is None
                     else torch.randint(119 + 2 * i, 128 + 2 * i, sw.shape, generator=g, dtype=torch.uint8))
        for lo, hi in self._guards():
            self.storage[lo:hi] = bp.SENTINEL

    def all_twins(self):
        """([data twins], [scale twins]) of the windows"""
        return [w.clone() for w in self.windows()], [s.clone() for s in self.scale_windows()]

    def all_intact(self):
        return self.intact() and all(bool((self.storage[lo:hi] == bp.SENTINEL).all()) for lo, hi in self._guards())

    def dequant(self, data, scales):
        from test_gpu_kv_mx4 import mx4_dequant

        return mx4_dequant(data.cpu().numpy(), scales.cpu().numpy().reshape(data.shape[0], self.h, -1))


@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("mla", [False, True], ids=["kv", "latent"])
def test_mx4_store_and_gather_reach_the_high_window(storage, ops, mla, idt):
    from test_gpu_kv_mx4 import mx4_quant

    P = Mx4(storage, "mx4_mla" if mla else "mx4_h2_d128", mla)
    n, h, D = 60, P.h, 2 * P.d
    g = torch.Generator().manual_seed(31 + mla)
    src = [(torch.randn(n, h * D // 16, 16, generator=g) * torch.exp2(torch.randint(-4, 5, (n, h * D // 16, 1), generator=g).float()))
           .to(BF16).view(n, h * D).to(DEV) for _ in range(1 if mla else 2)]
    rel = _loc(P, n, 33, idt).to(DEV)

    def store(data, scales, loc):
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        if mla:
            ops.store_cache_mla_mx4(src[0], None, data[0], scales[0], loc, page_size=PS, err_flag=err)
        else:
            ops.store_cache_mx4(src[0], src[1], data[0], data[1], scales[0], scales[1], loc, page_size=PS, err_flag=err)
        torch.cuda.synchronize()
        assert int(err.item()) == 0

    def gather(data, scales, loc):
        if mla:
            return ops.get_mla_kv_mx4(data[0], scales[0], loc, 512, 64, BF16, page_size=PS)
        return ops.gather_kv_mx4(data[0], data[1], scales[0], scales[1], loc, BF16, page_size=PS)

    P.prepare(None)
    d1, s1 = P.all_twins()
    store(d1, s1, rel)
    d2, s2 = P.all_twins()
    store(d2, s2, rel)
    assert all(_same(a, b) for a, b in zip(d1 + s1, d2 + s2))
    store([P.k, P.v][: len(d1)], P.scales, rel + P.win.lo)
    assert P.all_intact(), "a store went to an alias of its slot or outside the scale window"
    assert all(_same(a, b) for a, b in zip(P.windows() + P.scale_windows(), d1 + s1))
    idx = rel.cpu().long()
    for x, data, sb in zip(src, d1, s1):   # the format restated in numpy (test_gpu_kv_mx4.mx4_quant)
        wd, ws = mx4_quant(x.float().cpu().numpy().reshape(n, h, D))
        assert np.array_equal(data.cpu().numpy()[idx], wd) and np.array_equal(sb.cpu().numpy()[idx].reshape(n, h, -1), ws)
        untouched = torch.ones(P.n, dtype=torch.bool)
        untouched[idx] = False
        assert bool((data.cpu()[untouched] == 0x5A).all()) and bool((sb.cpu()[untouched] == 0x5A).all())
    a = gather(d1, s1, rel)
    b = gather(d1, s1, rel)
    c = gather([P.k, P.v][: len(d1)], P.scales, rel + P.win.lo)
    torch.cuda.synchronize()
    assert all(_same(x, y) and _same(x, z) for x, y, z in zip(a, b, c))
    got = torch.cat([t.cpu() for t in c], -1).view(n, h, D) if mla else None
    for i, (data, sb) in enumerate(zip(d1, s1)):
        want = torch.from_numpy(P.dequant(data, sb)[idx.numpy()]).to(BF16)
        assert _same(got if mla else c[i].cpu(), want)


MX4_DECODES = [("decode_mx4_kernel", False, 8, "i64", True), ("decode_mx4_kernel", False, 4, "r2t", False),
               ("decode_mx4_kernel", False, 8, "i32", False), ("decode_mla_mx4_kernel", True, 16, "i64", True),
               ("decode_mla_mx4_kernel", True, 5, "r2t", False), ("decode_mla_mx4_kernel", True, 16, "i32", False)]


@pytest.mark.parametrize("fam,mla,hq,mode,split", MX4_DECODES, ids=lambda v: str(v))
def test_mx4_decode_reads_the_high_window(storage, ops, rxlib, fam, mla, hq, mode, split):
    P = Mx4(storage, "mx4_mla" if mla else "mx4_h2_d128", mla)
    dk, dv = 2 * P.d, (512 if mla else 2 * P.d)
    lens = np.array([1, 33, 257, 300], dtype=np.int64)
    bs = len(lens)
    seed = zlib.crc32(repr((fam, hq, mode, split)).encode())
    P.prepare(seed)
    g = torch.Generator().manual_seed(seed)
    r2t = _paged_lists(lens, P.n, seed)
    rpi = np.arange(1, bs + 1, dtype=np.int64)
    ip, ii = orc.build_kv_indices(r2t, rpi, lens)
    q = torch.randn(bs, hq, dk, generator=g).to(BF16)
    qd, sm = q.to(DEV), dk ** -0.5
    S = 8 if split else 1
    splits = torch.tensor([1, 2, 2, 3], dtype=torch.int32, device=DEV) if split else None

    def run(data, scales, base):
        o = torch.full((bs, hq, dv), float("nan"), dtype=BF16, device=DEV)
        al = torch.zeros(bs, hq, S, dv, dtype=torch.float32, device=DEV) if split else None
        ls = torch.zeros(bs, hq, S, dtype=torch.float32, device=DEV) if split else None
        kw = dict(page_size=PS, k_scale_buffer=scales[0], v_scale_buffer=None if mla else scales[1])
        if mode == "r2t":
            ops.decode_attention_fwd_paged(qd, data[0], data[-1], o, _dev(r2t + base, torch.int32), _dev(rpi), _dev(lens), al, ls,
                                           splits, S, sm, 1.0, 1.0, **kw)
        else:
            ops.decode_attention_fwd(qd, data[0], data[-1], o, _dev(ip), _dev(ii + base, torch.int32 if mode == "i32" else torch.int64),
                                     al, ls, splits, S, sm, 1.0, 1.0, **kw)
        torch.cuda.synchronize()
        return o, rxlib.last_dispatch()

    dt_, st_ = P.all_twins()
    o1, _ = run(dt_, st_, 0)
    o2, _ = run(dt_, st_, 0)
    assert _same(o1, o2), "the twin is not bit-stable run to run"
    o, got = run([P.k, P.v][: len(dt_)], P.scales, P.win.lo)
    assert got.startswith(fam + "<"), got
    assert P.all_intact() and _same(o, o1), "the high window and its low twin differ: an offset was truncated"
    kbo = P.dequant(dt_[0], st_[0])
    vbo = kbo[..., :512] if mla else P.dequant(dt_[1], st_[1])
    want, absw = orc.decode_attention(_bits(q), kbo, vbo, ip, ii, sm, return_absw=True)
    parity.check_out(o.float().cpu().numpy(), want, BF16, ("big pool", fam, mode), ulps=1, absw=absw)


@pytest.mark.parametrize("hq,idx", [(8, "i64"), (2, "i32")], ids=lambda v: str(v))
def test_mx4_extend_reads_its_prefix_from_the_high_window(storage, ops, rxlib, hq, idx):
    P = Mx4(storage, "mx4_h2_d128")
    d, hkv = 2 * P.d, P.h
    pre, ext = np.asarray(PRE, np.int64), np.asarray([100, 40, 57, 129], np.int64)
    T_ = int(ext.sum())
    seed = zlib.crc32(repr(("extend_mx4", hq, idx)).encode())
    P.prepare(seed)
    g = torch.Generator().manual_seed(seed)
    r2t = _paged_lists(pre, P.n, seed)
    kvp, kvi = orc.build_kv_indices(r2t, np.arange(1, len(pre) + 1), pre)
    q, ke, ve = (torch.randn(T_, h_, d, generator=g).to(BF16) for h_ in (hq, hkv, hkv))
    qo = np.concatenate([[0], np.cumsum(ext)]).astype(np.int64)
    qd, ked, ved = q.to(DEV), ke.to(DEV), ve.to(DEV)
    idt = torch.int32 if idx == "i32" else torch.int64

    def run(data, scales, base):
        o = torch.full((T_, hq, d), float("nan"), dtype=BF16, device=DEV)
        ops.extend_attention_fwd(qd, ked, ved, o, data[0], data[1], _dev(qo), _dev(kvp, torch.int32), _dev(kvi + base, idt), None, True,
                                 None, int(ext.max()), 1.0, 1.0, sm_scale=d ** -0.5, page_size=PS, k_scale_buffer=scales[0],
                                 v_scale_buffer=scales[1])
        torch.cuda.synchronize()
        return o, rxlib.last_dispatch()

    dt_, st_ = P.all_twins()
    o1, _ = run(dt_, st_, 0)
    o2, _ = run(dt_, st_, 0)
    assert _same(o1, o2), "the twin is not bit-stable run to run"
    o, got = run([P.k, P.v], P.scales, P.win.lo)
    assert got.startswith("extend_mx4_kernel<"), got
    assert P.all_intact() and _same(o, o1), "the high window and its low twin differ: an offset was truncated"
    want, absw = orc.extend_attention(_bits(q), _bits(ke), _bits(ve), P.dequant(dt_[0], st_[0]), P.dequant(dt_[1], st_[1]), qo,
                                      kvp.astype(np.int32), kvi, is_causal=True, sm_scale=d ** -0.5, return_absw=True)
    parity.check_out(o.float().cpu().numpy(), want, BF16, ("big pool", "extend_mx4", idx), ulps=1, absw=absw)
