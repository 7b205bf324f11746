"""The edges of the two 4-bit (MXFP4 block-16) pools that tests/test_gpu_kv_mx4.py and tests/test_gpu_mla_mx4.py leave out.

* every compiled instance of decode_mx4_kernel / decode_mla_mx4_kernel is the `expect` of a case of INSTANCE_CASES (a CPU test
  holds the table to the library's symbol table, both ways); the cases carry GQA groups above 16 (two q blocks, a partly filled
  last one), page sizes 1 / 48 / 64 and the padded-page views, splits longer than 512 tokens;
* empty requests (single pass and split-KV, the latter held to what rx_decode_attn gives on a 16-bit pool), xai_temperature_len
  and request_order on both kernels;
* scale bytes over the whole in-contract range: the gathers bit for bit, the decode kernels with neighbouring blocks of a row
  at very different scales; the store at the top and the bottom of each dtype's range; a gather above the largest finite value;
* adversarial score sequences (scale bytes that rise, fall or spike along the context).

Every attention result goes through parity_util.check_out with ulps=1 against the fp64 oracle fed the exactly dequantised
bytes the pool holds (the bound of the existing 4-bit cases); stores and gathers are compared bit for bit."""
import os
import re
import subprocess
import types
import zlib

import numpy as np
import pytest
import torch

import parity_util as parity
from oracle import radix_oracle as orc
from test_gpu_kv_mx4 import BOUNDS, PS, _canon, _dev, _random_pool, _step, mx4_dequant, mx4_quant

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
RANK, ROPE, DL = 512, 64, 576   # the latent row: d == DL selects decode_mla_mx4_kernel (v = the first RANK columns)
FAMILIES = ("decode_mx4_kernel", "decode_mla_mx4_kernel")


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _table(rng, lens, ps):
    """req_to_token rows [bs + 1, max + ps] over shuffled pages (page 0 unused) and the number of pages"""
    pages = [-(-int(n) // ps) for n in lens]
    n_pages = sum(pages) + 3
    ids = rng.permutation(np.arange(1, n_pages))
    r2t = np.zeros((len(lens) + 1, max(int(max(lens)), 1) + ps), dtype=np.int32)
    pi = 0
    for i, n in enumerate(lens):
        r2t[i + 1, : int(n)] = (ids[pi: pi + pages[i], None] * ps + np.arange(ps)[None]).reshape(-1)[: int(n)]
        pi += pages[i]
    return r2t, n_pages


def _put(a, lay, ps, flat=False, dev=DEV):
    """canonical [slots, H, X] bytes -> the buffer of layout `lay`: "nhd" as is (scales flat [slots, H * X]), "hnd" pages
    [pages, H, page, X], "pad" the [:, :, :page] view of HND pages with two pad tokens (never slot-major, whatever H)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if lay == "nhd":
        return (t.view(a.shape[0], -1) if flat else t).to(dev)
    paged = t.view(-1, ps, *a.shape[1:]).permute(0, 2, 1, 3)
    if lay == "hnd":
        return paged.contiguous().to(dev)
    buf = torch.zeros(paged.shape[0], a.shape[1], ps + 2, a.shape[2], dtype=torch.uint8)
    buf[:, :, :ps] = paged
    return buf.to(dev)[:, :, :ps]


def _get(t, lay, like):
    t = t.cpu()
    return (t if lay == "nhd" else t.permute(0, 2, 1, 3)).reshape(like.shape).numpy()


def _expect(c):
    """the instance and lookup the launchers must name for case c"""
    hkv, ps, lay = c["heads"][1], c.get("page", PS), c["lay"]
    idx = "long" if c["mode"] == "i64" else "int"
    tail = "req_to_token" if c["mode"] == "r2t" else "indices"
    linear = ps == 1 or lay == "nhd" or (lay == "hnd" and hkv == 1)   # (one kv head makes HND pages slot-major)
    lin = "true" if linear else "false"
    if c["d"] == DL:
        return f"decode_mla_mx4_kernel<rx::{c['dt'].upper()}, {idx}, {lin}>", tail
    return f"decode_mx4_kernel<rx::{c['dt'].upper()}, {c['d']}, {idx}, {lin}>", "slots," + tail


def _default_pool(rng, slots, hkv, d, r2t, lens):
    """random nibbles, scale bytes of the existing cases (K 119..127, V 121..129; latent rows 119..127)"""
    if d == DL:
        return [rng.integers(0, 256, (slots, 1, d // 2), dtype=np.uint8), rng.integers(119, 128, (slots, 1, d // 16)).astype(np.uint8)]
    return _random_pool(rng, slots, hkv, d)


def _attend(c, q, bufs, r2t, lens, ip, ii, okw, order=None):
    """the decode call of case c on the device buffers (k data, k scales, v data, v scales): (o, dispatch, num_kv_splits)"""
    from sglang_amd import lib as rxlib
    from sglang_amd import ops

    d, (hq, hkv), ps, S = c["d"], c["heads"], c.get("page", PS), c.get("S", 1)
    dv, bs = (RANK if d == DL else d), len(lens)
    kd, ksd, vd, vsd = bufs
    lens_d = _T(lens)
    splits = al = ls = None
    if S > 1:
        splits = torch.zeros(bs, dtype=torch.int32, device=DEV)
        ops.get_num_kv_splits_balanced(splits, lens_d, hq, hkv, S, 64, 128)   # (a small budget: the long requests are cut)
        al =torch.zeros(bs, hq, S, dv, dtype=torch.float32, device=DEV)
        ls = torch.zeros(bs, hq, S, dtype=torch.float32, device=DEV)
    o = torch.full((bs, hq, dv), float("nan"), dtype=q.dtype, device=DEV)
    kw = dict(page_size=ps, k_scale_buffer=ksd, v_scale_buffer=vsd, logit_cap=okw.get("logit_cap", 0.0),
              sinks=_T(okw["sinks"]) if "sinks" in okw else None, xai_temperature_len=okw.get("xai_temperature_len", -1),
              request_order=order)
    ksc, vsc, sm = okw.get("k_scale", 1.0), okw.get("v_scale", 1.0), d ** -0.5
    if c["mode"] == "r2t":
        rpi = np.arange(1, bs + 1, dtype=np.int64)
        ops.decode_attention_fwd_paged(q, kd, vd, o, _T(r2t), _T(rpi), lens_d, al, ls, splits, S, sm, ksc, vsc, **kw)
    else:
        ops.decode_attention_fwd(q, kd, vd, o, _T(ip), _T(ii).to(torch.int64 if c["mode"] == "i64" else torch.int32), al, ls,
                                 splits, S, sm, ksc, vsc, **kw)
    torch.cuda.synchronize()
    return o, rxlib.last_dispatch(), splits


def _oracle_kw(c, rng):
    """c["kw"] (k_scale, v_scale, logit_cap, sinks: True, xai: L) as the oracle's keyword arguments"""
    kw = c.get("kw", {})
    okw = {k: kw[k] for k in ("k_scale", "v_scale", "logit_cap") if k in kw}
    if kw.get("sinks"):
        okw["sinks"] = rng.standard_normal(c["heads"][0]).astype(np.float32)
    if "xai" in kw:
        okw["xai_temperature_len"] = kw["xai"]
    return okw


def _decode(c, pool_fn=_default_pool, qmul=None, order=False):
    """Case c -- dt, d (64 / 128 / DL), mode (i32 / i64 / r2t), lay (nhd / hnd / pad), page, heads (Hq, Hkv), lens, S (kv
    splits, 1 = single pass), kw -- on a pool from pool_fn: asserts the dispatch, no NaN, and parity with the oracle on the
    rows of the non-empty requests.  qmul [d]: exact powers of two on q (values below 1/8 are lifted first, so that nothing
    lands under the 16-bit normal range).  Returns what the call saw and gave."""
    dt, d, lay, ps, (hq, hkv) = c["dt"], c["d"], c["lay"], c.get("page", PS), c["heads"]
    dtype, mla = DT[dt], c["d"] == DL
    lens = np.asarray(c["lens"], dtype=np.int64)
    bs = len(lens)
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    r2t, n_pages = _table(rng, lens, ps)
    pool = pool_fn(rng, n_pages * ps, hkv, d, r2t, lens)
    kf = mx4_dequant(pool[0], pool[1])
    vf = kf[..., :RANK] if mla else mx4_dequant(pool[2], pool[3])
    qf = torch.from_numpy(rng.standard_normal((bs, hq, d)).astype(np.float32))
    if qmul is not None:
        qf = torch.where(qf.abs() < 0.125, torch.copysign(torch.tensor(0.125), qf), qf) * torch.from_numpy(np.asarray(qmul, np.float32))
    q = qf.to(dtype)
    ip, ii = orc.build_kv_indices(r2t, np.arange(1, bs + 1, dtype=np.int64), lens)
    okw = _oracle_kw(c, rng)
    qb = q.view(torch.uint16).numpy() if dtype == torch.bfloat16 else q.numpy()
    want, absw = orc.decode_attention(qb, kf, vf, ip, ii, d ** -0.5, return_absw=True, **okw)
    if mla:   # one buffer; the scale bytes [slots, 36] -- v_scale_buffer None or the same tensor, by turns
        kd, ksd = _put(pool[0], lay, ps), _put(pool[1], lay, ps, flat=True)
        bufs = (kd, ksd, kd, ksd if hq % 2 else None)
    else:
        bufs = tuple(_put(a, lay, ps, flat=i % 2 == 1) for i, a in enumerate(pool))
    order_t = torch.argsort(_T(lens), descending=True, stable=True).to(torch.int32) if order else None
    o, name, splits = _attend(c, q.to(DEV), bufs, r2t, lens, ip, ii, okw, order_t)
    inst, tail = _expect(c)
    assert name == f"{inst}|{tail}", (name, inst, tail)
    assert splits is None or int(splits.max()) > 1
    got, live = o.float().cpu().numpy(), lens > 0
    assert not np.isnan(got[live]).any(), c
    # the unpack is exact, so the result carries the 16-bit kernel's roundings: the bound of the existing 4-bit cases
    parity.check_out(got[live], want[live], dtype, ("mx4 edges", _cid(c)), ulps=1, absw=absw[live])
    return types.SimpleNamespace(o=o, got=got, live=live, q=q, kf=kf, vf=vf, ip=ip, ii=ii, lens=lens, splits=splits, okw=okw)


def _cid(c):
    return "-".join(str(c[k]).replace(" ", "") for k in ("dt", "d", "mode", "lay", "heads") if k in c) + \
        f"-p{c.get('page', PS)}-S{c.get('S', 1)}" + ("-" + c["tag"] if "tag" in c else "")


# ----------------------------------------------------------------------------------------------------------------------
# A. one case per compiled instance (the CPU test holds this table to the library, both ways)
# ----------------------------------------------------------------------------------------------------------------------
LENS_SINGLE = [1, 16, 17, 33, 64, 65, 300, 1100]   # (above 1024: the second-level slot prefetch of decode_mx4_kernel)
LENS_SPLIT = [1, 17, 33, 65, 300, 700, 2100]       # (two splits of 2100: more than 512 tokens each, the register sets refill)


def _instance_cases():
    out = []
    # decode_mx4_kernel<T, D, IdxT, LINEAR>.  LINEAR = false: HND pages with two kv heads; true: NHD, or HND with one kv head.
    # GQA groups 20 (a partly filled second q block) and 32 (two full ones) throughout; pages 1, 16, 48, 64.
    mha = {
        ("bf16", 128, "int", False): ("i32", "hnd", 48, (40, 2), 1), ("bf16", 128, "long", False): ("i64", "hnd", 64, (64, 2), 2),
        ("bf16", 64, "int", False): ("r2t", "hnd", 48, (64, 2), 2), ("bf16", 64, "long", False): ("i64", "hnd", 16, (40, 2), 1),
        ("f16", 128, "int", False): ("r2t", "hnd", 64, (64, 2), 1), ("f16", 128, "long", False): ("i64", "hnd", 48, (40, 2), 2),
        ("f16", 64, "int", False): ("i32", "hnd", 64, (40, 2), 2), ("f16", 64, "long", False): ("i64", "hnd", 48, (64, 2), 1),
        ("bf16", 128, "int", True): ("r2t", "hnd", 48, (32, 1), 2), ("bf16", 128, "long", True): ("i64", "nhd", 1, (20, 1), 1),
        ("bf16", 64, "int", True): ("i32", "nhd", 1, (20, 1), 2), ("bf16", 64, "long", True): ("i64", "hnd", 64, (32, 1), 1),
        ("f16", 128, "int", True): ("r2t", "hnd", 16, (20, 1), 1), ("f16", 128, "long", True): ("i64", "nhd", 48, (32, 1), 2),
        ("f16", 64, "int", True): ("r2t", "nhd", 1, (32, 1), 1), ("f16", 64, "long", True): ("i64", "hnd", 48, (20, 1), 2),
    }
    for (dt, d, _, _), (mode, lay, page, heads, S) in mha.items():
        out.append(dict(dt=dt, d=d, mode=mode, lay=lay, page=page, heads=heads, S=S, lens=LENS_SPLIT if S > 1 else LENS_SINGLE))
    # ... and padded pages under ONE kv head (not slot-major although Hkv == 1), a page that is no power of two
    out.append(dict(dt="bf16", d=128, mode="i64", lay="pad", page=48, heads=(20, 1), S=1, lens=LENS_SINGLE))
    out.append(dict(dt="f16", d=64, mode="i32", lay="pad", page=16, heads=(5, 1), S=2, lens=LENS_SPLIT))
    # decode_mla_mx4_kernel<T, IdxT, LINEAR>: Hq 1, 17 (a second q block with one head) and 128 (short contexts)
    short = [1, 17, 33, 65, 300]
    mla = {
        ("bf16", "int", True): ("r2t", "nhd", 1, 17, 1, LENS_SINGLE), ("bf16", "int", False): ("i32", "pad", 48, 1, 2, LENS_SPLIT[:-1] + [1100]),
        ("bf16", "long", True): ("i64", "nhd", 16, 128, 1, short), ("bf16", "long", False): ("i64", "pad", 48, 17, 2, LENS_SPLIT[:-1] + [1100]),
        ("f16", "int", True): ("i32", "nhd", 48, 1, 2, LENS_SPLIT[:-1] + [1100]), ("f16", "int", False): ("r2t", "pad", 16, 128, 1, short),
        ("f16", "long", True): ("i64", "nhd", 64, 17, 2, LENS_SPLIT[:-1] + [1100]), ("f16", "long", False): ("i64", "pad", 48, 1, 1, LENS_SINGLE),
    }
    for (dt, _, _), (mode, lay, page, hq, S, lens) in mla.items():
        out.append(dict(dt=dt, d=DL, mode=mode, lay=lay, page=page, heads=(hq, 1), S=S, lens=lens))
    for c in out:
        c["expect"] = _expect({k: v for k, v in c.items()})[0]
    return out


INSTANCE_CASES = _instance_cases()


def test_every_mx4_decode_instance_has_a_parity_case():
    """As test_dispatch_coverage.test_every_attention_kernel_instance_has_a_parity_case, for the two 4-bit families: the
    host launch stubs of the library against the `expect` strings of INSTANCE_CASES, in both directions."""
    from sglang_amd import build

    if not os.path.exists(build.LIB_PATH):
        pytest.skip("libradix_hip.so not built")
    syms = subprocess.run(["nm", build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    mangled = sorted({ln.split()[-1] for ln in syms.splitlines() if "__device_stub__" in ln})
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
    inst = set()
    for d in dem:
        m = re.search(r"__device_stub__(\w+<.*>)\(", d)
        if m and m.group(1).split("<")[0] in FAMILIES:
            inst.add(m.group(1))
    assert len(inst) >= 24, f"only {len(inst)} 4-bit decode instances found: symbol parsing broke?"
    covered = {c["expect"] for c in INSTANCE_CASES}
    missing = sorted(inst - covered)
    assert not missing, f"{len(missing)} kernel instances without a dispatch-asserting parity case: {missing}"
    stale = sorted(covered - inst)
    assert not stale, f"cases that name instances the library does not have: {stale}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", INSTANCE_CASES, ids=[_cid(c) for c in INSTANCE_CASES])
def test_instance_is_dispatched_and_matches_the_oracle(case):
    c = {k: v for k, v in case.items() if k != "expect"}
    assert _expect(c)[0] == case["expect"]
    _decode(c)   # (asserts rx_last_dispatch() and parity)


# ----------------------------------------------------------------------------------------------------------------------
# B. targeted edges
# ----------------------------------------------------------------------------------------------------------------------
EMPTY_CASES = [dict(dt="bf16", d=128, lay="hnd", heads=(8, 2)), dict(dt="f16", d=64, lay="nhd", heads=(20, 1)),
               dict(dt="bf16", d=DL, lay="nhd", heads=(16, 1)), dict(dt="f16", d=DL, lay="pad", heads=(5, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 8], ids=["single", "split"])
@pytest.mark.parametrize("case", EMPTY_CASES, ids=[_cid(c) for c in EMPTY_CASES])
def test_empty_requests_inside_a_batch(case, S):
    """Zero-length requests between live ones.  Single pass: their rows are exactly zero (tests/test_gpu_parity.py,
    test_decode_edge_cases, states that for the 16-bit kernels).  Split-KV: whatever rx_decode_attn writes there for a 16-bit
    pool holding the same values, in the same call shape.  The neighbours match the oracle either way (_decode)."""
    from sglang_amd import ops

    c = dict(case, mode="i64", S=S, lens=[0, 33, 700, 0, 65, 1100])
    r = _decode(c)
    assert not r.live.all()
    if S == 1:
        assert np.all(r.got[~r.live] == 0)
        return
    dtype, d, (hq, hkv), bs = DT[c["dt"]], c["d"], c["heads"], len(r.lens)
    k16 = torch.from_numpy(r.kf).to(dtype).to(DEV)
    v16 = k16[..., :RANK] if d == DL else torch.from_numpy(r.vf).to(dtype).to(DEV)
    dv = v16.shape[-1]
    al = torch.zeros(bs, hq, S, dv, dtype=torch.float32, device=DEV)
    ls = torch.zeros(bs, hq, S, dtype=torch.float32, device=DEV)
    o16 = torch.full((bs, hq, dv), float("nan"), dtype=dtype, device=DEV)
    ops.decode_attention_fwd(r.q.to(DEV), k16, v16, o16, _T(r.ip), _T(r.ii), al, ls, r.splits, S, d ** -0.5, 1.0, 1.0)
    torch.cuda.synchronize()
    a, b = r.o[_T(~r.live)], o16[_T(~r.live)]
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    assert bool(same.all()), ("the empty rows of the 4-bit call and of the 16-bit call differ", a.flatten()[:4].tolist(), b.flatten()[:4].tolist())


XAI_L = 64
XAI_LENS = [1, 33, XAI_L, XAI_L + 1, XAI_L + 2, XAI_L + 3, 300, 700]   # (the factor switches on between L + 1 and L + 2)
XAI_CASES = [dict(dt="bf16", d=128, mode="i32", lay="nhd", heads=(8, 2)), dict(dt="f16", d=64, mode="r2t", lay="hnd", heads=(4, 4)),
             dict(dt="bf16", d=DL, mode="i64", lay="nhd", heads=(16, 1)), dict(dt="f16", d=DL, mode="r2t", lay="pad", heads=(5, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 8], ids=["single", "split"])
@pytest.mark.parametrize("case", XAI_CASES, ids=[_cid(c) for c in XAI_CASES])
def test_xai_temperature_len(case, S):
    _decode(dict(case, S=S, lens=XAI_LENS, kw=dict(xai=XAI_L)))


ORDER_CASES = [dict(dt="bf16", d=128, mode="i64", lay="hnd", heads=(8, 2), S=1), dict(dt="f16", d=64, mode="r2t", lay="nhd", heads=(20, 1), S=8),
               # the latent kernel ignores request_order (as the 16-bit latent kernel does): passing one changes nothing
               dict(dt="bf16", d=DL, mode="i32", lay="nhd", heads=(16, 1), S=8)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ORDER_CASES, ids=[_cid(c) for c in ORDER_CASES])
def test_request_order_changes_no_bit(case):
    c = dict(case, lens=[17, 700, 1, 300, 65, 1100, 33])
    plain, ordered = _decode(c), _decode(c, order=True)   # (each against the oracle)
    assert torch.equal(plain.o.view(torch.int16), ordered.o.view(torch.int16))


# ---- scale bytes over the whole range -------------------------------------------------------------------------------------
def _byte_range(dt):
    """the scale bytes under which all eight e2m1 magnitudes are normal numbers of the dtype (or zero)"""
    fin = torch.finfo(DT[dt])
    lo = 127 + int(round(np.log2(fin.tiny))) + 1          # 0.5 * 2^(b - 127) >= the smallest normal number
    hi = 127 + int(np.floor(np.log2(fin.max / 6.0)))      # 6 * 2^(b - 127) <= the largest finite one
    return lo, hi


def test_the_in_contract_byte_ranges():
    assert _byte_range("bf16") == (2, 252) and _byte_range("f16") == (114, 140)


def _sweep_pool(rng, dt, H, d):
    """[data, scale bytes] of ceil(n / PS) pages: block bi of (slot s, head h) carries byte number (s + 7 h + 37 bi) mod n
    of the dtype's n in-contract bytes -- every byte in every block position, neighbours 37 (mod n) apart -- and every
    block holds all sixteen nibbles in a random order"""
    lo, hi = _byte_range(dt)
    n, nb = hi - lo + 1, d // 16
    slots = -(-n // PS) * PS
    s, h, b = np.arange(slots)[:, None, None], np.arange(H)[None, :, None], np.arange(nb)[None, None, :]
    sb = (lo + (s + 7 * h + 37 * b) % n).astype(np.uint8)
    nib = rng.permuted(np.tile(np.arange(16, dtype=np.uint8), (slots, H, nb, 1)), axis=-1).reshape(slots, H, d)
    return [nib[..., 0::2] | (nib[..., 1::2] << 4), sb]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,d,lay", [("bf16", 128, "nhd"), ("f16", 64, "hnd"), ("bf16", 64, "hnd"), ("f16", 128, "nhd"),
                                      ("bf16", DL, "nhd"), ("f16", DL, "nhd")])
def test_gather_over_the_whole_scale_range_is_bit_exact(dt, d, lay):
    from sglang_amd import ops

    dtype, hnd, H = DT[dt], lay == "hnd", 1 if d == DL else 2
    rng = np.random.default_rng(d + len(dt))
    kp, vp = _sweep_pool(rng, dt, H, d), _sweep_pool(rng, dt, H, d)
    vp[1] = np.roll(vp[1], 5, axis=0)
    slots = kp[0].shape[0]
    loc = rng.permutation(slots)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    if d == DL:
        nope, rope = ops.get_mla_kv_mx4(_T(kp[0]), _T(kp[1][:, 0]), _T(loc), RANK, ROPE, dtype, err_flag=err)
        pairs = [(torch.cat([nope, rope], -1), kp)]
    else:
        bufs = [_dev(a, hnd, flat=i % 2 == 1) for i, a in enumerate((kp[0], kp[1], vp[0], vp[1]))]
        got = ops.gather_kv_mx4(bufs[0], bufs[2], bufs[1], bufs[3], _T(loc), dtype, page_size=PS, err_flag=err)
        pairs = list(zip(got, (kp, vp)))
    for out, (data, sb) in pairs:
        want = torch.from_numpy(mx4_dequant(data, sb)[loc]).to(dtype)
        assert sorted(np.unique(sb).tolist()) == list(range(_byte_range(dt)[0], _byte_range(dt)[1] + 1))
        assert torch.isfinite(want.float()).all() and tuple(out.shape) == (slots, H, d)
        bad = (out.cpu().view(torch.int16) != want.view(torch.int16)).view(slots, H, d // 16, 16).any(-1).numpy()
        assert not bad.any(), (int(bad.sum()), "blocks differ, under the scale bytes", sorted(set(sb[loc][bad].tolist()))[:8])
    assert int(err.item()) == 0


def _wide_pool(dt, ck):
    """K scale bytes 3 or 4 BELOW the centre ck in the even blocks of a row and 3 or 4 ABOVE it in the odd ones (a swapped or
    shifted byte moves a block by 2^6 or more); V scale bytes wide: bf16 100..150, fp16 the widest range symmetric about 127
    whose values are normal and at most 6 * 2^11.  Latent rows (v = the row itself): the 32 latent blocks around 123, so that
    the output keeps its size, and the four rope blocks -- K only -- around ck."""
    lo, hi = _byte_range(dt)
    r = min(127 - lo, 138 - 127) if dt == "f16" else None   # (6 * 2^(138 - 127) = 6 * 2^11)
    vlo, vhi = (100, 150) if dt == "bf16" else (127 - r, 127 + r)

    def fn(rng, slots, hkv, d, r2t, lens):
        nb = d // 16
        off = rng.integers(3, 5, (slots, hkv, nb)) * np.where(np.arange(nb) % 2, 1, -1)
        centre = np.where(np.arange(nb) < RANK // 16, 123, ck) if d == DL else ck
        ks = (centre + off).astype(np.uint8)
        assert lo <= ks.min() and ks.max() <= hi
        data = [rng.integers(0, 256, (slots, hkv, d // 2), dtype=np.uint8) for _ in range(2)]
        if d == DL:
            return [data[0], ks]
        return [data[0], ks, data[1], rng.integers(vlo, vhi + 1, (slots, hkv, nb)).astype(np.uint8)]
    return fn


WIDE_CENTRES = {"bf16": (100, 123, 146), "f16": (118, 123, 134)}   # fp16: ck - 4 >= 114 (normal), ck + 4 <= 138
WIDE_CASES = [dict(dt=dt, d=d, mode=mode, lay=lay, heads=heads, S=S, tag=f"c{ck}")
              for dt in DT for ck, (d, mode, lay, heads, S) in zip(
                  WIDE_CENTRES[dt] * 2, [(128, "i64", "hnd", (8, 2), 1), (64, "r2t", "nhd", (5, 1), 8), (DL, "i32", "nhd", (16, 1), 1),
                                         (64, "i32", "hnd", (4, 4), 1), (DL, "i64", "pad", (5, 1), 8), (128, "r2t", "nhd", (20, 1), 8)])]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_CASES, ids=[_cid(c) for c in WIDE_CASES])
def test_decode_over_wide_scale_bytes(case):
    """q carries the exact factor 2^(123 - ck) where K sits around ck: the scores keep the size of the existing cases, so the
    oracle's fp64 scores and the kernel's fp32 scores stay comparable under the unchanged bound."""
    c = dict(case, lens=[1, 17, 33, 65, 300, 700])
    ck, d = int(c["tag"][1:]), c["d"]
    qmul = np.full(d, 2.0 ** (123 - ck), dtype=np.float32)
    if d == DL:
        qmul[:RANK] = 1.0
    _decode(c, pool_fn=_wide_pool(c["dt"], ck), qmul=qmul)


# ---- the store at the ends of the range ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("dt", DT)
def test_store_at_the_top_and_bottom_of_the_range_is_bit_exact(dt, scaled):
    """Block maxima at the largest finite value, at 3.5 * 2^(emax - 1) (the first maximum whose code 6 decodes above the
    dtype's range) and a step either side of it; blocks under 6 * 2^-33 (scale byte 94; bf16 only -- fp16 has no such
    numbers but zero); k_scale 0.5 and v_scale 3.0, whose divisions land exactly on the ties.  Expected bytes: mx4_quant."""
    from sglang_amd import ops

    dtype, d, H, n, slots = DT[dt], 64, 2, 12, 2 * PS
    fin = torch.finfo(dtype)
    g = torch.Generator().manual_seed(len(dt) + scaled)
    ks, vs = (0.5, 3.0) if scaled else (1.0, 1.0)
    edge = torch.tensor([3.5 * 2.0 ** (int(np.floor(np.log2(fin.max))) - 1)]).to(dtype)   # fp16 57344, bf16 3.5 * 2^126
    tops = [_step(edge, False), edge, _step(edge, True), torch.tensor([fin.max]).to(dtype)]
    if dt == "f16":
        assert [float(t) for t in tops] == [57312.0, 57344.0, 57376.0, 65504.0]
    kv = []
    for sc in (ks, vs):
        x = torch.randn(n, H, d // 16, 16, generator=g) * torch.exp2(torch.randint(-6, 7, (n, H, d // 16, 1), generator=g).float())
        x = x.to(dtype)
        for i, top in enumerate(tops):       # row i, head i % 2: all four blocks end up with the maximum `top` after the division
            frac = (torch.rand(d // 16, 16, generator=g) * 2 - 1)
            blk = (frac * float(top) * (sc if sc == 0.5 else 1.0)).to(dtype)
            blk[:, 5] = (top.float() * (sc if sc == 0.5 else 1.0)).to(dtype) * (-1 if i % 2 else 1)
            x[i, i % 2] = blk
        for h, kk in ((0, -3), (1, 4)):      # every tie, both signs, AFTER the division by 0.5 / 3.0 (both exact)
            ties = torch.tensor(BOUNDS) * 2.0 ** kk * sc
            x[4, h, 0] = torch.cat([ties, -ties, torch.tensor([6 * 2.0 ** kk * sc, 0.0])]).to(dtype)
        x[5, 0, 1] = 0                       # an all-zero block
        if dt == "bf16":                     # under 6 * 2^-33: every tie of the grid 2^-33, and values that round to code 0
            tiny = torch.tensor(BOUNDS) * 2.0 ** -33 * (sc if sc == 0.5 else 1.0)
            x[6, 1, 2] = torch.cat([tiny, -tiny, torch.tensor([2.0 ** -36, -2.0 ** -40])]).to(dtype)
        kv.append(x.view(n, H * d))
    loc = torch.randperm(slots - 1, generator=g)[:n] + 1
    want = []
    for x, sc in zip(kv, (ks, vs)):
        data, sb = np.full((slots, H, d // 2), 0xAB, np.uint8), np.full((slots, H, d // 16), 0xAB, np.uint8)
        xq = (x / sc if sc != 1.0 else x).float().numpy().reshape(n, H, d)   # the in-place div_ rounds to the 16-bit dtype
        assert np.isfinite(xq).all()
        data[loc.numpy()], sb[loc.numpy()] = mx4_quant(xq)
        want += [data, sb]
    top_byte = 127 + int(np.floor(np.log2(fin.max))) - 1
    assert want[1][loc[1], 1, 0] == top_byte and want[1][loc[0], 0, 0] == top_byte and want[1][loc[5], 0, 1] == 94
    # element 5 of a block is the high nibble of its data byte 2: 3.5 -> code 6 (4.0, negative in row 1), a step below -> code 5 (3.0)
    assert want[0][loc[1], 1, 2] >> 4 == 8 + 6 and want[0][loc[0], 0, 2] >> 4 == 5
    if dt == "bf16":
        assert want[1][loc[6], 1, 2] == 94 and (want[0][loc[6], 1, 16] & 0x0F) == 1   # (0.25 * 2^-33: the tie goes up)
    bufs = [_dev(np.full_like(w, 0xAB), False, flat=i % 2 == 1) for i, w in enumerate(want)]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.store_cache_mx4(kv[0].to(DEV), kv[1].to(DEV), bufs[0], bufs[2], bufs[1], bufs[3], loc.to(DEV), page_size=PS,
                        k_scale=ks, v_scale=vs, err_flag=err)
    assert int(err.item()) == 0
    for name, buf, w in zip(("k data", "k scales", "v data", "v scales"), bufs, want):
        got = _canon(buf, False, w)
        assert np.array_equal(got, w), (name, int((got != w).sum()), np.argwhere(got != w)[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
def test_gather_above_the_largest_finite_value(dt):
    """A block whose maximum is >= 3.5 * 2^(emax - 1) of the dtype is stored with code 6 or 7 under scale byte emax + 126
    (fp16 141, bf16 253) and decodes to 4 or 6 times 2^(emax - 1): above the largest finite number.  The gathers return what
    the reference's dequantise gives there, the fp32 product rounded to the dtype: inf.  (No attention over such a block.)"""
    from sglang_amd import ops

    dtype, d, slots = DT[dt], 64, PS
    byte = 127 + int(np.floor(np.log2(torch.finfo(dtype).max))) - 1
    nib = np.tile(np.arange(16, dtype=np.uint8), (slots, 1, d // 16))
    data, sb = nib[..., 0::2] | (nib[..., 1::2] << 4), np.full((slots, 1, d // 16), 127, np.uint8)
    sb[3, 0, 1] = sb[9, 0, 2] = byte
    with np.errstate(over="ignore"):
        want = torch.from_numpy(mx4_dequant(data, sb)).to(dtype)
    assert int(torch.isinf(want).sum()) == 8 and bool(torch.isinf(want[3, 0, 16 + 6])) and float(want[3, 0, 16 + 5]) == 3 * 2.0 ** (byte - 127)
    loc = _T(np.arange(slots))
    k, v = ops.gather_kv_mx4(_T(data), _T(data), _T(sb.reshape(slots, -1)), _T(sb.reshape(slots, -1)), loc, dtype, page_size=PS)
    ld, ls = np.tile(data, (1, 1, DL // d)), np.tile(sb, (1, 1, DL // d))
    with np.errstate(over="ignore"):
        lwant = torch.from_numpy(mx4_dequant(ld, ls)).to(dtype)
    nope, rope = ops.get_mla_kv_mx4(_T(ld), _T(ls[:, 0]), loc, RANK, ROPE, dtype)
    for got, w in ((k, want), (v, want), (torch.cat([nope, rope], -1), lwant)):
        got = got.cpu()
        assert torch.equal(got.view(torch.int16), w.view(torch.int16)), (got[3, 0, 16:32].tolist(), w[3, 0, 16:32].tolist())


# ---- adversarial score sequences ------------------------------------------------------------------------------------------
def _pattern_pool(pattern):
    """test_gpu_adversarial_scores' ramp / falling / spikes as far as the 4-bit grid can say them: the K scale bytes of a
    token follow its position in the request (rising 119 -> 130 as the existing latent case, falling 130 -> 119, or flat 121
    with a spike every 300 tokens, each a byte higher than the last): the running maximum is overtaken again and again, never
    again after the start, or in a few huge jumps."""
    def fn(rng, slots, hkv, d, r2t, lens):
        pool = _default_pool(rng, slots, hkv, d, r2t, lens)
        for i, n in enumerate(lens):
            n, pos = int(n), np.arange(int(n))
            if pattern == "rising":
                b = 119 + pos * 12 // n
            elif pattern == "falling":
                b = 130 - pos * 12 // n
            else:
                b = np.full(n, 121)
                for j, p in enumerate(range(50, n, 300)):
                    b[p] = 128 + j
            pool[1][r2t[i + 1, :n]] = b.astype(np.uint8)[:, None, None]
        return pool
    return fn


ADVERSARIAL_CASES = [dict(dt=dt, d=128, mode=("i64", "r2t")[S > 1], lay=("hnd", "nhd")[dt == "f16"], heads=(8, 2), S=S, tag=p)
                     for dt in DT for S in (1, 8) for p in ("rising", "falling", "spikes")]
ADVERSARIAL_CASES += [dict(dt="f16", d=DL, mode="i64", lay="pad", heads=(16, 1), S=8, tag=p) for p in ("rising", "falling", "spikes")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ADVERSARIAL_CASES, ids=[_cid(c) for c in ADVERSARIAL_CASES])
def test_decode_under_adversarial_scores(case):
    _decode(dict(case, lens=[65, 700, 1100]), pool_fn=_pattern_pool(case["tag"]))   # (no NaN, then parity)
