"""Attention kernels on strided (non-contiguous) operands: the layout x kernel-family matrix.

Every entry point copies element strides from its tensors (ops._extend_params, _fill_decode_common, _set_new_kv, _set_rope,
the pools' separate K / V page, token and head strides) and the kernels do their own address arithmetic with them; the rest
of the suite runs them at stride_t == H * D, stride_h == D, K strides == V strides almost everywhere.  Here each family runs
next to its contiguous call L0, on the same values, under

  L1  q / k / v as views of ONE fused [T, (Hq + 2 Hkv) D] projection (the production layout; Dk == Dv), o contiguous
  L2  every operand carved into its own NaN-poisoned (inputs) / sentinel-filled (outputs) backing buffer, pads and offsets
      multiples of 8 elements and different for q, k, v, o; lse padded in both dims
  L3  k contiguous and v a wide view ("L3"), and the reverse ("L3r"): a K / V offset shared by mistake is wrong either way
  L4  q and o head-major ([H, T, D].transpose(0, 1): stride_h > stride_t)
  L5  pools with unequal K / V strides (V padded, K plain: "L5"; the reverse: "L5r"), NHD page 1 / NHD page 16 / HND pages
  L6  below the fast paths' alignment: offset 4 and pad_t 4 elements on q / k / v ("L6"), or on o only ("L6o")

and is held to (1) parity_util.check_out against the fp64 oracle on the LOGICAL values with the family's usual arguments,
(2) the same rx_last_dispatch() string as L0, (3) with the same kernel, bit-identical o / lse (same arithmetic: any
difference is a different element read), (4) strided_util.gaps_untouched on every carved operand, inputs included, (5) fused
stores: the pool row at the page table's slot holds the new row's bits.  Where a launcher declines a layout (another, named
kernel runs it: 1 and 4 hold) or refuses it (RuntimeError naming strides / alignment), EXPECT below says so per case.
The oracle's output is asserted finite before anything is launched: NaN poison is sound only then.
Below the matrix: VerifySplitKV's short extends, the fused-RoPE latent decode, the 4-bit pools' decode, and the quantising
stores / get_mla_kv / rope_store_kv with strided source rows, and HipRadixAttnBackend end to end on fused-qkv views."""
import re
import zlib

import numpy as np
import pytest
import torch

import parity_util as parity
import strided_util as su
from oracle import radix_oracle as orc

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
EXT, PRE = [1, 40, 129, 257], [0, 70, 200, 33]          # (the dispatch matrix's seams: one row, multi-block, long extends)
LENS = [1, 31, 33, 257, 900, 2100]
PS = 16
LSE_TOL = dict(atol=3e-3, rtol=1e-3)                     # lse as in test_gpu_random / test_gpu_parity


def _bits(t):
    if t.dtype == torch.bfloat16:
        return t.detach().cpu().contiguous().view(torch.uint16).numpy()
    return t.detach().cpu().contiguous().numpy()


def _seed(c):
    return zlib.crc32(c["id"].encode())


# ----------------------------------------------------------------------------------------------------------------------
# the cases: one per family (and flavour), bf16 everywhere, fp16 on at least one case per family
# ----------------------------------------------------------------------------------------------------------------------
def _e(id, fam, dk, dv=None, hq=4, hkv=2, dt="bf16", idx="long", pool="nhd1", opts=None, kw=None, **x):
    return dict(id=id, kind="extend", fam=fam, dk=dk, dv=dk if dv is None else dv, hq=hq, hkv=hkv, dt=dt, idx=idx, pool=pool,
                opts=opts or {}, kw=kw or {}, **x)


PACK = {"ext32_pack_min_wgs": 0, "ext32_pack_min_tiles": 0}
EXTEND_CASES = [
    _e("e32-plain-nw4", "extend_mfma32_kernel", 128, plain=True, hq=4, hkv=4, opts={"ext32_small_wg": 1}),
    _e("e32-plain-nw8-f16", "extend_mfma32_kernel", 128, plain=True, hq=4, hkv=2, dt="f16", idx="int", pool="hnd", opts={"ext32_small_wg": 0}, hint=4096),
    _e("e32-cap-nw4", "extend_mfma32_kernel", 128, hq=8, hkv=2, pool="hnd", opts={"ext32_small_wg": 1, "ext32_autopack": 0}, kw={"logit_cap": 30.0}),
    _e("e32-cap-nw8-f16", "extend_mfma32_kernel", 128, hq=4, hkv=4, dt="f16", opts={"ext32_small_wg": 0, "ext32_autopack": 0}, kw={"logit_cap": 30.0}, hint=4096),
    _e("e32-fp8-nw4", "extend_mfma32_kernel", 128, hq=8, hkv=1, opts={"ext32_small_wg": 1, "ext32_autopack": 0}, fp8=True, kw={"k_scale": 0.9, "v_scale": 1.25}),
    _e("e32-fp8-nw8-f16", "extend_mfma32_kernel", 128, hq=4, hkv=2, dt="f16", pool="hnd", opts={"ext32_small_wg": 0, "ext32_autopack": 0}, fp8=True, kw={"k_scale": 0.9}, hint=4096),
    _e("e32-cap-nw4-nhd16-f16", "extend_mfma32_kernel", 128, hq=4, hkv=2, dt="f16", pool="nhd16", opts={"ext32_small_wg": 1, "ext32_autopack": 0}, kw={"logit_cap": 30.0}),
    _e("e32-plain-nw4-nhd16", "extend_mfma32_kernel", 128, plain=True, hq=4, hkv=2, pool="nhd16", opts={"ext32_small_wg": 1}),
    _e("e32-plain-nw4-hnd", "extend_mfma32_kernel", 128, plain=True, hq=4, hkv=2, pool="hnd", opts={"ext32_small_wg": 1}),
    _e("e32-pkc4-nw8", "extend_mfma32_kernel", 128, plain=True, hq=8, hkv=2, opts=dict(PACK, ext32_small_wg=0), hint=4096),
    _e("e32-pkc4-nw4-f16", "extend_mfma32_kernel", 128, plain=True, hq=8, hkv=2, dt="f16", pool="hnd", opts=dict(PACK, ext32_small_wg=1)),
    _e("e32-pkc8-nw8-f16", "extend_mfma32_kernel", 128, plain=True, hq=8, hkv=1, dt="f16", idx="int", opts=dict(PACK, ext32_small_wg=0), hint=4096),
    _e("e32-pkc8-nw4", "extend_mfma32_kernel", 128, plain=True, hq=8, hkv=1, pool="nhd16", opts=dict(PACK, ext32_small_wg=1)),
    _e("e32-uni-nw4", "extend_mfma32_uni_kernel", 128, hq=4, hkv=2, opts={"ext32_small_wg": 1}, unified=True),
    _e("e32-uni-nw4-nhd16", "extend_mfma32_uni_kernel", 128, hq=4, hkv=2, pool="nhd16", opts={"ext32_small_wg": 1}, unified=True),
    _e("e32-uni-nw8-f16", "extend_mfma32_uni_kernel", 128, hq=8, hkv=2, dt="f16", pool="hnd", opts={"ext32_small_wg": 0}, unified=True),
    _e("mfma-d64", "extend_mfma_kernel", 64, hq=4, hkv=2, opts={"extend_d256_at64": 0}),
    _e("mfma-d64-f16", "extend_mfma_kernel", 64, hq=8, hkv=1, dt="f16", idx="int", pool="hnd", opts={"extend_d256_at64": 0}),
    _e("mfma-d128", "extend_mfma_kernel", 128, hq=4, hkv=2, pool="nhd16", opts={"extend_16x16_d128": 1}),
    _e("mfma-d128-f16", "extend_mfma_kernel", 128, hq=4, hkv=4, dt="f16", opts={"extend_16x16_d128": 1}),
    _e("generic-d80", "extend_generic_kernel", 80, hq=4, hkv=2, pool="hnd"),
    _e("generic-d80-f16", "extend_generic_kernel", 80, hq=4, hkv=4, dt="f16", idx="int"),
    _e("generic-d256-tree", "extend_generic_kernel", 256, hq=4, hkv=2, mask=True),
    _e("generic-d256-tree-f16", "extend_generic_kernel", 256, hq=4, hkv=4, dt="f16", pool="hnd", mask=True),
    _e("d256-256-g1", "extend_d256_kernel", 256, hq=2, hkv=2),
    _e("d256-256-g4-f16", "extend_d256_kernel", 256, hq=8, hkv=2, dt="f16", pool="hnd"),
    _e("d256-192x128-g1-f16", "extend_d256_kernel", 192, 128, hq=2, hkv=2, dt="f16", idx="int"),
    _e("d256-192x128-g8", "extend_d256_kernel", 192, 128, hq=8, hkv=1, pool="nhd16"),
    _e("d256-96-g1", "extend_d256_kernel", 96, hq=2, hkv=2, pool="hnd"),
    _e("d256-96-g4-f16", "extend_d256_kernel", 96, hq=8, hkv=2, dt="f16"),
    _e("d256-64-g1-f16", "extend_d256_kernel", 64, hq=2, hkv=2, dt="f16"),
    _e("d256-64-g16", "extend_d256_kernel", 64, hq=16, hkv=1, pool="hnd"),
    _e("nd-192x128", "extend_nd_kernel", 192, 128, hq=4, hkv=2, opts={"extend_d256": 0, "extend_d256_at96": 0}),
    _e("nd-256-f16", "extend_nd_kernel", 256, hq=4, hkv=1, dt="f16", pool="hnd", opts={"extend_d256": 0, "extend_d256_at96": 0}),
    _e("mla-aliased", "extend_mla_kernel", 576, 512, hq=16, hkv=1, mla=True, own_v=False),
    _e("mla-own-v-f16", "extend_mla_kernel", 576, 512, hq=5, hkv=1, dt="f16", pool="hnd", mla=True, own_v=True),
    _e("bias-d128", "extend_mfma32_kernel", 128, hq=4, hkv=2, opts={"ext32_autopack": 0}, bias=True),
    _e("bias-d128-f16", "extend_mfma32_kernel", 128, hq=4, hkv=4, dt="f16", pool="hnd", opts={"ext32_autopack": 0}, bias=True),
]
for _c in EXTEND_CASES:
    _c.setdefault("ext", [9, 40, 33] if _c["fam"] == "extend_generic_kernel" else EXT)   # (one scalar workgroup per (token, head))
    _c.setdefault("pre", [0, 70, 33] if _c["fam"] == "extend_generic_kernel" else PRE)


def _d(id, fam, dk, dv=None, hq=4, hkv=2, dt="bf16", mode="indices", pool="nhd1", opts=None, **x):
    return dict(id=id, kind="decode", fam=fam, dk=dk, dv=dk if dv is None else dv, hq=hq, hkv=hkv, dt=dt, mode=mode, pool=pool,
                opts=opts or {}, **x)


DECODE_CASES = [
    _d("dec-d64", "decode_mfma_kernel", 64, hq=4, hkv=2, mode="r2t"),
    _d("dec-d96-f16", "decode_mfma_kernel", 96, hq=8, hkv=2, dt="f16", pool="hnd"),
    _d("dec-d128", "decode_mfma_kernel", 128, hq=8, hkv=1, pool="nhd16", mode="r2t"),
    _d("dec-d128-f16", "decode_mfma_kernel", 128, hq=4, hkv=4, dt="f16", idx32=True),
    _d("dec-d128-hnd", "decode_mfma_kernel", 128, hq=8, hkv=2, pool="hnd"),
    _d("dec-d256", "decode_mfma_kernel", 256, hq=4, hkv=2, pool="hnd"),
    _d("dec-d128-kv8", "decode_mfma_kernel", 128, hq=8, hkv=2, fp8=True),
    _d("dec-d64-kv8-f16", "decode_mfma_kernel", 64, hq=4, hkv=2, dt="f16", fp8=True, pool="hnd", mode="r2t"),
    _d("dec-d128-fuse", "decode_mfma_kernel", 128, hq=8, hkv=2, fuse=True, mode="r2t"),
    _d("dec-d64-fuse-f16", "decode_mfma_kernel", 64, hq=4, hkv=4, dt="f16", fuse=True, pool="hnd"),
    _d("dec-d128-occ3", "decode_mfma_kernel", 128, hq=4, hkv=2, occ3=True, items=True),
    _d("dec-d128-items-f16", "decode_mfma_kernel", 128, hq=8, hkv=2, dt="f16", items=True, pool="hnd", mode="r2t"),
    _d("dec-d128-units", "decode_mfma_kernel", 128, hq=8, hkv=2, items=True, units=True, mode="r2t"),
    _d("dec-bias-d128", "decode_mfma_bias_kernel", 128, hq=4, hkv=2, bias=True),
    _d("dec-bias-d64-f16", "decode_mfma_bias_kernel", 64, hq=8, hkv=2, dt="f16", bias=True, pool="hnd", mode="r2t"),
    _d("dec-generic-d80", "decode_generic_kernel", 80, hq=4, hkv=2, pool="hnd"),
    _d("dec-generic-d80-f16", "decode_generic_kernel", 80, hq=4, hkv=4, dt="f16", idx32=True),
    _d("mla-rows16", "decode_mla_kernel", 576, 512, hq=16, hkv=1, mla=True),
    _d("mla-rows16-f16", "decode_mla_kernel", 576, 512, hq=5, hkv=1, dt="f16", mla=True, pool="hnd", mode="r2t"),
    _d("mla-fp8-staged", "decode_mla_kernel", 576, 512, hq=16, hkv=1, mla=True, fp8=True, opts={"decode_mla8_dma": 0}),
    _d("mla-fp8-dma-f16", "decode_mla8_dma_kernel", 576, 512, hq=16, hkv=1, dt="f16", mla=True, fp8=True, opts={"decode_mla8_t64": 0}, pool="hnd"),
    _d("mla-fp8-dma", "decode_mla8_dma_kernel", 576, 512, hq=16, hkv=1, mla=True, fp8=True, opts={"decode_mla8_t64": 0}, pool="nhd16", mode="r2t"),
    _d("mla-fp8-t64-f16", "decode_mla8_t64_kernel", 576, 512, hq=16, hkv=1, dt="f16", mla=True, fp8=True, opts={"decode_mla8_t64": 1}, pool="hnd"),
    _d("mla-rows16-nhd16", "decode_mla_kernel", 576, 512, hq=16, hkv=1, mla=True, pool="nhd16"),
    _d("mla-fp8-t64", "decode_mla8_t64_kernel", 576, 512, hq=128, hkv=1, mla=True, fp8=True, opts={"decode_mla8_t64": 1}, mode="r2t"),
]

# What is NOT "same kernel as L0, bit-identical" today, per family and layout.  "declined": the launcher falls through to
# another kernel (the regex must match its dispatch string) and assertions 1 and 4 hold on it; "refused": RuntimeError
# whose message names strides or alignment (regex).
#   extend, D = 128 32x32x16 PLAIN instances (packed or not): ONE row offset serves the K and the V load, so unequal K / V
#     strides (L2, L3, L3r, L5, L5r) go to the general instance <.., PLAIN = false, PKC = 0>; L1 (equal strides) runs natively
#   extend, unified instance: the same for unequal pool strides (L5, L5r) -> the general 32x32x16 instance
#   extend, D = 128 with an o that is only 8-byte aligned (L6o): extend_mfma_kernel<.., 128, ..>; refused where only the
#     32x32x16 kernel can do the job (fp8 prefix, score bias, unified)
#   extend / decode, D in {64, 128} (decode also 96, 256) with q / k / v strides that are no multiples of 8 (L6): refused
#   extend, the other head dims (AGPR template, 16x16x32 nd kernel, latent MLA) under L6: extend_generic_kernel
#   decode, latent rows under L6: decode_generic_kernel (16-bit pool); refused on an fp8 pool (no other kernel reads it)
def _expect(c, layout):
    fam, d128 = c["fam"], c["dk"] == 128 and c["dv"] == 128
    if c["kind"] == "extend":
        vec = c["dk"] == c["dv"] and c["dk"] in (64, 128)
        if layout == "L6" and fam != "extend_generic_kernel":
            return ("refused", "strides must be multiples of 8") if vec else ("declined", r"^extend_generic_kernel<")
        if layout == "L6o" and d128 and fam in ("extend_mfma32_kernel", "extend_mfma32_uni_kernel"):
            if c.get("fp8") or c.get("bias") or c.get("unified"):
                return ("refused", "o must be 16-byte aligned with strides that are multiples of 8")
            return ("declined", r"^extend_mfma_kernel<rx::\w+, 128, ")
        if c.get("plain") and layout in ("L2", "L3", "L3r", "L5", "L5r"):
            return ("declined", r"^extend_mfma32_kernel<.*, false, 0>$")
        if c.get("unified") and layout in ("L5", "L5r"):
            return ("declined", r"^extend_mfma32_kernel<.*, false, false, 0>$")
    elif layout == "L6":
        if c["dk"] == c["dv"] and c["dk"] in (64, 96, 128, 256):
            return ("refused", "strides must be multiples of 8")
        if c.get("mla"):
            return ("refused", "strides that are multiples of 8 elements, 16-byte aligned") if c.get("fp8") else ("declined", r"^decode_generic_kernel<")
    return ("same", None)


# ----------------------------------------------------------------------------------------------------------------------
# logical data + oracle, once per case
# ----------------------------------------------------------------------------------------------------------------------
_DATA = {}


def _page_table(rng, counts, extra=3):
    pages = [-(-int(n) // PS) for n in counts]
    n_pages = sum(pages) + extra
    ids = rng.permutation(np.arange(1, n_pages))
    rows, pi = [], 0
    for n, npg in zip(counts, pages):
        rows.append((ids[pi: pi + npg, None] * PS + np.arange(PS)[None]).reshape(-1)[: int(n)])
        pi += npg
    return n_pages, rows


def extend_data(c):
    if c["id"] in _DATA:
        return _DATA[c["id"]]
    dtype = DT[c["dt"]]
    hq, hkv, dk, dv = c["hq"], c["hkv"], c["dk"], c["dv"]
    pre, ext = np.asarray(c["pre"], np.int64), np.asarray(c["ext"], np.int64)
    T = int(ext.sum())
    rng = np.random.default_rng(_seed(c))
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    uni = c.get("unified", False)
    n_pages, rows = _page_table(rng, pre + ext if uni else pre)
    kvi = np.concatenate(rows).astype(np.int64)
    kvp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    pool = n_pages * PS
    fp8 = c.get("fp8", False)
    pdt = torch.float8_e4m3fn if fp8 else dtype
    kb = torch.randn(pool, hkv, dk, generator=g).to(pdt)
    vb = kb[..., :dv] if c.get("mla") else torch.randn(pool, hkv, dv, generator=g).to(pdt)
    ke = torch.randn(T, hkv, dk, generator=g).to(dtype)
    ve = torch.randn(T, hkv, dv, generator=g).to(dtype) if (not c.get("mla") or c["own_v"]) else ke[..., :dv]
    q = torch.randn(T, hq, dk, generator=g).to(dtype)
    qo = np.concatenate([[0], np.cumsum(ext)]).astype(np.int64)
    kw = dict(c["kw"])
    ks, vs = kw.pop("k_scale", 1.0), kw.pop("v_scale", 1.0)
    sm = (192 if c.get("mla") else dk) ** -0.5
    dec = (lambda t: orc.fp8_e4m3fn_decode(t.contiguous().view(torch.uint8).numpy())) if fp8 else (lambda t: _bits(t))
    okw = dict(kw, k_scale=ks, v_scale=vs)
    aux = mask = mip = None
    if c.get("bias"):
        aux = (1.5 * torch.randn(T, hq, 150, generator=g)).to(torch.float32 if c["dt"] == "bf16" else dtype)
        okw["score_bias"] = aux.double().numpy()
    if c.get("mask"):  # a speculative tree mask over the new tokens (prefix columns are skipped: skip_prefix_custom_mask)
        segs = []
        for p_, e_ in zip(pre, ext):
            m = rng.integers(0, 2, size=(int(e_), int(p_ + e_))).astype(np.uint8)
            m[np.arange(int(e_)), int(p_) + np.arange(int(e_))] = 1
            segs.append(m.reshape(-1))
        mip = np.concatenate([[0], np.cumsum([s.size for s in segs])]).astype(np.int64)
        mask = np.concatenate(segs)
        okw.update(custom_mask=mask, mask_indptr=mip)
    if uni:
        want, absw = orc.extend_attention_unified(_bits(q), dec(kb), dec(vb), qo, kvp, kvi, pre, sm_scale=sm, return_absw=True)
        lse = None
    else:
        want, lse, absw = orc.extend_attention(_bits(q), _bits(ke), _bits(ve), dec(kb), dec(vb), qo, kvp, kvi, is_causal=True,
                                               sm_scale=sm, return_lse=True, return_absw=True, **okw)
    d = dict(q=q, ke=ke, ve=ve, kb=kb, vb=vb, qo=qo, kvp=kvp, kvi=kvi, pre=pre, ext=ext, T=T, n_pages=n_pages, sm=sm, ks=ks, vs=vs,
             kw=kw, aux=aux, mask=mask, mip=mip, want=want, absw=absw, lse=lse, dtype=dtype)
    _DATA[c["id"]] = d
    return d


def decode_data(c):
    if c["id"] in _DATA:
        return _DATA[c["id"]]
    dtype = DT[c["dt"]]
    hq, hkv, dk, dv = c["hq"], c["hkv"], c["dk"], c["dv"]
    lens = np.asarray(LENS, np.int64)
    bs = len(lens)
    rng = np.random.default_rng(_seed(c))
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    n_pages, rows = _page_table(rng, lens)
    r2t = np.zeros((bs + 1, int(lens.max()) + PS), dtype=np.int32)
    for i, r in enumerate(rows):
        r2t[i + 1, : len(r)] = r
    pool = n_pages * PS
    fp8 = c.get("fp8", False)
    pdt = torch.float8_e4m3fn if fp8 else dtype
    kb = torch.randn(pool, hkv, dk, generator=g).to(pdt)
    vb = kb[..., :dv] if c.get("mla") else torch.randn(pool, hkv, dv, generator=g).to(pdt)
    q = torch.randn(bs, hq, dk, generator=g).to(dtype)
    rpi = np.arange(1, bs + 1, dtype=np.int64)
    ip, ii = orc.build_kv_indices(r2t, rpi, lens)
    kn = vn = last = None
    kb_dev, vb_dev = kb, vb
    if c.get("fuse"):  # the step's rows are stored by the launch: the pool given to it holds 7 / -7 there
        kn = torch.randn(bs, hkv, dk, generator=g).to(dtype)
        vn = torch.randn(bs, hkv, dv, generator=g).to(dtype)
        last = torch.from_numpy(r2t[rpi, lens - 1].astype(np.int64))
        kb_dev, vb_dev = kb.clone(), vb.clone()
        kb_dev[last], vb_dev[last] = 7.0, -7.0
        kb[last], vb[last] = kn, vn
    dec = (lambda t: orc.fp8_e4m3fn_decode(t.contiguous().view(torch.uint8).numpy())) if fp8 else (lambda t: _bits(t))
    ks, vs = (0.8, 1.25) if (fp8 and not c.get("mla")) else (1.0, 1.0)
    aux = (1.5 * torch.randn(bs, hq, 70, generator=g)).to(torch.float32 if c["dt"] == "bf16" else dtype) if c.get("bias") else None
    sm = (192 if c.get("mla") else dk) ** -0.5
    want, absw = orc.decode_attention(_bits(q), dec(kb), dec(vb), ip, ii, sm, k_scale=ks, v_scale=vs,
                                      score_bias=None if aux is None else aux.double().numpy(), return_absw=True)
    d = dict(q=q, kb=kb_dev, vb=vb_dev, kn=kn, vn=vn, last=last, r2t=r2t, rpi=rpi, lens=lens, ip=ip, ii=ii, n_pages=n_pages, sm=sm,
             ks=ks, vs=vs, aux=aux, want=want, absw=absw, dtype=dtype)
    _DATA[c["id"]] = d
    return d


# ----------------------------------------------------------------------------------------------------------------------
# layouts
# ----------------------------------------------------------------------------------------------------------------------
class Placed:
    """Device operands of one call and the carved ones among them with the fill their gaps must still hold."""

    def __init__(self):
        self.carved = []

    def inp(self, name, t, pad_t=0, pad_h=0, offset=0, tail=0):
        v = su.carve(t.to(DEV), pad_t, pad_h, offset, su.nan_bits(t.dtype), tail)
        self.carved.append((name, v, su.nan_bits(t.dtype)))
        return v

    def inp_strided(self, name, t, strides, offset=0, tail=0):
        v = su.carve_strided(t.to(DEV), strides, offset, su.nan_bits(t.dtype), tail)
        self.carved.append((name, v, su.nan_bits(t.dtype)))
        return v

    def out(self, name, shape, dtype, pad_t=0, pad_h=0, offset=0):
        v = su.carve(torch.full(shape, float("nan"), dtype=dtype, device=DEV), pad_t, pad_h, offset, su.sentinel_bits(dtype))
        self.carved.append((name, v, su.sentinel_bits(dtype)))
        return v

    def check_gaps(self, tag):
        for name, v, fill in self.carved:
            assert su.gaps_untouched(v, fill), (tag, f"elements outside the logical rows of `{name}` were written")


def _fused_qkv(q, k, v):
    """q, k, v [T, H*, D] as views of one [T, (Hq + 2 Hkv) D] buffer (no gaps: every element is an operand's)."""
    T, hq, d = q.shape
    hkv = k.shape[1]
    buf = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], dim=1).to(DEV)
    qv, kv, vv = buf.split([hq * d, hkv * d, hkv * d], dim=1)
    return qv.view(T, hq, d), kv.view(T, hkv, d), vv.view(T, hkv, d)


def _wide(P, name, t, other_cols, tail):
    """`t` as the middle columns of a wide poisoned row (what a view of a fused projection looks like to the kernel)."""
    T, h, d = t.shape
    return P.inp_strided(name, t, (h * d + other_cols, d, 1), offset=other_cols // 2 // 8 * 8, tail=tail)


def place_qkvo(P, layout, q, k, v, o_shape, dtype, lse_shape=None, slack=0):
    """q, k, v inputs ([T, H, D] logical CPU tensors; k / v may be None) and the o / lse outputs under `layout`.  `slack`: fill
    elements behind every carved input, so that a kernel that walked one operand with another's stride stays inside it."""
    T, hq, dq = q.shape
    alias = v is not None and k is not None and v.data_ptr() == k.data_ptr()   # (latent rows: v = k[..., :512])
    dv = o_shape[-1]
    lse = None
    cont_o = lambda: torch.full(o_shape, float("nan"), dtype=dtype, device=DEV)   # noqa: E731
    if layout == "L0":
        qd, kd, vd, od = q.to(DEV), None if k is None else k.to(DEV), None, cont_o()
        if v is not None:
            vd = kd[..., :dv] if alias else v.to(DEV)
        if lse_shape:
            lse = torch.full(lse_shape, float("nan"), dtype=torch.float32, device=DEV)
        return qd, kd, vd, od, lse
    if layout == "L1":
        assert k is not None and not alias and k.shape == v.shape and k.shape[2] == dq
        qd, kd, vd = _fused_qkv(q, k, v)
        od = cont_o()
    elif layout == "L2":
        qd = P.inp("q", q, 8, 8, 8, slack)
        kd = None if k is None else P.inp("k", k, 16, 8, 16, slack)
        vd = None if v is None else (kd[..., :dv] if alias else P.inp("v", v, 24, 16, 8, slack))
        od = P.out("o", o_shape, dtype, 8, 16, 24)
    elif layout in ("L3", "L3r"):
        assert k is not None and not alias
        qd, od = q.to(DEV), cont_o()
        wide = (hq + k.shape[1]) * dq
        if layout == "L3":
            kd, vd = P.inp("k", k, tail=slack), _wide(P, "v", v, wide, slack)
        else:
            kd, vd = _wide(P, "k", k, wide, slack), P.inp("v", v, tail=slack)
    elif layout == "L4":
        qd = P.inp_strided("q", q, (dq, T * dq, 1), tail=slack)
        od = su.carve_strided(torch.full(o_shape, float("nan"), dtype=dtype, device=DEV), (dv, T * dv, 1), 0, su.sentinel_bits(dtype))
        P.carved.append(("o", od, su.sentinel_bits(dtype)))
        kd = None if k is None else k.to(DEV)
        vd = None if v is None else (kd[..., :dv] if alias else v.to(DEV))
    elif layout == "L6":
        qd = P.inp("q", q, 4, 0, 4, slack)
        kd = None if k is None else P.inp("k", k, 4, 0, 4, slack)
        vd = None if v is None else (kd[..., :dv] if alias else P.inp("v", v, 4, 0, 4, slack))
        od = cont_o()
    elif layout == "L6o":
        qd, kd = q.to(DEV), None if k is None else k.to(DEV)
        vd = None if v is None else (kd[..., :dv] if alias else v.to(DEV))
        od = P.out("o", o_shape, dtype, 4, 0, 4)
    else:
        raise ValueError(layout)
    if lse_shape:
        if layout == "L2":
            lse = su.carve(torch.full(lse_shape, float("nan"), dtype=torch.float32, device=DEV), 8, 8, 8, su.sentinel_bits(torch.float32))
            P.carved.append(("lse", lse, su.sentinel_bits(torch.float32)))
        else:
            lse = torch.full(lse_shape, float("nan"), dtype=torch.float32, device=DEV)
    return qd, kd, vd, od, lse


def place_new_kv(P, layout, k, v, slack):
    """The decode step's k_new / v_new [bs, Hkv, D] under `layout` (the k / v part of place_qkvo)."""
    if layout == "L2":
        return P.inp("k_new", k, 16, 8, 16, slack), P.inp("v_new", v, 24, 16, 8, slack)
    if layout in ("L3", "L3r"):
        wide = 3 * k.shape[1] * k.shape[2]
        if layout == "L3":
            return P.inp("k_new", k, tail=slack), _wide(P, "v_new", v, wide, slack)
        return _wide(P, "k_new", k, wide, slack), P.inp("v_new", v, tail=slack)
    if layout == "L6":
        return P.inp("k_new", k, 4, 0, 4, slack), P.inp("v_new", v, 4, 0, 4, slack)
    return k.to(DEV), v.to(DEV)


def place_pool(P, ops, kind, kb, vb, variant="sym", mla=False):
    """Canonical pools [slots, H, D] on the device as `kind`: "nhd1" (slot-major rows, page 1), "nhd16" ([pages, 16, H, D] with a
    padded page), "hnd" ([pages, H, 16 + pad tokens, D]).  variant "sym": K and V alike (what the rest of the suite does);
    "v" / "k": that pool also has a per-token pad and another page pad, the other one is as in "sym".  Gaps are poisoned.
    Returns k, v, page_size, layout, rows(): the K rows back as [slots, H, D]."""
    slots, h, dk = kb.shape
    dv = vb.shape[2]
    pages = slots // PS
    tail = 2 * slots * h * max(dk, dv)

    def one(name, t, odd):
        d = t.shape[2]
        if kind == "nhd1":
            return P.inp(name, t, 16 if odd else 0, 0, 8 if odd else 0, tail)
        if kind == "nhd16":
            tok = h * d + (8 if odd else 0)
            return P.inp_strided(name, t.view(pages, PS, h, d), (PS * tok + (64 if odd else 32), tok, d, 1), 0, tail)
        padtok = 4 if odd else 2
        t4 = t.view(pages, PS, h, d).permute(0, 2, 1, 3)
        return P.inp_strided(name, t4, (h * (PS + padtok) * d + (24 if odd else 0), (PS + padtok) * d, d, 1), 0, tail)

    kd = one("k_pool", kb, variant == "k" or (mla and variant != "sym"))   # (latent rows: ONE pool, padded or not)
    vd = kd[..., :dv] if mla else one("v_pool", vb, variant == "v")
    if kind == "nhd1":
        return kd, vd, 1, None, lambda: kd
    if kind == "nhd16":
        return kd, vd, PS, None, lambda: kd.reshape(slots, h, dk)
    return kd, vd, PS, ops.kv_layout_hnd(kd, vd), lambda: kd.permute(0, 2, 1, 3).reshape(slots, h, dk)


def _slack(c, rows):
    return rows * (c["hq"] + 2 * c["hkv"]) * (max(c["dk"], c["dv"]) + 16) + 64


class _Options:
    def __init__(self, rxlib, opts):
        self.cms = [rxlib.option(k, v) for k, v in opts.items()]

    def __enter__(self):
        for cm in self.cms:
            cm.__enter__()

    def __exit__(self, *a):
        for cm in reversed(self.cms):
            cm.__exit__(None, None, None)


# ----------------------------------------------------------------------------------------------------------------------
# extend
# ----------------------------------------------------------------------------------------------------------------------
def run_extend(c, layout, ops, rxlib):
    """One call under `layout`: (o [T, Hq, Dv] logical, lse or None, dispatch string, Placed)."""
    d = extend_data(c)
    assert np.isfinite(d["want"]).all() and (d["lse"] is None or np.isfinite(d["lse"]).all())   # NaN poison is sound only then
    P = Placed()
    uni = c.get("unified", False)
    T, hq, dv = d["T"], c["hq"], c["dv"]
    qkv_layout = "L0" if layout.startswith("L5") else layout
    q, k, v, o, lse = place_qkvo(P, qkv_layout, d["q"], None if uni else d["ke"], None if uni else d["ve"], (T, hq, dv), d["dtype"],
                                 None if uni else (T, hq), slack=_slack(c, T))
    variant = {"L5": "v", "L5r": "k"}.get(layout, "sym")
    kd, vd, page, lay, _ = place_pool(P, ops, c["pool"], d["kb"], d["vb"], variant, mla=c.get("mla", False))
    idt = torch.int32 if c["idx"] == "int" else torch.int64
    Tn = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    kw = dict(d["kw"])
    if d["aux"] is not None:
        kw.update(score_mod=ops.relative_bias_score_mod, aux_tensors=[d["aux"].to(DEV)])
    with _Options(rxlib, c["opts"]):
        if uni:
            ops.extend_attention_fwd_unified(q, o, kd, vd, 1.0, 1.0, Tn(d["qo"]), Tn(d["kvp"]), Tn(d["kvi"]).to(idt),
                                             Tn(d["pre"].astype(np.int32)), int(d["ext"].max()), sm_scale=d["sm"], is_causal=True,
                                             page_size=page, kv_layout=lay)
        else:
            ops.extend_attention_fwd(q, k, v, o, kd, vd, Tn(d["qo"]), Tn(d["kvp"]), Tn(d["kvi"]).to(idt),
                                     None if d["mask"] is None else Tn(d["mask"]), True, None if d["mip"] is None else Tn(d["mip"]),
                                     int(d["ext"].max()), d["ks"], d["vs"], sm_scale=d["sm"], page_size=page, kv_layout=lay,
                                     lse_extend=lse, avg_kv_len_hint=c.get("hint"), **kw)
        torch.cuda.synchronize()
        name = rxlib.last_dispatch()
    return o, lse, name, P


_L0 = {}


def check_against_l0(c, layout, run, want, absw, lse_want, ops, rxlib, key=None):
    """Assertions 1-4 (and the declined / refused outcomes of EXPECT) of `layout` next to L0."""
    from sglang_amd.lib import RadixHipError

    key = key or c["id"]
    d_dtype = DT[c["dt"]]
    if key not in _L0:   # the contiguous call, once per (case, form): its output is only read afterwards
        o0, lse0, name0, _ = run(c, "L0", ops, rxlib)
        assert name0.startswith(c["fam"] + "<"), (c["id"], "L0 did not reach the family", name0)
        parity.check_out(o0.float().cpu().numpy(), want, d_dtype, ("strided", c["id"], "L0"), ulps=1, absw=absw)
        _L0[key] = (o0, lse0, name0)
    o0, lse0, name0 = _L0[key]
    outcome, arg = _expect(c, layout)
    if outcome == "refused":
        with pytest.raises(RuntimeError, match=arg):
            run(c, layout, ops, rxlib)
        return
    assert issubclass(RadixHipError, RuntimeError)
    o, lse, name, P = run(c, layout, ops, rxlib)
    print(f"STRIDED {c['id']} {layout}: {name}  (L0: {name0})")
    got = o.float().cpu().numpy()
    assert not np.isnan(got).any(), (c["id"], layout, name, "NaN: poison was read, or rows of o were not written")
    parity.check_out(got, want, d_dtype, ("strided", c["id"], layout), ulps=1, absw=absw)
    if lse is not None and lse_want is not None:
        np.testing.assert_allclose(lse.cpu().numpy(), lse_want, **LSE_TOL)
    P.check_gaps((c["id"], layout, name))
    if outcome == "declined":
        assert name != name0 and re.search(arg, name.split("|")[0]), (c["id"], layout, "expected the launcher to decline to", arg, "got", name)
        return
    assert name == name0, (c["id"], layout, "aligned strides changed the kernel", name, name0)
    assert su.bits_equal(o.contiguous(), o0.contiguous()), (c["id"], layout, name, "same kernel, same values, different bits of o")
    if lse is not None:
        assert su.bits_equal(lse.contiguous(), lse0.contiguous()), (c["id"], layout, name, "same kernel, different bits of lse")


def _extend_layouts(c):
    ls = ["L2", "L4", "L6", "L6o"]
    if not c.get("unified"):
        if c["dk"] == c["dv"]:
            ls.insert(0, "L1")
        if not (c.get("mla") and not c["own_v"]):
            ls += ["L3", "L3r"]
    ls += ["L5"] if c.get("mla") else ["L5", "L5r"]   # (latent rows: "L5" = the one pool with padded rows / pages)
    return ls


EXTEND_PARAMS = [(c, l) for c in EXTEND_CASES for l in _extend_layouts(c)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,layout", EXTEND_PARAMS, ids=[f"{c['id']}-{l}" for c, l in EXTEND_PARAMS])
def test_extend_strided(case, layout):
    from sglang_amd import lib as rxlib
    from sglang_amd import ops

    d = extend_data(case)
    check_against_l0(case, layout, run_extend, d["want"], d["absw"], d["lse"], ops, rxlib)


# ----------------------------------------------------------------------------------------------------------------------
# decode: single pass, split + the stage-2 launch, split + the in-kernel merge
# ----------------------------------------------------------------------------------------------------------------------
def run_decode(c, layout, ops, rxlib, form="split"):
    d = decode_data(c)
    assert np.isfinite(d["want"]).all()
    P = Placed()
    lens, bs, hq, hkv, dv = d["lens"], len(d["lens"]), c["hq"], c["hkv"], c["dv"]
    fuse = c.get("fuse", False)
    q_layout = layout if layout in ("L0", "L2", "L4", "L6", "L6o") else "L0"
    q, _, _, o, _ = place_qkvo(P, q_layout, d["q"], None, None, (bs, hq, dv), d["dtype"], slack=_slack(c, bs))
    kn = vn = None
    if fuse:  # the step's new rows: plain, or as the views a model hands over
        kl = layout if layout in ("L1", "L2", "L3", "L3r", "L6") else "L0"
        if kl == "L1":
            q, kn, vn = _fused_qkv(d["q"], d["kn"], d["vn"])
        else:
            kn, vn = place_new_kv(P, kl, d["kn"], d["vn"], _slack(c, bs))
    variant = {"L5": "v", "L5r": "k"}.get(layout, "sym")
    kd, vd, page, lay, k_rows = place_pool(P, ops, c["pool"], d["kb"], d["vb"], variant, mla=c.get("mla", False))
    Tn = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    lens_d = Tn(lens)
    S = 8 if form != "single" else 1
    splits = al = ls = None
    if S > 1:
        splits = torch.zeros(bs, dtype=torch.int32, device=DEV)
        ops.get_num_kv_splits_balanced(splits, lens_d, hq, hkv, S, 64, 128)   # (a small budget: the long requests are cut)
        assert int(splits.max()) > 1
        al = torch.zeros(bs, hq, S, dv, dtype=torch.float32, device=DEV)
        ls = torch.zeros(bs, hq, S, dtype=torch.float32, device=DEV)
    mfma = c["fam"] in ("decode_mfma_kernel", "decode_mfma_bias_kernel")
    extra = {}
    if mfma:
        extra["request_order"] = torch.argsort(lens_d, descending=True).to(torch.int32)
    items = None
    if S > 1 and c.get("items"):
        items = ops.SplitItems(int(splits.clamp_min(1).sum()), DEV).build(splits, extra["request_order"], wgs_per_cu=3 if c.get("occ3") else 0)
        extra["split_items"] = items
    if form == "merge":
        extra["merge_counters"] = torch.zeros(bs * hq, dtype=torch.int32, device=DEV)
    if fuse:
        extra.update(k_new=kn, v_new=vn)
    if d["aux"] is not None:
        extra.update(score_mod=ops.relative_bias_score_mod, aux_tensors=[d["aux"].to(DEV)])
    with _Options(rxlib, c["opts"]):
        if c["mode"] == "indices":
            ops.decode_attention_fwd(q, kd, vd, o, Tn(d["ip"]), Tn(d["ii"]).to(torch.int32 if c.get("idx32") else torch.int64), al, ls,
                                     splits, S, d["sm"], d["ks"], d["vs"], page_size=page, kv_layout=lay, **extra)
        else:
            r2t_d, rpi_d = Tn(d["r2t"]), Tn(d["rpi"])
            if c.get("units") and (items is not None or S == 1):
                extra["units"] = ops.DecodeUnits(max(bs, 0 if items is None else items.cap), DEV).build(
                    r2t_d, rpi_d, lens_d, splits, S, items, extra["request_order"])
            ops.decode_attention_fwd_paged(q, kd, vd, o, r2t_d, rpi_d, lens_d, al, ls, splits, S, d["sm"], d["ks"], d["vs"],
                                           page_size=page, kv_layout=lay, **extra)
        torch.cuda.synchronize()
        name = rxlib.last_dispatch()
    if form == "merge":
        assert int(extra["merge_counters"].abs().sum()) == 0   # (the kernels leave the counters zero)
    if fuse:  # assertion 5: the pool rows at the page table's slots hold exactly the new rows' bits
        lastd = d["last"].to(DEV)
        assert su.bits_equal(k_rows()[lastd].cpu(), d["kn"]), (c["id"], layout, "fused store: K rows")
        v_rows = vd if c["pool"] == "nhd1" else (vd.reshape(-1, hkv, dv) if c["pool"] == "nhd16" else vd.permute(0, 2, 1, 3).reshape(-1, hkv, dv))
        assert su.bits_equal(v_rows[lastd].cpu(), d["vn"]), (c["id"], layout, "fused store: V rows")
    return o, None, name, P


def _decode_layouts(c):
    ls = ["L2", "L4", "L6", "L6o"]
    if c.get("fuse"):
        ls = ["L1", "L2", "L3", "L3r", "L4", "L6", "L6o"]
    ls += ["L5"] if c.get("mla") else ["L5", "L5r"]
    return ls


DECODE_PARAMS = [(c, l, f) for c in DECODE_CASES for l in _decode_layouts(c) for f in ("single", "split", "merge")
                 if not (f == "merge" and c["fam"] == "decode_generic_kernel")      # (no in-kernel merge there: the same call as "split")
                 and not (f == "single" and (c.get("items") or c.get("occ3")))]     # (split schedules only)


@pytest.mark.gpu
@pytest.mark.parametrize("case,layout,form", DECODE_PARAMS, ids=[f"{c['id']}-{l}-{f}" for c, l, f in DECODE_PARAMS])
def test_decode_strided(case, layout, form):
    from sglang_amd import lib as rxlib
    from sglang_amd import ops

    d = decode_data(case)
    run = lambda c, l, o_, r_: run_decode(c, l, o_, r_, form)  # noqa: E731
    check_against_l0(case, layout, run, d["want"], d["absw"], None, ops, rxlib, key=(case["id"], form))


# ----------------------------------------------------------------------------------------------------------------------
# the oracle is finite on every case's logical inputs (checked on the CPU: NaN poison proves a wrong read only then)
# ----------------------------------------------------------------------------------------------------------------------
def test_oracle_outputs_are_finite_for_every_case():
    """(the fused-RoPE and 4-bit decode tests build their inputs in their bodies and assert the same there before launching)"""
    for c in EXTEND_CASES + DECODE_CASES + VERIFY_CASES:
        d = verify_data(c) if c in VERIFY_CASES else (extend_data(c) if c["kind"] == "extend" else decode_data(c))
        assert np.isfinite(d["want"]).all() and np.isfinite(d["absw"]).all(), c["id"]
        if d.get("lse") is not None:
            assert np.isfinite(d["lse"]).all(), c["id"]


# ----------------------------------------------------------------------------------------------------------------------
# the split-KV short extend (VerifySplitKV): one request, prefix 2048, 8 new tokens, at D = 128 and at the latent shape
# ----------------------------------------------------------------------------------------------------------------------
VERIFY_CASES = [dict(id="verify-d128", dt="bf16", dk=128, dv=128, hq=8, hkv=2, pool="nhd1"),
                dict(id="verify-d128-f16", dt="f16", dk=128, dv=128, hq=8, hkv=2, pool="hnd"),
                dict(id="verify-latent", dt="bf16", dk=576, dv=512, hq=16, hkv=1, pool="nhd1", mla=True),
                dict(id="verify-latent-f16", dt="f16", dk=576, dv=512, hq=16, hkv=1, pool="hnd", mla=True)]


def verify_data(c):
    if c["id"] in _DATA:
        return _DATA[c["id"]]
    dtype, hq, hkv, dk, dv, nd, P0 = DT[c["dt"]], c["hq"], c["hkv"], c["dk"], c["dv"], 8, 2048
    rng = np.random.default_rng(_seed(c))
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    n_pages, rows = _page_table(rng, [P0])
    sc = 0.5 if c.get("mla") else 1.0
    kb = (torch.randn(n_pages * PS, hkv, dk, generator=g) * sc).to(dtype)
    vb = kb[..., :dv] if c.get("mla") else torch.randn(n_pages * PS, hkv, dv, generator=g).to(dtype)
    ke = (torch.randn(nd, hkv, dk, generator=g) * sc).to(dtype)
    ve = ke[..., :dv] if c.get("mla") else torch.randn(nd, hkv, dv, generator=g).to(dtype)
    q = torch.randn(nd, hq, dk, generator=g).to(dtype)
    qo, kvp, kvi = np.array([0, nd], np.int64), np.array([0, P0], np.int32), rows[0].astype(np.int64)
    sm = (192 if c.get("mla") else dk) ** -0.5
    want, absw = orc.extend_attention(_bits(q), _bits(ke), _bits(ve), _bits(kb), _bits(vb), qo, kvp, kvi, is_causal=True, sm_scale=sm,
                                      return_absw=True)
    _DATA[c["id"]] = d = dict(q=q, ke=ke, ve=ve, kb=kb, vb=vb, qo=qo, kvp=kvp, kvi=kvi, sm=sm, nd=nd, want=want, absw=absw, dtype=dtype)
    return d


def run_verify(c, layout, ops, rxlib):
    d = verify_data(c)
    assert np.isfinite(d["want"]).all()
    P = Placed()
    nd, hq, hkv, dv, mla = d["nd"], c["hq"], c["hkv"], c["dv"], c.get("mla", False)
    slack = _slack(c, nd)
    q, o = d["q"].to(DEV), torch.full((nd, hq, dv), float("nan"), dtype=d["dtype"], device=DEV)   # (q / o: contiguous by contract)
    if layout == "L1":    # k and v as views of one fused [T, 2 Hkv D] projection (equal strides)
        buf = torch.cat([d["ke"].reshape(nd, -1), d["ve"].reshape(nd, -1)], dim=1).to(DEV)
        k, v = (t.view(nd, hkv, -1) for t in buf.split([hkv * c["dk"], hkv * dv], dim=1))
    elif layout == "L0" or mla and layout != "L2":
        k = d["ke"].to(DEV)
        v = k[..., :dv] if mla else d["ve"].to(DEV)
    elif mla:             # one latent row per new token, carved; v its first 512 columns
        k = P.inp("k", d["ke"], 16, 8, 16, slack)
        v = k[..., :dv]
    else:
        k, v = place_new_kv(P, layout, d["ke"], d["ve"], slack)
    variant = {"L5": "v", "L5r": "k"}.get(layout, "sym")
    kd, vd, page, lay, _ = place_pool(P, ops, c["pool"], d["kb"], d["vb"], variant, mla=mla)
    Tn = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    ops.verify_attention_splitkv(q, k, v, o, kd, vd, Tn(d["qo"]), Tn(d["kvp"]), Tn(d["kvi"]), None, None, nd, 4, 1.0, 1.0,
                                 sm_scale=d["sm"], page_size=page, kv_layout=lay)
    torch.cuda.synchronize()
    return o, None, rxlib.last_dispatch(), P   # (the dispatch of the LAST launch: the new tokens' own block)


VERIFY_PARAMS = [(c, l) for c in VERIFY_CASES for l in (["L2", "L5"] if c.get("mla") else ["L1", "L2", "L3", "L3r", "L5", "L5r"])]


@pytest.mark.gpu
@pytest.mark.parametrize("case,layout", VERIFY_PARAMS, ids=[f"{c['id']}-{l}" for c, l in VERIFY_PARAMS])
def test_verify_splitkv_strided(case, layout):
    """q / o are contiguous by VerifySplitKV's contract (checked below); k / v and the pools carry the layouts.  2 ulp as in
    test_verify_attention_splitkv_vs_oracle: 16-bit chunk partials merged by LSE.  Every layout keeps the kernels of L0."""
    from sglang_amd import lib as rxlib
    from sglang_amd import ops

    d = verify_data(case)
    o0, _, name0, _ = run_verify(case, "L0", ops, rxlib)
    parity.check_out(o0.float().cpu().numpy(), d["want"], d["dtype"], ("strided", case["id"], "L0"), ulps=2, absw=d["absw"])
    o, _, name, P = run_verify(case, layout, ops, rxlib)
    got = o.float().cpu().numpy()
    assert not np.isnan(got).any(), (case["id"], layout, name)
    parity.check_out(got, d["want"], d["dtype"], ("strided", case["id"], layout), ulps=2, absw=d["absw"])
    P.check_gaps((case["id"], layout, name))
    # Outcome per layout today (rx_last_dispatch names the LAST launch, the new tokens' own block): at D = 128 that block runs
    # a packed PLAIN instance, which declines unequal K / V strides -- of the new rows (L2, L3, L3r) or of the pools (L5, L5r) --
    # to the general instance; L1 (equal strides) and every latent layout keep L0's kernel and its bits.
    declined = not case.get("mla") and layout in ("L2", "L3", "L3r", "L5", "L5r")
    print(f"STRIDED {case['id']} {layout}: {name}  (L0: {name0})")
    if declined:
        assert name != name0 and re.search(r"^extend_mfma32_kernel<.*, false, 0>$", name.split("|")[0]), (case["id"], layout, name, name0)
    else:
        assert name == name0, (case["id"], layout, "aligned strides changed the kernel", name, name0)
        assert su.bits_equal(o, o0), (case["id"], layout, name, "same kernels, different bits of o")


@pytest.mark.gpu
def test_verify_splitkv_refuses_strided_q_and_o():
    from sglang_amd import ops

    c = VERIFY_CASES[0]
    d = verify_data(c)
    nd, hq, hkv, dk = d["nd"], c["hq"], c["hkv"], c["dk"]
    q = su.carve(d["q"].to(DEV), 8, 8, 8)
    o = torch.zeros(nd, hq, dk, dtype=d["dtype"], device=DEV)
    Tn = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    args = (d["kb"].to(DEV), d["vb"].to(DEV), Tn(d["qo"]), Tn(d["kvp"]), Tn(d["kvi"]), None, None, nd, 4, 1.0, 1.0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.verify_attention_splitkv(q, d["ke"].to(DEV), d["ve"].to(DEV), o, *args)
    with pytest.raises(ValueError, match="contiguous"):
        ops.verify_attention_splitkv(d["q"].to(DEV), d["ke"].to(DEV), d["ve"].to(DEV), su.carve(o, 8, 8, 8, su.sentinel_bits(o.dtype)), *args)
    assert su.gaps_untouched(q, su.nan_bits(q.dtype))


# ----------------------------------------------------------------------------------------------------------------------
# decode_attention_fwd_grouped_rope, both forms: strided q / o, k_new, rope_k_pe_out, a cos_sin_cache with row stride > 64
# ----------------------------------------------------------------------------------------------------------------------
ROPE_PARAMS = [(dt, form, S, pool) for dt, form, S, pool in
               [("bf16", "pool_row", 1, "nhd1"), ("bf16", "k_new", 8, "hnd"), ("f16", "pool_row", 8, "hnd"), ("f16", "k_new", 1, "nhd1")]]


def _rope_call(ops, rxlib, d, form, S, pool, strided):
    P = Placed()
    bs, hq, dtype = d["bs"], d["hq"], d["dtype"]
    kb = d["kb"].clone()
    if form == "k_new":
        kb[d["last"]] = 7.0                                    # the pool does NOT hold the step's rows yet
    kd, vd, page, lay, rows = place_pool(P, ops, pool, kb, kb[..., :512], "k" if strided else "sym", mla=True)
    if strided:
        q = P.inp("q", d["q"], 8, 8, 8)
        o = P.out("o", (bs, hq, 512), dtype, 8, 16, 24)
        kpe = P.out("k_pe_out", (bs, 64), dtype, 24, 0, 8)
        cache = P.inp("cos_sin_cache", d["cache"], 8, 0, 8)    # row stride 72
        kn = P.inp("k_new", d["new_rows"], 16, 0, 8) if form == "k_new" else None
    else:
        q, o = d["q"].to(DEV), torch.full((bs, hq, 512), float("nan"), dtype=dtype, device=DEV)
        kpe, cache = torch.full((bs, 64), float("nan"), dtype=dtype, device=DEV), d["cache"].to(DEV)
        kn = d["new_rows"].to(DEV) if form == "k_new" else None
    Tn = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    ops.decode_attention_fwd_grouped_rope(q, kd, vd, o, Tn(d["kv_indptr"]), Tn(d["kv_indices"]), kpe, 512, 64, cache, Tn(d["positions"]),
                                          None, S, d["sm"], use_rope=True, is_neox_style=True, k_new=kn, page_size=page, kv_layout=lay)
    torch.cuda.synchronize()
    return o, kpe, rows().reshape(-1, 576).clone(), rxlib.last_dispatch(), P


@pytest.mark.gpu
@pytest.mark.parametrize("dt,form,S,pool", ROPE_PARAMS, ids=[f"{a}-{b}-S{c_}-{e}" for a, b, c_, e in ROPE_PARAMS])
def test_grouped_rope_decode_strided(dt, form, S, pool):
    from sglang_amd import lib as rxlib
    from sglang_amd import ops
    from test_gpu_mla_rope import _absw_rope

    dtype, hq = DT[dt], 16
    rng = np.random.default_rng(S + len(form))
    g = torch.Generator().manual_seed(S)
    lens = np.array([1, 33, 700, 64, 2049, 65], dtype=np.int64)
    bs = len(lens)
    n_pages, rows = _page_table(rng, lens)
    kv_indices = np.concatenate(rows).astype(np.int64)
    kv_indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    kb = (torch.randn(n_pages * PS, 1, 576, generator=g) * 0.5).to(dtype)
    q = (torch.randn(bs, hq, 576, generator=g) * 0.5).to(dtype)
    fr = torch.outer(torch.arange(4096).float(), 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64)))
    cache = torch.cat((fr.cos(), fr.sin()), dim=-1)
    positions = lens - 1 + rng.integers(0, 1000, size=bs)
    last = torch.from_numpy(np.array([r[-1] for r in rows], dtype=np.int64))
    sm = 192 ** -0.5
    want, kpe_want = orc.decode_attention_grouped_rope(_bits(q), _bits(kb), kv_indptr, kv_indices, cache.numpy(), positions, sm, is_neox=True)
    assert np.isfinite(want).all() and np.isfinite(kpe_want).all()
    kabs = kb.clone()
    kabs[..., :512] = kabs[..., :512].abs()
    absw = _absw_rope(_bits(q), _bits(kb), _bits(kabs), dict(positions=positions, cos_sin=cache.numpy(), kv_indices=kv_indices,
                                                             kv_indptr=kv_indptr, sm_scale=sm), True)
    d = dict(bs=bs, hq=hq, dtype=dtype, kb=kb, q=q, cache=cache, positions=positions, last=last, new_rows=kb[last, 0].clone(),
             kv_indptr=kv_indptr, kv_indices=kv_indices, sm=sm)
    o0, kpe0, rows0, name0, _ = _rope_call(ops, rxlib, d, form, S, pool, False)
    o, kpe, rows1, name, P = _rope_call(ops, rxlib, d, form, S, pool, True)
    for got in (o0, o):
        assert not torch.isnan(got.float()).any()
        parity.check_out(got.float().cpu().numpy(), want, dtype, ("strided fused rope", form, S, pool), ulps=1, absw=absw)
    u = 2.0 ** (-10 if dtype == torch.float16 else -7)   # one 16-bit rounding of the rotation, as test_fused_rope_decode_matches_oracle
    assert np.abs(kpe.float().cpu().numpy().astype(np.float64) - kpe_want).max() <= u * max(1.0, np.abs(kpe_want).max())
    assert name == name0 and name.startswith("decode_mla_kernel<"), (name, name0)
    assert su.bits_equal(o.contiguous(), o0) and su.bits_equal(kpe.contiguous(), kpe0)
    assert su.bits_equal(rows1, rows0)                    # the pool: untouched (pool_row) / the same finished rows (k_new)
    if form == "k_new":
        assert su.bits_equal(rows1[last.to(DEV), :512].cpu(), d["new_rows"][:, :512])
        assert su.bits_equal(rows1[last.to(DEV), 512:], kpe.contiguous())
    P.check_gaps(("fused rope", form, S, pool))


# ----------------------------------------------------------------------------------------------------------------------
# decode over the 4-bit pools (decode_mx4_kernel, decode_mla_mx4_kernel): q / o strides, L5 on the data AND scale buffers
# ----------------------------------------------------------------------------------------------------------------------
def _bytes_pool(P, name, a, hnd, odd, flat=False):
    """canonical uint8 [slots, H, X] -> the device buffer, carved: NHD [slots, H, X] (scales of the latent pool flat
    [slots, X]) with a per-token pad, or HND [pages, H, page + pad tokens, X] with a padded page.  odd: the other pads."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    slots, h, x = t.shape
    tail = 2 * t.numel()
    if hnd:
        padtok = 3 if odd else 1
        t4 = t.view(slots // PS, PS, h, x).permute(0, 2, 1, 3)
        return P.inp_strided(name, t4, (h * (PS + padtok) * x + (48 if odd else 16), (PS + padtok) * x, x, 1), 16, tail)
    if flat:
        return P.inp_strided(name, t.view(slots, x), (x + (28 if odd else 12), 1), 16, tail)
    return P.inp_strided(name, t, (h * x + (32 if odd else 16), x, 1), 16, tail)


MX4_PARAMS = [("bf16", 128, "nhd", (8, 2), "i64", True), ("f16", 128, "hnd", (4, 4), "r2t", True), ("bf16", 64, "hnd", (8, 2), "i32", False),
              ("f16", 64, "nhd", (16, 1), "r2t", True), ("bf16", 576, "nhd", (16, 1), "i64", True), ("f16", 576, "hnd", (16, 1), "r2t", True),
              ("bf16", 576, "hnd", (5, 1), "i32", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,d,lay,heads,mode,split", MX4_PARAMS, ids=lambda v: str(v).replace(" ", ""))
def test_mx4_decode_strided(dt, d, lay, heads, mode, split):
    """L0: the pools as the rest of the suite builds them, q / o contiguous.  Strided: q and o carved, the K data / K scale /
    V data / V scale buffers each carved with pads of its own (latent rows: the one data and the one scale buffer)."""
    from sglang_amd import lib as rxlib
    from sglang_amd import ops
    from test_gpu_kv_mx4 import _random_pool, mx4_dequant

    dtype, hnd, (hq, hkv), mla = DT[dt], lay == "hnd", heads, d == 576
    dv = 512 if mla else d
    lens = np.asarray(LENS, np.int64)
    bs = len(lens)
    rng = np.random.default_rng(d + hq + len(mode + lay))
    n_pages, rows = _page_table(rng, lens)
    r2t = np.zeros((bs + 1, int(lens.max()) + PS), dtype=np.int32)
    for i, r in enumerate(rows):
        r2t[i + 1, : len(r)] = r
    pool = _random_pool(rng, n_pages * PS, hkv, d)
    q = torch.from_numpy(rng.standard_normal((bs, hq, d)).astype(np.float32)).to(dtype)
    rpi = np.arange(1, bs + 1, dtype=np.int64)
    ip, ii = orc.build_kv_indices(r2t, rpi, lens)
    sm = (192 if mla else d) ** -0.5
    kf = mx4_dequant(pool[0], pool[1])
    vf = kf[..., :dv] if mla else mx4_dequant(pool[2], pool[3])
    want, absw = orc.decode_attention(_bits(q), kf, vf, ip, ii, sm, return_absw=True)
    assert np.isfinite(want).all()
    Tn = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    lens_d = Tn(lens)
    S = 8 if split else 1
    splits = al = ls = None
    if split:
        splits = torch.zeros(bs, dtype=torch.int32, device=DEV)
        ops.get_num_kv_splits_balanced(splits, lens_d, hq, hkv, S, 64, 128)
        assert int(splits.max()) > 1
        al = torch.zeros(bs, hq, S, dv, dtype=torch.float32, device=DEV)
        ls = torch.zeros(bs, hq, S, dtype=torch.float32, device=DEV)
    out = {}
    for layout in ("L0", "L2"):
        P = Placed()
        if layout == "L0":
            qd, o = q.to(DEV), torch.full((bs, hq, dv), float("nan"), dtype=dtype, device=DEV)
            def dev(a, flat=False):
                t = torch.from_numpy(np.ascontiguousarray(a))
                t = t.view(-1, PS, *a.shape[1:]).permute(0, 2, 1, 3).contiguous() if hnd else (t.view(a.shape[0], -1) if flat else t)
                return t.to(DEV)
            kd, ksd = dev(pool[0]), dev(pool[1], flat=True)
            vd, vsd = (kd, ksd) if mla else (dev(pool[2]), dev(pool[3], flat=True))
        else:
            qd = P.inp("q", q, 8, 8, 8)
            o = P.out("o", (bs, hq, dv), dtype, 8, 16, 24)
            kd, ksd = _bytes_pool(P, "k data", pool[0], hnd, False), _bytes_pool(P, "k scales", pool[1], hnd, True, flat=mla)
            vd, vsd = (kd, ksd) if mla else (_bytes_pool(P, "v data", pool[2], hnd, True), _bytes_pool(P, "v scales", pool[3], hnd, False))
        common = dict(page_size=PS, k_scale_buffer=ksd, v_scale_buffer=None if mla else vsd)
        if mode == "r2t":
            ops.decode_attention_fwd_paged(qd, kd, vd, o, Tn(r2t), Tn(rpi), lens_d, al, ls, splits, S, sm, 1.0, 1.0, **common)
        else:
            ops.decode_attention_fwd(qd, kd, vd, o, Tn(ip), Tn(ii).to(torch.int64 if mode == "i64" else torch.int32), al, ls, splits, S, sm,
                                     1.0, 1.0, **common)
        torch.cuda.synchronize()
        name = rxlib.last_dispatch()
        print(f"STRIDED mx4 {dt} {d} {lay} {layout}: {name}")
        got = o.float().cpu().numpy()
        assert not np.isnan(got).any(), (layout, name)
        parity.check_out(got, want, dtype, ("strided mx4", dt, d, lay, layout), ulps=1, absw=absw)
        P.check_gaps(("mx4", dt, d, lay, layout, name))
        out[layout] = (o.contiguous(), name)
    assert out["L0"][1].startswith("decode_mla_mx4_kernel<" if mla else "decode_mx4_kernel<"), out["L0"][1]
    # (the LINEAR flag follows the page strides: padded pages are not slot-major -- the same family, the same arithmetic per row)
    assert out["L2"][1].split("<")[0] == out["L0"][1].split("<")[0], (out["L2"][1], out["L0"][1])
    assert su.bits_equal(out["L2"][0], out["L0"][0]), ("same values, different bits of o", out["L2"][1])


# ----------------------------------------------------------------------------------------------------------------------
# stores and gathers with strided source rows (L2: carved, own pads; L3: one plain, one a wide view) into / out of pools
# carved with padded rows: bit-exact against the same call on contiguous copies, gaps untouched on sources and pools
# ----------------------------------------------------------------------------------------------------------------------
def _src_rows(P, layout, a, b):
    """two [n, C] source tensors under L0 / L2 / L3 / L3r (b may be None)"""
    def put(name, t, how):
        if t is None:
            return None
        if how == "plain":
            return t.to(DEV)
        return P.inp_strided(name, t, {"carve_a": (t.shape[1] + 24, 1), "carve_b": (t.shape[1] + 40, 1), "wide": (3 * t.shape[1] + 16, 1)}[how],
                             {"carve_a": 8, "carve_b": 16, "wide": 2 * t.shape[1]}[how], tail=4 * t.numel())
    how = {"L0": ("plain", "plain"), "L2": ("carve_a", "carve_b"), "L3": ("plain", "wide"), "L3r": ("wide", "plain")}[layout]
    if b is None and layout == "L3":   # one source tensor: it carries the layout (carve_b: other pads than L2's)
        how = ("carve_b", None)
    return put("src a", a, how[0]), put("src b", b, how[1])


def _byte_pool(P, name, shape, pad, dtype=torch.uint8):
    t = torch.full(shape, 0xAB, dtype=torch.uint8).view(dtype) if dtype != torch.uint8 else torch.full(shape, 0xAB, dtype=torch.uint8)
    strides = [1]
    for s in reversed(shape[1:]):
        strides.insert(0, strides[0] * s)
    strides[0] += pad
    return P.inp_strided(name, t, tuple(strides), 16, tail=64)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("layout", ["L2", "L3", "L3r"])
@pytest.mark.parametrize("op", ["fp8", "mx4", "mla_mx4_row", "mla_mx4_pair"])
def test_stores_from_strided_rows(op, layout, dt):
    from sglang_amd import ops

    dtype, n, slots, H, D = DT[dt], 70, 6 * PS, 2, 128
    g = torch.Generator().manual_seed(len(op) + len(layout))
    loc = (torch.randperm(slots - 1, generator=g)[:n] + 1).to(DEV)
    if op in ("fp8", "mx4"):
        a, b = torch.randn(n, H * D, generator=g).to(dtype), torch.randn(n, H * D, generator=g).to(dtype)
    elif op == "mla_mx4_row":
        a, b = torch.randn(n, 576, generator=g).to(dtype), None   # (one source tensor: carved under L2 / L3 with different pads, the wide view under L3r)
    else:
        a, b = torch.randn(n, 512, generator=g).to(dtype), torch.randn(n, 64, generator=g).to(dtype)
    got = {}
    for lay in ("L0", layout):
        P = Placed()
        sa, sb = _src_rows(P, lay, a, b)
        if op == "fp8":
            pools = [_byte_pool(P, "k pool", (slots, H, D), 32, torch.float8_e4m3fn), _byte_pool(P, "v pool", (slots, H, D), 48, torch.float8_e4m3fn)]
            ops.store_cache_fp8(sa, sb, ops._kv_layout(pools[0], pools[1], 1), loc, H, D, D, size_limit=slots, k_scale=0.8, v_scale=1.25)
        elif op == "mx4":
            pools = [_byte_pool(P, "k data", (slots, H, D // 2), 16), _byte_pool(P, "v data", (slots, H, D // 2), 32),
                     _byte_pool(P, "k scales", (slots, H, D // 16), 8), _byte_pool(P, "v scales", (slots, H, D // 16), 24)]
            ops.store_cache_mx4(sa, sb, pools[0], pools[1], pools[2], pools[3], loc, page_size=1)
        else:
            pools = [_byte_pool(P, "kv data", (slots, 1, 288), 16), _byte_pool(P, "kv scales", (slots, 36), 12)]
            ops.store_cache_mla_mx4(sa, sb, pools[0], pools[1], loc)
        torch.cuda.synchronize()
        P.check_gaps((op, lay))
        got[lay] = [p.contiguous() for p in pools]
    for p0, p1 in zip(got["L0"], got[layout]):
        assert su.bits_equal(p0, p1), (op, layout, "pool bytes differ from the contiguous call's")
    written = got[layout][0].view(torch.uint8).reshape(slots, -1)
    assert (written[loc] != 0xAB).any(dim=1).all() and (written[0] == 0xAB).all()   # (the rows were stored; slot 0 never)


@pytest.mark.gpu
@pytest.mark.parametrize("pdt", ["bf16", "f16", "fp8"])
def test_get_mla_kv_from_padded_rows(pdt):
    """The source of this gather is the latent pool itself: one head of 576 columns per row, so the only stride it has is the
    row stride -- a carve with row stride 592 and an offset IS L2 here, and L3 (k and v apart) does not exist for it."""
    from sglang_amd import ops

    slots, g = 6 * PS, torch.Generator().manual_seed(3)
    dst = DT.get(pdt, torch.bfloat16)
    rows = (torch.randn(slots, 1, 576, generator=g) * 0.5).to(torch.float8_e4m3fn if pdt == "fp8" else dst)
    loc = torch.randint(0, slots, (50,), generator=g).to(DEV)
    P = Placed()
    padded = P.inp_strided("kv pool", rows, (592, 576, 1), 16, tail=4096)
    n0, r0 = ops.get_mla_kv(rows.to(DEV), loc, 512, 64, dst, size_limit=slots)
    n1, r1 = ops.get_mla_kv(padded, loc, 512, 64, dst, size_limit=slots)
    torch.cuda.synchronize()
    assert su.bits_equal(n0, n1) and su.bits_equal(r0, r1) and not torch.isnan(n1.float()).any() and not torch.isnan(r1.float()).any()
    want = rows.to(DEV)[loc].to(dst) if pdt == "fp8" else rows.to(DEV)[loc]
    assert su.bits_equal(torch.cat([n1, r1], -1), want)
    P.check_gaps(("get_mla_kv", pdt))


# ----------------------------------------------------------------------------------------------------------------------
# rope_store_kv: q / k rotated in place inside strided views, the rotated k and v stored into pools with padded rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("pool", ["nhd16bit", "nhd_fp8", "hnd16bit"])
@pytest.mark.parametrize("layout", ["L1", "L2", "L3", "L3r"])
def test_rope_store_kv_strided(layout, pool, dt):
    """Bit-exact against the same call on contiguous copies: the rotated q and k (written in place, inside the views) and every
    pool byte; gaps untouched around q, k, v and in the padded pools.  L1: q / k / v are views of one fused qkv, rotated in
    place there (the out-of-place rotation that leaves k contiguous beside a v view is L3)."""
    from sglang_amd import ops

    dtype, n, hq, hkv, d, slots = DT[dt], 70, 8, 2, 128, 6 * PS
    g = torch.Generator().manual_seed(len(layout) + len(pool))
    q, k, v = (torch.randn(n, h, d, generator=g).to(dtype) for h in (hq, hkv, hkv))
    pos = torch.randint(0, 4096, (n,), generator=g).to(DEV)
    fr = torch.outer(torch.arange(4096).float(), 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d)))
    cache = torch.cat((fr.cos(), fr.sin()), dim=-1).to(DEV)
    loc = (torch.randperm(slots - 1, generator=g)[:n] + 1).to(DEV)
    got = {}
    for lay in ("L0", layout):
        P = Placed()
        if lay == "L0":
            qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
        elif lay == "L1":
            qd, kd, vd = _fused_qkv(q, k, v)
        else:
            qd = P.inp("q", q, 8, 8, 8) if lay == "L2" else q.to(DEV)
            kd, vd = place_new_kv(P, lay, k, v, 0)
        if pool == "hnd16bit":
            shape, strides = (slots // PS, hkv, PS, d), (hkv * (PS + 2) * d + 24, (PS + 2) * d, d, 1)
            pools = [P.inp_strided(nm, torch.zeros(shape, dtype=dtype), strides, 16, tail=64) for nm in ("k pool", "v pool")]
            lay_kv = ops.kv_layout_hnd(*pools)
        else:
            pdt = torch.float8_e4m3fn if pool == "nhd_fp8" else dtype
            pools = [P.inp_strided(nm, torch.zeros(slots, hkv, d).to(pdt),
                                   (hkv * d + pad, d, 1), 16, tail=64) for nm, pad in (("k pool", 32), ("v pool", 48))]
            lay_kv = ops._kv_layout(pools[0], pools[1], 1)
        sc = dict(k_scale=0.5, v_scale=2.0) if pool == "nhd_fp8" else {}
        ops.rope_store_kv(qd, kd, vd, pos, cache, True, layout=lay_kv, loc=loc, size_limit=slots, **sc)
        torch.cuda.synchronize()
        P.check_gaps(("rope_store_kv", lay, pool))
        got[lay] = [qd.contiguous(), kd.contiguous(), vd.contiguous()] + [p.contiguous() for p in pools]
    for name, a, b in zip(("q", "k", "v", "k pool", "v pool"), got["L0"], got[layout]):
        assert su.bits_equal(a, b), (layout, pool, name, "differs from the contiguous call")
    assert not su.bits_equal(got[layout][0], q.to(DEV)) and su.bits_equal(got[layout][2], v.to(DEV))   # (q was rotated, v only read)
    rows = got[layout][3] if pool != "hnd16bit" else got[layout][3].permute(0, 2, 1, 3).reshape(slots, hkv, d)
    if pool != "nhd_fp8":
        assert su.bits_equal(rows[loc], got[layout][1])   # the pool holds exactly the rotated k


# ----------------------------------------------------------------------------------------------------------------------
# the backend, end to end: forward_extend then forward_decode with q / k / v as views of one fused qkv projection
# ----------------------------------------------------------------------------------------------------------------------
def _backend_run(kind, fused):
    """A fresh pool + HipRadixAttnBackend; prefixes stored, one extend forward, one decode forward.  Returns the two outputs,
    the two dispatch strings and every byte of the pool."""
    from sglang_amd import lib as rxlib
    from sglang_amd import ops
    from sglang_amd.attention.backend import HipRadixAttnBackend
    from sglang_amd.attention.radix_attention import RadixAttention
    from sglang_amd.forward_batch import ForwardBatch
    from sglang_amd.mem_cache.allocator import PagedTokenToKVPoolAllocator
    from sglang_amd.mem_cache.memory_pool import MHATokenToKVPool, MHATokenToKVPoolFP4, ReqToTokenPool

    hq, hkv, d, dtype, size = 8, 2, 128, torch.bfloat16, 2048
    if kind == "mx4":
        pool = MHATokenToKVPoolFP4(size, PS, dtype, hkv, d, 1, DEV)
    else:
        pool = MHATokenToKVPool(size, PS, torch.float8_e4m3fn if kind == "fp8" else dtype, hkv, d, 1, DEV)
    r2t = ReqToTokenPool(8, 1024, DEV)
    alloc = PagedTokenToKVPoolAllocator(size, PS, dtype, DEV, pool, debug_mode=True)

    class MC:
        num_attention_heads, num_key_value_heads, context_len = hq, hkv, 1024

    class MR:
        device, req_to_token_pool, token_to_kv_pool, token_to_kv_pool_allocator, model_config, page_size = DEV, r2t, pool, alloc, MC, PS
        dtype = torch.bfloat16

        class server_args:
            triton_attention_num_kv_splits = 8

    backend = HipRadixAttnBackend(MR)
    layer = RadixAttention(hq, d, d ** -0.5, hkv, 0)
    g = torch.Generator().manual_seed(3)
    rand = lambda *shape: torch.randn(*shape, generator=g).to(dtype).to(DEV)  # noqa: E731
    pre, ext = [0, 70, 200, 33], [1, 40, 129, 257]
    rows = r2t.alloc(len(pre))
    rpi = torch.tensor(rows, dtype=torch.int64, device=DEV)

    def grow(old, new):   # alloc_for_extend: slots + req_to_token rows
        o_, n_ = torch.tensor(old, dtype=torch.int64), torch.tensor(new, dtype=torch.int64)
        last = torch.tensor([int(r2t.req_to_token[r, p - 1]) if p > 0 else -1 for r, p in zip(rows, old)], dtype=torch.int64, device=DEV)
        out = alloc.alloc_extend(o_.to(DEV), o_, n_.to(DEV), n_, last, int((n_ - o_).sum()))
        ops.write_req_to_token(r2t.req_to_token, rpi, None, o_.to(DEV), n_.to(DEV), (n_ - o_).to(DEV), out)
        return out

    def qkv(n):   # the same values either way: views of ONE [n, (Hq + 2 Hkv) D] buffer, or contiguous copies of them
        buf = rand(n, (hq + 2 * hkv) * d)
        parts = buf.split([hq * d, hkv * d, hkv * d], dim=1)
        assert not parts[0].is_contiguous() and parts[1].stride(0) == (hq + 2 * hkv) * d
        return parts if fused else tuple(p.contiguous() for p in parts)

    pool.set_kv_buffer(layer, grow([0] * len(pre), pre), rand(sum(pre), hkv, d), rand(sum(pre), hkv, d))
    seq = [p + e for p, e in zip(pre, ext)]
    loc = grow(pre, seq)
    q, k, v = qkv(sum(ext))
    fb = ForwardBatch.for_extend(rpi, torch.tensor(seq, device=DEV), loc, pre, ext)
    backend.init_forward_metadata(fb)
    o_ext = layer(q, k, v, fb, backend).clone()
    torch.cuda.synchronize()
    name_ext = rxlib.last_dispatch()
    seq1 = [s + 1 for s in seq]
    loc = grow(seq, seq1)
    q, k, v = qkv(len(pre))
    seq_t = torch.tensor(seq1, dtype=torch.int64)
    fb = ForwardBatch.for_decode(rpi, seq_t.to(DEV), loc, seq_t)
    backend.init_forward_metadata(fb)
    o_dec = layer(q, k, v, fb, backend).clone()
    torch.cuda.synchronize()
    name_dec = rxlib.last_dispatch()
    assert pool.check_errors() == 0
    bufs = pool.k_buffer + pool.v_buffer + (pool.k_scale_buffer + pool.v_scale_buffer if kind == "mx4" else [])
    return o_ext, o_dec, name_ext, name_dec, [b.clone() for b in bufs]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nhd16", "fp8", "mx4"])
def test_backend_on_fused_qkv_views(kind):
    """The production layout end to end: the backend's own .view(-1, H, D) of the views, the store into the pool, the decode
    from what was stored.  Outputs and pool bytes bit-identical to the run on contiguous copies, the same kernels."""
    oe0, od0, ne0, nd0, bytes0 = _backend_run(kind, fused=False)
    oe1, od1, ne1, nd1, bytes1 = _backend_run(kind, fused=True)
    assert not torch.isnan(oe1.float()).any() and not torch.isnan(od1.float()).any()
    assert (ne1, nd1) == (ne0, nd0), ("the fused views changed a kernel", ne1, ne0, nd1, nd0)
    assert nd0.startswith("decode_mx4_kernel<" if kind == "mx4" else "decode_mfma_kernel<"), nd0
    assert su.bits_equal(oe1, oe0) and su.bits_equal(od1, od0)
    assert len(bytes0) == len(bytes1) and all(su.bits_equal(a, b) for a, b in zip(bytes0, bytes1))
    assert any(int(b.view(torch.uint8).count_nonzero()) > 0 for b in bytes1)
