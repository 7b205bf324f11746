"""Shared-prefix (cascade) decode over a 4-bit (MXFP4) pool against the routes around it, same pool, same batch, same session
(DESIGN 4.1c):

  (a) "plain":    per-request rx_decode_attn_mx4 on the whole rows, native split schedule -- the only route before the cascade;
  (b) "cascade" / "cascade_extend": ops.CascadeDecode(mx4=True), the whole op (phase 1 + suffix decode + stage 2; the plan is made
      once, outside), phase 1 on cascade_mx4_kernel (option cascade_mx4 = 1) / on extend_mx4_kernel (= 0);
  (c) "phase1_cascade" / "phase1_extend": phase 1 alone on identical arguments, option cascade_mx4 = 1 (cascade_mx4_kernel)
      against = 0 (extend_mx4_kernel);
  (d) "cascade16": the 16-bit pool's cascade on the same page table, for scale.

    python tools/cascade_mx4_sweep.py [--shapes p,s,l] [--rounds 7] [--out profiles/cascade_mx4.jsonl]

Warm launches (~80 ms of all routes), then the routes interleaved round by round, each timed as a run of back-to-back eager
launches between two events (the option of (c) is read on the host at launch, so nothing is graph-captured); medians and every
round are printed, one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sglang_amd import lib as rxlib  # noqa: E402
from sglang_amd import ops  # noqa: E402

DEV, PS, HQ, HKV, D = "cuda", 16, 32, 8, 128
# name -> (requests, shared tokens, own tokens, launches per timed run)
SHAPES = {"p": (256, 3584, 512, 20), "s": (64, 3584, 512, 40), "l": (256, 8192, 256, 20)}


def run(name, rounds):
    bs, shared, own, launches = SHAPES[name]
    g = torch.Generator(device=DEV).manual_seed(1)
    pages = (shared + bs * own) // PS
    perm = (torch.randperm(pages, device=DEV, generator=g) + 1).to(torch.int32)   # shuffled pages; page 0 is the padding sink
    slots = (perm.view(-1, 1) * PS + torch.arange(PS, device=DEV, dtype=torch.int32)).view(-1)
    r2t = torch.zeros(bs + 1, shared + own + PS, dtype=torch.int32, device=DEV)
    r2t[1:, :shared] = slots[:shared]
    r2t[1:, shared: shared + own] = slots[shared:].view(bs, own)
    rpi = torch.arange(1, bs + 1, dtype=torch.int64, device=DEV)
    lens = torch.full((bs,), shared + own, dtype=torch.int64, device=DEV)
    u8 = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=g)  # noqa: E731
    sb = lambda lo: torch.randint(lo, lo + 9, (pages + 1, HKV, PS, D // 16), device=DEV, generator=g).to(torch.uint8)  # noqa: E731
    kd, vd, ksd, vsd = u8(pages + 1, HKV, PS, D // 2), u8(pages + 1, HKV, PS, D // 2), sb(119), sb(121)   # HND pages
    k16 = torch.randn(pages + 1, HKV, PS, D, device=DEV, generator=g).to(torch.bfloat16)
    v16 = torch.randn(pages + 1, HKV, PS, D, device=DEV, generator=g).to(torch.bfloat16)
    q = torch.randn(bs, HQ, D, device=DEV, generator=g).to(torch.bfloat16)
    sm, cus = D ** -0.5, torch.cuda.get_device_properties(0).multi_processor_count
    outs = {r: torch.empty_like(q) for r in ("plain", "cascade", "cascade16")}

    S = ops.native_max_kv_splits(bs, HQ, HKV, cus, 32)
    splits = torch.ones(bs, dtype=torch.int32, device=DEV)
    if S > 1:
        ops.get_num_kv_splits_native(splits, lens, HQ, HKV, S, cus)
    al = torch.empty(bs, HQ, S, D, dtype=torch.float32, device=DEV)
    ls = torch.empty(bs, HQ, S, dtype=torch.float32, device=DEV)
    cd = ops.CascadeDecode(bs, HQ, HKV, D, torch.bfloat16, DEV, max_shared=r2t.shape[1], cu_count=cus, min_shared=64, mx4=True)
    cd16 = ops.CascadeDecode(bs, HQ, HKV, D, torch.bfloat16, DEV, max_shared=r2t.shape[1], cu_count=cus, min_shared=64)
    for c in (cd, cd16):
        c.plan(r2t, rpi, lens)
    assert cd.shared_len() == shared
    nc = cd.num_chunks
    q_rep = q.unsqueeze(0).expand(nc, -1, -1, -1).reshape(nc * bs, HQ, D).contiguous()
    kx = torch.zeros(1, HKV, D, dtype=torch.bfloat16, device=DEV)   # (skip_extend: only its kv head count is read)
    o1 = torch.empty_like(q_rep)
    lse1 = torch.empty(nc * bs, HQ, dtype=torch.float32, device=DEV)

    def plain():
        ops.decode_attention_fwd_paged(q, kd, vd, outs["plain"], r2t, rpi, lens, al, ls, splits if S > 1 else None, S, sm, page_size=PS,
                                       k_scale_buffer=ksd, v_scale_buffer=vsd)

    def phase1(opt):
        with rxlib.option("cascade_mx4", opt):
            ops.extend_attention_fwd(q_rep, kx, kx, o1, kd, vd, cd.qo_indptr, cd.chunk_indptr, cd.shared_indices, None, False, None, bs, 1.0,
                                     1.0, sm_scale=sm, skip_extend=True, lse_extend=lse1, page_size=PS, k_scale_buffer=ksd,
                                     v_scale_buffer=vsd)

    def cascade(opt):
        with rxlib.option("cascade_mx4", opt):
            cd(q, kd, vd, outs["cascade"], sm, page_size=PS, k_scale_buffer=ksd, v_scale_buffer=vsd)

    routes = {"plain": plain, "cascade": lambda: cascade(1), "cascade_extend": lambda: cascade(0),
              "phase1_cascade": lambda: phase1(1), "phase1_extend": lambda: phase1(0),
              "cascade16": lambda: cd16(q, k16, v16, outs["cascade16"], sm, page_size=PS, kv_layout=ops.kv_layout_hnd(k16, v16))}
    kernels = {}
    for route, fn in routes.items():
        fn()
        torch.cuda.synchronize()
        kernels[route] = rxlib.last_dispatch()
    diff = float((outs["plain"].float() - outs["cascade"].float()).abs().max())
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < 80.0:   # the clock ramp after idle, on these launches
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
    times = {route: [] for route in routes}
    for _ in range(rounds):
        for route, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[route].append(e0.elapsed_time(e1) * 1e3 / launches)
    out = dict(shape=dict(name=name, bs=bs, shared=shared, own=own, hq=HQ, hkv=HKV, d=D, page=PS, layout="hnd"), chunks=nc,
               plain_max_kv_splits=S, launches_per_run=launches, max_abs_plain_minus_cascade=diff)
    for route in routes:
        out[route] = dict(us_per_call=round(float(np.median(times[route])), 2), us_all=[round(t, 2) for t in times[route]],
                          kernel=kernels[route])
    out["cascade_over_plain"] = round(out["cascade"]["us_per_call"] / out["plain"]["us_per_call"], 4)
    out["cascade_extend_over_plain"] = round(out["cascade_extend"]["us_per_call"] / out["plain"]["us_per_call"], 4)
    out["phase1_cascade_over_extend"] = round(out["phase1_cascade"]["us_per_call"] / out["phase1_extend"]["us_per_call"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name in a.shapes.split(","):
        lines.append(json.dumps(run(name, a.rounds)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
