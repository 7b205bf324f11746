"""Extend attention over a 4-bit (MXFP4) pool, two routes on the same pool and the same batch, same session: "native"
(rx_extend_attn_mx4: the packed prefix and the new tokens in one pass) against "gather" (rx_gather_kv_mx4 into a dense 16-bit
copy + the 16-bit extend on it with kv_indices = arange: the backend's other route).  Launches back to back inside a replayed
graph (at least ~10 ms of them per timed replay), the routes interleaved round by round, ~80 ms of the same launches before the
timed rounds.

    python tools/extend_mx4_sweep.py [--shapes a,b,...] [--rounds 7] [--out profiles/extend_mx4_vs_gather.jsonl]

Prints one JSON line per shape: us per layer call of each route (median and every round), the native route's TB/s on its own
algorithmic bytes, the bytes each route moves, and the largest |native - gather| of the outputs."""
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
# name -> (requests, prefix tokens, new tokens, launches per replayed graph: a timed replay is >= ~10 ms of launches).
# (a)-(d): the shapes of the first table; (e)-(l): at most 64 query rows per kv head (16 new tokens x G 4) over grids from
# 8 to 2048 workgroups and prefixes from 256 to 32 k, the regime the routing rule is drawn in
SHAPES = {"a": (8, 8192, 64, 40), "b": (1, 32768, 64, 20), "c": (64, 1024, 16, 200), "d": (32, 3584, 512, 10),
          "e": (1, 32768, 16, 20), "f": (8, 8192, 16, 40), "g": (16, 4096, 16, 80), "h": (32, 2048, 16, 120),
          "i": (64, 256, 16, 400), "j": (256, 1024, 16, 60), "k": (16, 32768, 16, 10), "l": (64, 8192, 16, 20)}


def run(name, rounds):
    bs, pre, ext, launches = SHAPES[name]
    g = torch.Generator(device=DEV).manual_seed(1)
    pages = bs * pre // PS
    perm = torch.randperm(pages, device=DEV, generator=g) + 1   # shuffled pages; page 0 is the padding sink
    kv_indices = (perm.view(-1, 1) * PS + torch.arange(PS, device=DEV)).view(-1)
    kv_indptr = (torch.arange(bs + 1, device=DEV) * pre).to(torch.int32)
    qo_indptr = (torch.arange(bs + 1, device=DEV) * ext).to(torch.int32)
    u8 = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=g)  # noqa: E731
    sb = lambda lo: torch.randint(lo, lo + 9, (pages + 1, HKV, PS, D // 16), device=DEV, generator=g).to(torch.uint8)  # noqa: E731
    kd, vd, ksd, vsd = u8(pages + 1, HKV, PS, D // 2), u8(pages + 1, HKV, PS, D // 2), sb(119), sb(121)   # HND pages
    q = torch.randn(bs * ext, HQ, D, device=DEV, generator=g).to(torch.bfloat16)
    k = torch.randn(bs * ext, HKV, D, device=DEV, generator=g).to(torch.bfloat16)
    v = torch.randn(bs * ext, HKV, D, device=DEV, generator=g).to(torch.bfloat16)
    outs = {r: torch.empty_like(q) for r in ("native", "gather")}

    def native():
        ops.extend_attention_fwd(q, k, v, outs["native"], kd, vd, qo_indptr, kv_indptr, kv_indices, None, True, None, ext, 1.0, 1.0,
                                 sm_scale=D ** -0.5, page_size=PS, k_scale_buffer=ksd, v_scale_buffer=vsd)

    def gather():
        kb, vb = ops.gather_kv_mx4(kd, vd, ksd, vsd, kv_indices, torch.bfloat16, page_size=PS)
        ops.extend_attention_fwd(q, k, v, outs["gather"], kb, vb, qo_indptr, kv_indptr,
                                 torch.arange(kb.shape[0], dtype=torch.int64, device=DEV), None, True, None, ext, 1.0, 1.0,
                                 sm_scale=D ** -0.5, page_size=1)

    graphs, kernels = {}, {}
    for route, fn in (("native", native), ("gather", gather)):
        fn()
        torch.cuda.synchronize()
        kernels[route] = rxlib.last_dispatch()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(launches):
                fn()
        graphs[route] = gr
    diff = float((outs["native"].float() - outs["gather"].float()).abs().max())
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < 80.0:   # the clock ramp after idle, on these launches
        for gr in graphs.values():
            gr.replay()
        torch.cuda.synchronize()
    times = {route: [] for route in graphs}
    for _ in range(rounds):
        for route, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[route].append(e0.elapsed_time(e1) * 1e3 / launches)
    rows = bs * pre * HKV * 2                                  # (token, kv head) rows of K and of V
    qkvo = 2 * (2 * q.numel() + k.numel() + v.numel())
    nbytes = {"native": rows * (D // 2 + D // 16) + qkvo, "gather": rows * (D // 2 + D // 16 + 2 * 2 * D) + qkvo}
    out = dict(shape=dict(name=name, bs=bs, prefix=pre, new=ext, hq=HQ, hkv=HKV, d=D, page=PS, layout="hnd"),
               launches_per_replay=launches, max_abs_native_minus_gather=diff)
    for route in graphs:
        us = float(np.median(times[route]))
        out[route] = dict(us_per_call=round(us, 2), us_all=[round(t, 2) for t in times[route]], algorithmic_bytes=nbytes[route],
                          tb_per_s=round(nbytes[route] / us / 1e6, 3), kernel=kernels[route])
    out["native_over_gather"] = round(out["native"]["us_per_call"] / out["gather"]["us_per_call"], 4)
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
