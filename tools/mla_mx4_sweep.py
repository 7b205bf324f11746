"""Per-layer MLA decode time of the three latent pools -- 16-bit, fp8 e4m3 and 4-bit MXFP4 -- at one shape, same session:
launches back to back inside a replayed graph, the pools interleaved round by round.

    python tools/mla_mx4_sweep.py [--bs 64 --len 8192 --hq 16] [--out profiles/x.jsonl]   (appends one line)

Prints one JSON line: us per layer, and TB/s on each pool's own algorithmic bytes (sum seq * row bytes + Q + O)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sglang_amd import lib as rxlib  # noqa: E402
from sglang_amd import ops  # noqa: E402

DEV, PS, D, DV = "cuda", 16, 576, 512


def main():
    ap = argparse.ArgumentParser()
    for name, val in (("bs", 64), ("len", 8192), ("hq", 16), ("launches", 20), ("rounds", 7)):
        ap.add_argument("--" + name, type=int, default=val)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bs, L, hq = a.bs, a.len, a.hq
    pages = bs * L // PS
    slots = (pages + 1) * PS
    g = torch.Generator(device=DEV).manual_seed(1)
    perm = torch.randperm(pages, device=DEV, generator=g) + 1   # shuffled pages; page 0 is the padding sink
    r2t = torch.zeros(bs + 1, L, dtype=torch.int32, device=DEV)
    r2t[1:] = (perm.view(bs, L // PS, 1) * PS + torch.arange(PS, device=DEV)).view(bs, L).to(torch.int32)
    rpi = torch.arange(1, bs + 1, dtype=torch.int64, device=DEV)
    lens = torch.full((bs,), L, dtype=torch.int64, device=DEV)
    q = torch.randn(bs, hq, D, device=DEV, generator=g).to(torch.bfloat16)
    u8 = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=g)  # noqa: E731
    pools = {
        "bf16": dict(k=torch.randn(slots, 1, D, device=DEV, generator=g).to(torch.bfloat16), row=2 * D, kw={}),
        "fp8": dict(k=(u8(slots, 1, D) & 0x77).view(torch.float8_e4m3fn), row=D, kw={}),   # (no NaN encodings)
        "mx4": dict(k=u8(slots, 1, D // 2), row=D // 2 + D // 16,
                    kw=dict(k_scale_buffer=torch.randint(119, 128, (slots, D // 16), device=DEV, generator=g).to(torch.uint8))),
    }
    # one schedule for the three pools: whole requests when they cover the chip twice, else the balanced split
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = bs * ((hq + 15) // 16)
    S = 1 if blocks >= 2 * cus else 8
    splits = al = ls = None
    if S > 1:
        splits = torch.zeros(bs, dtype=torch.int32, device=DEV)
        ops.get_num_kv_splits_balanced(splits, lens, hq, 1, S, 2 * cus, 1024)
        al = torch.zeros(bs, hq, S, DV, dtype=torch.float32, device=DEV)
        ls = torch.zeros(bs, hq, S, dtype=torch.float32, device=DEV)
    graphs, names = {}, {}
    for name, p in pools.items():
        o = torch.empty(bs, hq, DV, dtype=torch.bfloat16, device=DEV)
        v = p["k"] if name == "mx4" else p["k"][..., :DV]

        def call(p=p, o=o, v=v):
            ops.decode_attention_fwd_paged(q, p["k"], v, o, r2t, rpi, lens, al, ls, splits, S, D ** -0.5, page_size=PS, **p["kw"])

        call()
        torch.cuda.synchronize()
        names[name] = rxlib.last_dispatch()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(a.launches):
                call()
        graphs[name] = gr
    for gr in graphs.values():   # warm clocks
        for _ in range(3):
            gr.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in pools}
    for _ in range(a.rounds):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    out = dict(shape=dict(bs=bs, len=L, hq=hq, page=PS, split_slots=S,
                          splits_per_request=int(splits.max()) if splits is not None else 1), launches_per_replay=a.launches)
    for name, p in pools.items():
        us = float(np.median(times[name]))
        nbytes = bs * L * p["row"] + bs * hq * (D + DV) * 2
        out[name] = dict(us_per_layer=round(us, 2), us_all=[round(t, 2) for t in times[name]], algorithmic_bytes=nbytes,
                         tb_per_s=round(nbytes / us / 1e6, 3), kernel=names[name])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
