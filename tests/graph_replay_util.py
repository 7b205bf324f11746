"""The runner's graph-replay protocol around HipRadixAttnBackend, for tests/test_gpu_graph_replay_matrix.py (and
`capture` for tests/test_gpu_backend.py): a mock runner over real pools, the allocator and ReqToTokenPool; ONE captured
graph of two layers at batch size B; a script of live batches replayed through it, each one checked against the fp64
oracle, its eager twin, the bytes set_kv_buffer writes on a scratch pool, and a snapshot of everything a step must
leave alone.  `metadata_sweep` is the attention-free half: init_forward_metadata_out_graph at every batch size, with the
addresses, extents and counts of whatever it returns."""
import dataclasses
import json
import os
import types
from typing import Optional, Tuple

import numpy as np
import torch

import parity_util as parity
from oracle import radix_oracle as orc

DEV = "cuda"
B = 4                             # the captured batch size
POOL_SLOTS, MAX_CTX = 8192, 2304  # smallest shapes that reach a split schedule, a page edge and the padded grid
RANK, ROPE = 512, 64              # latent rows: 576 / 512 over one kv head
EXTENT = 48                       # relative-bias table per (request, head)
LOG = os.path.join(os.path.dirname(parity.LOG), "graph_replay_matrix.jsonl")   # next to parity_util's own records
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6], dtype=np.float64)

# lengths BEFORE the step's new token
SCRIPT = (("R1", (600, 33, 1024, 7)),     # mixed: some requests cut, some whole
          ("R2", (1, 2047, 130, 15)),     # one long request; 2047 -> 2048 and 15 -> 16 end a page; a length-1 request
          ("R3", (16, 2200)),             # + two padding rows; 16 -> 17 opens a page; the script's longest request
          ("R4", (40, 41, 42, 43)))       # everyone one pass: R3's counts and partials must not leak
SWA_R1 = (10, 64, 65, 700)                # W = 64: below, at and above the window


def capture(fn):
    """Warm on a side stream (allocator, lazy launchers), then capture fn() into a HIP graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


@dataclasses.dataclass(frozen=True)
class Config:
    id: str
    kind: str = "mha"                      # "mha" | "mx4" | "mla" | "mla-mx4"
    hq: int = 8
    hkv: int = 2
    dk: int = 128
    dv: int = 0                            # 0: dk
    dtype: torch.dtype = torch.bfloat16    # q / o / incoming rows
    pool_dtype: Optional[torch.dtype] = None
    page: int = 16
    hnd: bool = False
    window: int = 0                        # layer 1 is the windowed one, layer 0 global
    sinks: bool = False
    logit_cap: float = 0.0
    xai: int = 0
    relbias: bool = False
    det: bool = False
    static: bool = False
    policy: str = "native"
    scales: Optional[Tuple[float, float]] = None   # the layers' (k_scale, v_scale)
    family: Tuple[str, ...] = ("decode_mfma_kernel",)

    @property
    def v(self):
        return self.dv or self.dk

    @property
    def latent(self):
        return self.kind in ("mla", "mla-mx4")


def mx4_dequant(data, scales):
    """uint8 data [..., D/2] + scale bytes [..., D/16] -> float32 [..., D], exact (include/radix_hip.h, "4-bit KV pool")."""
    nib = np.stack([data & 15, data >> 4], -1).reshape(*data.shape[:-1], -1)
    val = E2M1[nib & 7] * np.where(nib & 8, -1.0, 1.0)
    return (val * np.exp2(np.repeat(scales.astype(np.float64), 16, -1) - 127)).astype(np.float32)


def make_pool(cfg: Config):
    from sglang_amd.mem_cache import memory_pool as mp

    pdt = cfg.pool_dtype or cfg.dtype
    if cfg.kind == "mha":
        return mp.MHATokenToKVPool(POOL_SLOTS, cfg.page, pdt, cfg.hkv, cfg.dk, 2, DEV, v_head_dim=cfg.v, use_hnd=cfg.hnd)
    if cfg.kind == "mx4":
        return mp.MHATokenToKVPoolFP4(POOL_SLOTS, cfg.page, cfg.dtype, cfg.hkv, cfg.dk, 2, DEV, use_hnd=cfg.hnd)
    if cfg.kind == "mla":
        return mp.MLATokenToKVPool(POOL_SLOTS, cfg.page, pdt, RANK, ROPE, 2, DEV)
    assert cfg.kind == "mla-mx4", cfg.kind
    return mp.MLATokenToKVPoolFP4(POOL_SLOTS, cfg.page, cfg.dtype, RANK, ROPE, 2, DEV)


def pool_buffers(pool):
    """Every device buffer of a pool, all layers: data and (4-bit pools) scale bytes."""
    out = []
    for name in ("k_buffer", "v_buffer", "k_scale_buffer", "v_scale_buffer", "kv_buffer", "kv_scale_buffer"):
        out += [(f"{name}[{i}]", b) for i, b in enumerate(getattr(pool, name, []))]
    return out


def held_rows(cfg: Config, pool, layer_id: int, slots: torch.Tensor):
    """The values the pool HOLDS at ``slots`` as the oracle's float K [n, Hkv, Dk] / V [n, Hkv, Dv]: 16-bit and fp8 bytes
    upcast (exact), 4-bit bytes dequantised in numpy from the raw data and scale bytes."""
    ps, n = pool.page_size, slots.numel()

    def rows(buf, x):
        if pool.use_hnd:
            return buf[slots // ps, :, slots % ps, :]
        return buf[slots].reshape(n, -1, x)

    if cfg.kind == "mha":
        kb, vb = pool.get_kv_buffer(layer_id)
        return rows(kb, cfg.dk).float().cpu().numpy(), rows(vb, cfg.v).float().cpu().numpy()
    if cfg.kind == "mx4":
        kb, vb, ksb, vsb = pool.get_mx4_buffers(layer_id)
        return (mx4_dequant(rows(kb, cfg.dk // 2).cpu().numpy(), rows(ksb, cfg.dk // 16).cpu().numpy()),
                mx4_dequant(rows(vb, cfg.v // 2).cpu().numpy(), rows(vsb, cfg.v // 16).cpu().numpy()))
    if cfg.kind == "mla":
        k = pool.get_key_buffer(layer_id)[slots].float().cpu().numpy()
    else:
        kb, ksb = pool.get_mx4_buffers(layer_id)
        k = mx4_dequant(kb[slots].cpu().numpy(), ksb[slots].cpu().numpy()[:, None])
    return k, np.ascontiguousarray(k[..., :RANK])


@dataclasses.dataclass
class Batch:
    rows: list
    lens: tuple            # before the new token
    loc: torch.Tensor      # the new token's slots
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    aux: Optional[torch.Tensor]
    prefix_loc: torch.Tensor
    prefix_kv: list        # per layer (k rows, v rows)
    table: list            # per request: its req_to_token row up to and including the new slot

    @property
    def seq(self):
        return [n + 1 for n in self.lens]


class Rig:
    """Mock runner + backend + two layers for one config; `start` captures, `step` replays one live batch and asserts."""

    def __init__(self, cfg: Config, index_mode: str, max_reqs: int = 8, scratch: bool = True):
        from sglang_amd.attention.backend import HipRadixAttnBackend
        from sglang_amd.attention.radix_attention import RadixAttention
        from sglang_amd.mem_cache.allocator import PagedTokenToKVPoolAllocator, TokenToKVPoolAllocator
        from sglang_amd.mem_cache.memory_pool import ReqToTokenPool

        self.cfg, self.index_mode = cfg, index_mode
        self.pool = make_pool(cfg)
        self.scratch = make_pool(cfg) if scratch else None
        self.r2t = ReqToTokenPool(max_reqs, MAX_CTX, DEV)
        self.gen = torch.Generator().manual_seed(17)
        if cfg.page == 1:
            self.alloc = TokenToKVPoolAllocator(POOL_SLOTS, cfg.dtype, DEV, self.pool)
        else:
            self.alloc = PagedTokenToKVPoolAllocator(POOL_SLOTS, cfg.page, cfg.dtype, DEV, self.pool, debug_mode=True)
            fp = self.alloc.free_pages
            self.alloc.free_pages = fp[torch.randperm(len(fp), generator=self.gen).to(DEV)]
        r2t, pool, alloc = self.r2t, self.pool, self.alloc

        class MC:
            num_attention_heads, num_key_value_heads, context_len = cfg.hq, cfg.hkv, MAX_CTX

        class MR:
            device, req_to_token_pool, token_to_kv_pool, token_to_kv_pool_allocator = DEV, r2t, pool, alloc
            model_config, page_size, dtype = MC, cfg.page, cfg.dtype
            sliding_window_size = cfg.window or None

            class server_args:
                triton_attention_num_kv_splits = 8
                enable_deterministic_inference = cfg.det

        self.runner = MR
        self.be = HipRadixAttnBackend(MR, decode_index_mode=index_mode, split_policy=cfg.policy)
        scaling = (128 + ROPE) ** -0.5 if cfg.latent else cfg.dk ** -0.5
        self.layers = []
        for i in range(2):
            layer = RadixAttention(cfg.hq, cfg.dk, scaling, cfg.hkv, i, logit_cap=cfg.logit_cap, v_head_dim=cfg.v,
                                   sliding_window_size=cfg.window if (cfg.window and i == 1) else -1)
            if cfg.xai:
                layer.xai_temperature_len = cfg.xai
            if cfg.scales:   # a loaded model: device tensors + the floats cached next to them
                layer.k_scale, layer.v_scale = (torch.tensor(s, device=DEV) for s in cfg.scales)
                layer.k_scale_float, layer.v_scale_float = cfg.scales
            self.layers.append(layer)
        self.sinks = torch.randn(cfg.hq, generator=self.gen).to(DEV) if cfg.sinks else None
        self.record = []          # per step: (name, split step?, bit-identical to eager?)

    # ---- data and slots --------------------------------------------------------------------------------------------
    def rand(self, *shape, mul=1.0):
        return (torch.randn(*shape, generator=self.gen) * mul).to(self.cfg.dtype).to(DEV)

    def store(self, pool, layer, loc, k, v):
        if self.cfg.latent:
            pool.set_kv_buffer(layer, loc, k.reshape(loc.numel(), 1, self.cfg.dk))
        else:
            pool.set_kv_buffer(layer, loc, k.reshape(loc.numel(), self.cfg.hkv, self.cfg.dk),
                               v.reshape(loc.numel(), self.cfg.hkv, self.cfg.v), *(self.cfg.scales or ()))

    def grow(self, rows, old, new):
        """alloc_for_extend: slots from the allocator, req_to_token rows through rx_write_req_to_token."""
        from sglang_amd import ops

        o_, n_ = torch.tensor(old, dtype=torch.int64), torch.tensor(new, dtype=torch.int64)
        n = int((n_ - o_).sum())
        if self.cfg.page == 1:
            out = self.alloc.alloc(n)
        else:
            tab = self.r2t.req_to_token[rows].cpu()
            last = torch.tensor([int(tab[i, p - 1]) if p > 0 else -1 for i, p in enumerate(old)], dtype=torch.int64, device=DEV)
            out = self.alloc.alloc_extend(o_.to(DEV), o_, n_.to(DEV), n_, last, n)
        assert out is not None
        ops.write_req_to_token(self.r2t.req_to_token, torch.tensor(rows, dtype=torch.int64, device=DEV), None,
                               o_.to(DEV), n_.to(DEV), (n_ - o_).to(DEV), out)
        return out

    def prepare(self, rows, lens) -> Batch:
        """One live batch: prefixes allocated and stored in both layers, then alloc_for_decode (allocation.py:578-580:
        the new slot sits at req_to_token[req, seq_len - 1] before the forward)."""
        cfg, live = self.cfg, len(lens)
        rows = list(rows[:live])
        ploc = self.grow(rows, [0] * live, list(lens))
        pkv = []
        for layer in self.layers:
            kv = (self.rand(sum(lens), cfg.hkv * cfg.dk), None if cfg.latent else self.rand(sum(lens), cfg.hkv * cfg.v))
            self.store(self.pool, layer, ploc, *kv)
            pkv.append(kv)
        seq = torch.tensor([n + 1 for n in lens], dtype=torch.int64)
        rpi = torch.tensor(rows, dtype=torch.int64, device=DEV)
        if cfg.page == 1:
            loc = self.alloc.alloc(live)
        else:
            last = self.r2t.req_to_token[rpi, torch.tensor(lens, device=DEV) - 1].to(torch.int64)
            loc = self.alloc.alloc_decode(seq.to(DEV), seq, last)
        assert loc is not None
        self.r2t.req_to_token[rpi, torch.tensor(lens, device=DEV)] = loc.to(torch.int32)
        q = self.rand(live, cfg.hq * cfg.dk, mul=4.0 if cfg.logit_cap else 1.0)   # (the cap must bite: logits of +-10 and more)
        k = self.rand(live, cfg.hkv * cfg.dk)
        v = k.view(live, cfg.hkv, cfg.dk)[..., :RANK] if cfg.latent else self.rand(live, cfg.hkv * cfg.v)
        aux = (1.5 * torch.randn(live, cfg.hq, EXTENT, generator=self.gen)).to(DEV) if cfg.relbias else None
        table = [self.r2t.req_to_token[r, : n + 1].clone() for r, n in zip(rows, lens)]
        return Batch(rows, tuple(lens), loc, q, k, v, aux, ploc, pkv, table)

    def restore(self, b: Batch):
        """The same batch once more, into the same slots and rows (everything else has been freed by now)."""
        for r, t in zip(b.rows, b.table):
            self.r2t.req_to_token[r, : t.numel()] = t
        for layer, kv in zip(self.layers, b.prefix_kv):
            self.store(self.pool, layer, b.prefix_loc, *kv)

    def free(self, b: Batch):
        for t in b.table:
            self.alloc.free(t.to(torch.int64))

    # ---- capture ---------------------------------------------------------------------------------------------------
    def start(self):
        """decode_cuda_graph_runner.py: static inputs filled with row 0 / the fill value / slot 0, metadata with
        in_capture=True, warm-up on a side stream, both layers in one graph."""
        from sglang_amd import lib as rxlib
        from sglang_amd import ops
        from sglang_amd.forward_batch import ForwardBatch

        cfg, be = self.cfg, self.be
        be.init_cuda_graph_state(8, 8)
        self.fill = be.get_cuda_graph_seq_len_fill_value()
        self.s_rpi = torch.zeros(B, dtype=torch.int64, device=DEV)
        self.s_seq = torch.full((B,), self.fill, dtype=torch.int64, device=DEV)
        self.s_loc = torch.zeros(B, dtype=torch.int64, device=DEV)
        self.q, self.k = self.rand(B, cfg.hq * cfg.dk), self.rand(B, cfg.hkv * cfg.dk)
        self.v = self.k.view(B, cfg.hkv, cfg.dk)[..., :RANK] if cfg.latent else self.rand(B, cfg.hkv * cfg.v)
        self.aux = torch.zeros(B, cfg.hq, EXTENT, device=DEV) if cfg.relbias else None
        self.kw = {}
        if cfg.sinks:
            self.kw["sinks"] = self.sinks
        if cfg.relbias:
            self.kw.update(score_mod=ops.relative_bias_score_mod, aux_tensors=[self.aux])
        fb_g = ForwardBatch.for_decode(self.s_rpi, self.s_seq, self.s_loc, torch.full((B,), self.fill, dtype=torch.int64))
        be.init_forward_metadata_out_graph(fb_g, in_capture=True)
        self.graph, self.outs = capture(lambda: tuple(layer(self.q, self.k, self.v, fb_g, be, **self.kw) for layer in self.layers))
        name = rxlib.last_dispatch()
        assert name.startswith(cfg.family), (cfg.id, name)
        self.rows = self.r2t.alloc(B)

    # ---- one replay ------------------------------------------------------------------------------------------------
    def _oracle(self, layer, b: Batch):
        cfg = self.cfg
        tab = self.r2t.req_to_token.cpu().numpy()
        W = layer.sliding_window_size if (layer.sliding_window_size or -1) > 0 else 0
        pieces, indptr = [], [0]
        for r, n in zip(b.rows, b.seq):
            w = min(n, W) if W else n   # the last min(len, W) tokens, the new one among them (triton_backend.py:2043-2110)
            pieces.append(tab[r, n - w: n])
            indptr.append(indptr[-1] + w)
        slots = torch.from_numpy(np.concatenate(pieces).astype(np.int64)).to(DEV)
        kf, vf = held_rows(cfg, self.pool, layer.layer_id, slots)
        ks, vs = cfg.scales or (1.0, 1.0)
        live = len(b.rows)
        return orc.decode_attention(
            b.q.view(live, cfg.hq, cfg.dk).float().cpu().numpy(), kf, vf, np.array(indptr, dtype=np.int64),
            np.arange(slots.numel(), dtype=np.int64), layer.scaling, k_scale=ks, v_scale=vs, logit_cap=cfg.logit_cap,
            sinks=None if self.sinks is None else self.sinks.double().cpu().numpy(), xai_temperature_len=cfg.xai or -1,
            score_bias=None if b.aux is None else b.aux.double().cpu().numpy(), return_absw=True)

    def _check_store(self, b: Batch, snap, table_snap, who):
        """The step's rows equal, as bytes, set_kv_buffer's on a scratch pool of the same class; every other slot but
        page 0 (the padding sink) and all of req_to_token are the snapshot's."""
        assert torch.equal(self.r2t.req_to_token, table_snap), (self.cfg.id, who, "req_to_token changed")
        for (_, s), (_, t) in zip(pool_buffers(self.scratch), snap):
            s.copy_(t)
        for layer in self.layers:
            self.store(self.scratch, layer, b.loc, b.k, b.v)
        skip = 1 if self.pool.use_hnd else self.pool.page_size
        for (name, got), (_, want) in zip(pool_buffers(self.pool), pool_buffers(self.scratch)):
            if not torch.equal(got[skip:], want[skip:]):
                bad = (got[skip:] != want[skip:]).reshape(got.shape[0] - skip, -1).any(1).nonzero().flatten() + skip
                raise AssertionError((self.cfg.id, who, name, "first-dim indices that differ from snapshot + set_kv_buffer",
                                      bad[:8].tolist(), "new slots", b.loc.tolist()))

    def step(self, name: str, b: Batch):
        from sglang_amd.forward_batch import ForwardBatch

        cfg, be, live = self.cfg, self.be, len(b.rows)
        rpi = torch.tensor(b.rows, dtype=torch.int64, device=DEV)
        seq = torch.tensor(b.seq, dtype=torch.int64)
        # padding rows: request row 0, the fill value, slot 0; their q / k / v are whatever the buffers held
        self.s_rpi.zero_(); self.s_seq.fill_(self.fill); self.s_loc.zero_()
        self.s_rpi[:live] = rpi; self.s_seq[:live] = seq.to(DEV); self.s_loc[:live] = b.loc
        self.q[:live].copy_(b.q); self.k[:live].copy_(b.k)
        if not cfg.latent:
            self.v[:live].copy_(b.v)
        if b.aux is not None:
            self.aux[:live].copy_(b.aux)     # in place: the captured kernels hold the table's address
        seq_cpu = torch.full((B,), self.fill, dtype=torch.int64)
        seq_cpu[:live] = seq
        snap = [(n_, t.clone()) for n_, t in pool_buffers(self.pool)]
        table_snap = self.r2t.req_to_token.clone()
        be.init_forward_metadata_out_graph(ForwardBatch.for_decode(self.s_rpi, self.s_seq, self.s_loc, seq_cpu))
        self.graph.replay()
        torch.cuda.synchronize()
        got = [o[:live].clone() for o in self.outs]
        counts_g = self._counts(live)
        self._check_store(b, snap, table_snap, (name, "replay"))
        wants = [self._oracle(layer, b) for layer in self.layers]
        for layer, o, (want, absw) in zip(self.layers, got, wants):
            self._parity(o, want, absw, (cfg.id, self.index_mode, name, "replay", layer.layer_id))
        # the eager twin: the same batch through init_forward_metadata and the two layers
        fb_e = ForwardBatch.for_decode(rpi, seq.to(DEV), b.loc, seq)
        be.init_forward_metadata(fb_e)
        kw = dict(self.kw)
        if b.aux is not None:
            kw["aux_tensors"] = [b.aux]
        eager = [layer(b.q, b.k, b.v, fb_e, be, **kw) for layer in self.layers]
        torch.cuda.synchronize()
        counts_e = self._counts(live)
        for layer, o, (want, absw) in zip(self.layers, eager, wants):
            self._parity(o, want, absw, (cfg.id, self.index_mode, name, "eager", layer.layer_id))
        same = len(counts_g) == len(counts_e) and all(torch.equal(a, c) for a, c in zip(counts_g, counts_e))
        split = any(int(c.max()) > 1 for c in counts_g)
        if same:
            for layer, o, e in zip(self.layers, got, eager):
                assert torch.equal(o, e), (cfg.id, self.index_mode, name, "layer", layer.layer_id,
                                           "same num_kv_splits as the eager step, different bits",
                                           (o.float() - e.float()).abs().max().item())
        self._check_store(b, snap, table_snap, (name, "eager"))
        assert self.pool.check_errors() == 0
        self.record.append((name, split, same))
        return got

    def _counts(self, live):
        md = self.be.forward_metadata
        return [t[:live].clone() for t in (md.num_kv_splits, md.window_num_kv_splits) if t is not None]

    def _parity(self, o, want, absw, tag):
        cfg = self.cfg   # ulps=1 with the |V| term: what the eager test of every one of these pools and layer kinds states
        parity.check_out(o.view(-1, cfg.hq, cfg.v).float().cpu().numpy(), want, cfg.dtype, tag, ulps=1, absw=absw)

    def finish(self):
        """At least one SPLIT step of the config ran the eager step's schedule and was held to its bits."""
        _write({"config": self.cfg.id, "index_mode": self.index_mode,
                "steps": [dict(step=n_, split=s, bit_identical_to_eager=e) for n_, s, e in self.record]})
        assert any(s and e for _, s, e in self.record), (self.cfg.id, self.index_mode, self.record)


def _write(rec):
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def run_script(cfg: Config, index_mode: str):
    """Capture once, then R1, R2, R3 (padded), R4, R4 again, R1 again -- all through the one graph."""
    rig = Rig(cfg, index_mode)
    rig.start()
    outs, first = {}, None
    for name, lens in SCRIPT:
        if name == "R1" and cfg.window:
            lens = SWA_R1
        b = rig.prepare(rig.rows, lens)
        outs[name] = rig.step(name, b)
        if name == "R1":
            first = b
        if name == "R4":
            again = rig.step("R4'", b)    # nothing changed but what the eager twin left behind
            for x, y in zip(outs["R4"], again):
                assert torch.equal(x, y), (cfg.id, index_mode, "R4 replayed again differs")
        rig.free(b)
    rig.restore(first)
    again = rig.step("R1'", first)
    for x, y in zip(outs["R1"], again):
        assert torch.equal(x, y), (cfg.id, index_mode, "R1 rebuilt into the same slots differs from R1")
    rig.finish()
    return rig


# ---------------------------------------------------------------------------------------------------------------------
# the metadata alone, at every batch size the runner can capture
# ---------------------------------------------------------------------------------------------------------------------
def _tensors_of(obj, prefix, out, depth=0):
    if torch.is_tensor(obj):
        out.append((prefix, obj))
    elif isinstance(obj, dict):
        for key, val in obj.items():
            _tensors_of(val, f"{prefix}[{key!r}]", out, depth)
    elif isinstance(obj, (list, tuple)):
        for i, val in enumerate(obj):
            _tensors_of(val, f"{prefix}[{i}]", out, depth)
    elif depth < 1 and hasattr(obj, "__dict__") and not isinstance(obj, (type, types.ModuleType, types.FunctionType)):
        for key, val in vars(obj).items():
            _tensors_of(val, f"{prefix}.{key}", out, depth + 1)


def metadata_tensors(md):
    """Every tensor of a ForwardMetadata: its dataclass fields, and the tensor attributes of the objects they hold
    (ops.SplitItems, ops.DecodeUnits)."""
    out = []
    for f in dataclasses.fields(md):
        _tensors_of(getattr(md, f.name), f.name, out)
    return out


def _span(t):
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    ext = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
    return t.data_ptr(), t.data_ptr() + ext * t.element_size()


def _storage_span(t):
    st = t.untyped_storage()
    return st.data_ptr(), st.data_ptr() + st.nbytes()


def metadata_sweep(cfg: Config, index_mode: str, max_bs: int = 64):
    from sglang_amd.forward_batch import ForwardBatch

    rig = Rig(cfg, index_mode, max_reqs=max_bs, scratch=False)
    be = rig.be
    be.init_cuda_graph_state(max_bs, max_bs)
    fill = be.get_cuda_graph_seq_len_fill_value()
    s_rpi = torch.zeros(max_bs, dtype=torch.int64, device=DEV)
    s_seq = torch.full((max_bs,), fill, dtype=torch.int64, device=DEV)
    s_loc = torch.zeros(max_bs, dtype=torch.int64, device=DEV)
    # where a piece of metadata may live: be._graph, the backend's persistent attributes as they stand now, our buffers
    known = []
    _tensors_of(vars(be), "be", known)
    _tensors_of(be._graph, "be._graph", known)
    for key, val in be._graph.items():
        _tensors_of(val, f"be._graph[{key!r}]", known)
    known += [("s_rpi", s_rpi), ("s_seq", s_seq), ("s_loc", s_loc)]
    homes = sorted({_storage_span(t) for _, t in known if t.is_cuda})
    rng = np.random.RandomState(7)
    keep = []   # every metadata object stays alive: a freed tensor's address could be handed out again
    for bs in range(1, max_bs + 1):
        s_rpi[:bs] = torch.arange(1, bs + 1, device=DEV)
        seen = None
        for kind in ("fill", "random", "max"):
            if kind == "fill":
                lens = np.full(bs, fill, dtype=np.int64)
            elif kind == "max":
                lens = np.full(bs, MAX_CTX, dtype=np.int64)
            else:
                lens = rng.randint(1, MAX_CTX + 1, size=bs).astype(np.int64)
                lens[rng.randint(bs)] = MAX_CTX
            seq_cpu = torch.from_numpy(lens)
            s_seq[:bs] = seq_cpu.to(DEV)
            be.init_forward_metadata_out_graph(ForwardBatch.for_decode(s_rpi[:bs], s_seq[:bs], s_loc[:bs], seq_cpu))
            md = be.forward_metadata
            keep.append(md)
            where = (cfg.id, index_mode, "bs", bs, kind)
            found = metadata_tensors(md)
            layout = [(n_, t.data_ptr(), tuple(t.shape), tuple(t.stride())) for n_, t in found]
            assert seen is None or layout == seen, (where, "address / shape / stride moved with the lengths",
                                                    [a for a, c in zip(layout, seen) if a != c][:4])
            seen = layout
            for n_, t in found:
                lo, hi = _span(t)
                assert lo == hi or any(a <= lo and hi <= z for a, z in homes), (
                    where, n_, "lies outside be._graph, the backend's persistent buffers and the static inputs")
            counted = [t for t in (md.num_kv_splits, md.window_num_kv_splits) if t is not None]
            if counted:
                host = torch.stack([t[:bs] for t in counted]).cpu().numpy()   # the one read-back of this call
                assert host.min() >= 1 and host.max() <= md.max_kv_splits, (where, host.max(), md.max_kv_splits)
                if md.split_items is not None:
                    assert int(host[0].sum()) <= md.split_items.cap <= md.split_items.items.numel() // 2, (
                        where, int(host[0].sum()), md.split_items.cap)
                if md.attn_logits is not None:
                    assert md.attn_logits.shape[0] >= bs and md.attn_logits.shape[2] >= md.max_kv_splits, where
    items = be._graph.get("split_items")
    if items is not None:   # sticky: set by a guarded build that had to replace a schedule its table could not hold
        assert int(items.overflow.item()) == 0, (cfg.id, index_mode, "split_pairs_bound was outgrown")
