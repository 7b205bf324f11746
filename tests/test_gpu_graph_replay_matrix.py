"""Graph-replayed decode on every KV pool and layer kind.

When serving, every decode step runs from a captured HIP graph: the runner captures once per batch size with seq_lens at
the fill value, and before every replay copies the live batch into address-stable buffers and calls
init_forward_metadata_out_graph (decode_cuda_graph_runner.py:946-953, :1168).  Captured kernels read pointers frozen at
capture time.  `graph_replay_util.run_script` drives HipRadixAttnBackend exactly so -- one graph of TWO layers at batch
size 4 over pools with layer_num = 2 -- and replays it over R1 (mixed), R2 (a long request, page ends, a length-1
request), R3 (two live rows + two padding rows), R4 (everyone one pass), R4 again and R1 rebuilt into its slots.  After
every replay, for the live rows: both layers meet the fp64 oracle fed the bytes the pool holds (ulps = 1 with the |V|
term, what the eager test of each pool and layer kind states); the eager twin meets it too and, where its num_kv_splits
equal the replay's element for element, the outputs are bit-identical (at least one SPLIT step per config must be:
`Rig.finish`; every step's branch is written to graph_replay_matrix.jsonl next to parity_util's log); the step's K / V rows equal
set_kv_buffer's bytes on a scratch pool while every other slot but page 0 -- the padding sink -- and all of req_to_token
equal a snapshot; pool.check_errors() == 0; and rx_last_dispatch() after the capture names the kernel family the config
is meant to reach.  `metadata_sweep` then calls init_forward_metadata_out_graph alone at every batch size 1 .. 64.

Which steps took the bit-identical branch on the MI355X (256 CUs): R1, R2, R3 and the rebuilt R1 -- all of them split
steps -- in EVERY config and index mode, the padded R3 included (its two live rows get the counts the two-request eager
batch gets); R4 and its second replay as well in det, static-splits, ref-policy and swa-w64, whose schedules keep a
count tensor for a one-pass batch.  Under the native schedule the eager R4 carries no num_kv_splits at all (S = 1: the
plain launch) while the replay carries a tensor of ones, so R4 is held to the oracle, the store and its own second
replay only.

Refused under graph metadata as everywhere (REFUSED below): a 4-bit pool with a sliding-window layer, score_mod or draft
decode.  Out of scope here: DCP decode (several processes), cascade / draft / verify (tests/test_gpu_cascade.py,
test_gpu_draft_decode.py and test_gpu_backend.py hold their graph cases), the ops-level fused-RoPE latent decode, and
extends of every kind."""
import types

import pytest
import torch

import graph_replay_util as gr
from graph_replay_util import Config

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
MLA = dict(hq=16, hkv=1, dk=gr.RANK + gr.ROPE, dv=gr.RANK)
CONFIGS = [
    Config("bf16-d128"),                                                     # fused store; padding; two layers
    Config("f16-d64", hq=4, hkv=4, dk=64, dtype=torch.float16),              # fused store, MHA
    Config("bf16-d96", dk=96),                                               # MFMA split-KV, no fused store
    Config("bf16-d256", dk=256),
    Config("bf16-d192v128", hq=4, hkv=1, dk=192, dv=128, family=("decode_generic_kernel",)),   # bs x slots grid
    Config("bf16-g20", hq=20, hkv=1),                                        # two workgroups per request, no fused store
    Config("fp8-d128", pool_dtype=FP8, scales=(0.75, 1.5)),                  # separate quantising store in the graph
    Config("hnd-bf16", hnd=True),
    Config("page1", page=1),                                                 # token allocator
    Config("page64", page=64),                                               # one page holds R1's short requests
    Config("mx4-nhd", kind="mx4", family=("decode_mx4_kernel",)),
    Config("mx4-hnd", kind="mx4", hnd=True, family=("decode_mx4_kernel",)),
    Config("mx4-d64", kind="mx4", hq=4, hkv=4, dk=64, family=("decode_mx4_kernel",)),
    Config("mla-bf16", kind="mla", family=("decode_mla_kernel",), **MLA),
    Config("mla-fp8", kind="mla", pool_dtype=FP8, family=("decode_mla_kernel", "decode_mla8_"), **MLA),
    Config("mla-mx4", kind="mla-mx4", family=("decode_mla_mx4_kernel",), **MLA),
    Config("swa-w64", window=64),                                            # window buffers live in be._graph
    Config("sinks", sinks=True),
    Config("logitcap", logit_cap=30.0),
    Config("xai", xai=512),
    Config("relbias", relbias=True, family=("decode_mfma_bias_kernel",)),    # the aux table is rewritten in place per step
    Config("det", det=True),
    Config("static-splits", static=True),
    Config("ref-policy", policy="reference"),
]
BY_ID = {c.id: c for c in CONFIGS}
BOTH_MODES = ("fp8-d128", "mla-bf16", "swa-w64")
MATRIX = [(c.id, "paged") for c in CONFIGS] + [(i, "indices") for i in BOTH_MODES]
SWEEP = [("bf16-d128", "paged"), ("bf16-g20", "paged"), ("bf16-d192v128", "paged"), ("fp8-d128", "indices"),
         ("mx4-nhd", "paged"), ("mla-fp8", "paged"), ("swa-w64", "paged")]


def _env(cfg, monkeypatch):
    if cfg.static:
        monkeypatch.setenv("SGLANG_TRITON_DECODE_ATTN_STATIC_KV_SPLITS", "true")


@pytest.mark.parametrize("cid,index_mode", MATRIX, ids=[f"{c}-{m}" for c, m in MATRIX])
def test_replayed_decode_matches_oracle_eager_twin_and_store(cid, index_mode, monkeypatch):
    cfg = BY_ID[cid]
    _env(cfg, monkeypatch)
    rig = gr.run_script(cfg, index_mode)
    assert rig.be.static_kv_splits == cfg.static and rig.be.enable_deterministic == cfg.det
    assert [n for n, _, _ in rig.record] == ["R1", "R2", "R3", "R4", "R4'", "R1'"]


@pytest.mark.parametrize("cid,index_mode", SWEEP, ids=[f"{c}-{m}" for c, m in SWEEP])
def test_graph_metadata_at_every_batch_size_stays_in_its_buffers(cid, index_mode):
    """No attention launch: for bs = 1 .. 64 and lengths all fill / random with one at the maximum / all at the maximum,
    init_forward_metadata_out_graph raises nothing (a view that does not fit its be._graph buffer would), returns
    every tensor at one address, shape and stride whatever the lengths, inside be._graph / the backend's persistent
    buffers / the static inputs, and hands out counts within the slots and the (request, split) table."""
    gr.metadata_sweep(BY_ID[cid], index_mode)


# what the backend refuses by name on a 4-bit pool -- under graph metadata too
REFUSED = [("window", "sliding-window"), ("score_mod", "score_mod is not supported on a 4-bit"), ("draft", "draft decode")]


@pytest.mark.parametrize("what,text", REFUSED, ids=[w for w, _ in REFUSED])
@pytest.mark.parametrize("cid", ["mx4-nhd", "mla-mx4"])
def test_refused_on_a_4bit_pool_under_graph_metadata(cid, what, text):
    from sglang_amd import ops
    from sglang_amd.attention.backend import HipRadixAttnBackend
    from sglang_amd.attention.radix_attention import RadixAttention
    from sglang_amd.forward_batch import ForwardBatch

    cfg = BY_ID[cid]
    rig = gr.Rig(cfg, "paged", scratch=False)
    be = rig.be
    be.init_cuda_graph_state(8, 8)
    fill = be.get_cuda_graph_seq_len_fill_value()
    zeros = torch.zeros(gr.B, dtype=torch.int64, device=gr.DEV)
    fb = ForwardBatch.for_decode(zeros, torch.full_like(zeros, fill), zeros.clone(), torch.full((gr.B,), fill, dtype=torch.int64))
    layer, kw = rig.layers[0], {}
    if what == "window":
        rig.runner.sliding_window_size = 64
        with pytest.raises(NotImplementedError, match=text):
            HipRadixAttnBackend(rig.runner)
        layer = RadixAttention(cfg.hq, cfg.dk, layer.scaling, cfg.hkv, 0, v_head_dim=cfg.v, sliding_window_size=64)
    elif what == "score_mod":
        kw = dict(score_mod=ops.relative_bias_score_mod, aux_tensors=[torch.zeros(gr.B, cfg.hq, gr.EXTENT, device=gr.DEV)])
    else:
        fb.spec_info = types.SimpleNamespace(kv_indptr=torch.zeros(gr.B + 1, dtype=torch.int32, device=gr.DEV),
                                             kv_indices=torch.zeros(1, dtype=torch.int64, device=gr.DEV))
    be.init_forward_metadata_out_graph(fb, in_capture=True)
    q, k = rig.rand(gr.B, cfg.hq * cfg.dk), rig.rand(gr.B, cfg.hkv * cfg.dk)
    v = k.view(gr.B, cfg.hkv, cfg.dk)[..., :gr.RANK] if cfg.latent else rig.rand(gr.B, cfg.hkv * cfg.v)
    with pytest.raises(NotImplementedError, match=text):
        layer(q, k, v, fb, be, **kw)
