// MLA (absorbed) decode attention over 4-bit latent rows (MXFP4, blocks of 16; include/radix_hip.h "4-bit KV pool"):
// Dk = 576 (512 latent + 64 rope), Dv = 512, one kv head, V = the first 512 columns of the SAME rows.  A row is 288 data
// bytes + 36 scale bytes = 324 B (1152 B in bf16, 576 B in fp8).
//
// Reference: MLATokenToKVPoolFP4 (srt/mem_cache/memory_pool.py:4182-4319), whose get_key_buffer runs
// FP4MXBlock16KVQuantizeUtil.batched_dequantize (srt/layers/quantization/kvfp4_tensor.py:105-147) over the WHOLE layer on
// every call before the 16-bit decode kernel reads it.
//
// Work split: launch_decode_mla's (rx_decode_mla.hip).  One 256-thread workgroup = one (request, 16-head q block, kv
// split); a (request, split) pair is bound to one XCD and its q blocks follow each other there.
//
// Data path of a 32-token tile (10 368 packed bytes):
//   * HBM -> VGPR.  A PIECE is 16-byte data chunk c of a row = elements 32 c .. 32 c + 31 = scale blocks 2 c, 2 c + 1.
//     18 pieces per row, 576 per tile: thread tid takes pieces tid and tid + 256, threads 0..63 also piece tid + 512
//     (consecutive lanes read consecutive 16 bytes of a row).  The piece's two scale bytes are ONE 16-bit load from an
//     address of their own (scale rows are 36 B: the pair is 2-byte aligned), issued with the data load: no load waits
//     for another.  5 VGPRs per piece; RX_MLA_MX4_DEPTH register sets = that many tiles in flight ahead of the image.
//   * unpack in registers: mx4x8_to_16 (four v_cvt_scalef32_pk_{bf16,f16}_fp4 per dword, scale byte << 23 as the f32
//     scale operand).  Exact.
//   * VGPR -> LDS: four ds_write_b128 per piece into the 16-bit image of decode_mla_kernel (rows padded to kMlaLdsRow
//     = 1184 B: conflict-free for the ds_read_b128 K fragments and the ds_read_b64_tr_b16 V^T reads).  Neighbouring
//     lanes' pieces are 64 B apart, so write j of lane (row, c) carries sub-chunk j ^ ((c >> 1) & 3): eight consecutive
//     lanes then cover eight different 16-byte bank groups instead of two.
//   * from the image on, the 16-bit kernel's arithmetic: S^T = K Q^T on v_mfma_f32_16x16x32 with the 16 q heads on the N
//     axis (cut four ways over the waves, partial sums exchanged through LDS in one fixed order), the sum-checked softmax
//     against the standing maximum, P as the next B operand, each wave owning 128 of the 512 output columns.
// One image serves both products and every HBM byte is read once.  As for fp8 rows the per-tile latency
// chain, not HBM, sets the rate at this few bytes: ONE image in LDS (41 KB) and THREE workgroups per CU.
//
// Why not the hardware's 4-bit paths: the scaled MFMA (v_mfma_scale_f32_*_f8f6f4) applies one scale per 32 contraction
// elements and this format has one per 16 -- feeding it means re-quantising (not exact) or splitting every k-step; a
// 4-bit LDS image read by ds_read_b64_tr_b4 has the same problem on the PV side.
#include "rx_common.h"
#include "rx_decode_common.h"
#include "rx_mla_common.h"
#include "rx_mx4_common.h"

namespace rx {

#ifndef RX_MLA_MX4_DEPTH
#define RX_MLA_MX4_DEPTH 2  // packed tiles in flight in registers ahead of the LDS image
#endif
#ifndef RX_MLA_MX4_PD
#define RX_MLA_MX4_PD 4  // K-fragment prefetch distance (LDS reads in flight ahead of the MFMA)
#endif

struct MlaMx4Args {
  const uint16_t* q;
  uint16_t* o;
  int64_t q_stride_t, q_stride_h, o_stride_t, o_stride_h;
  Mx4Pool kv;         // (one kv head: the head strides are not used)
  int32_t page_size;  // >= 1, or -(log2(page) + 1) for a power-of-two page (slot_offset)
  const int32_t* kv_indptr;
  const void* kv_indices;
  const int32_t* req_to_token;
  int64_t req_row_stride;
  const void* req_pool_indices;
  int32_t rpi64;
  const void* seq_lens;
  int32_t sl64;
  const int32_t* num_kv_splits;
  int32_t max_kv_splits;
  float* attn_logits;
  float* attn_lse;
  int32_t bs, hq, qblocks;
  float sm_scale;  // sm_scale * k_scale
  float v_scale, logit_cap;
  const float* sinks;
  int32_t xai_len;
};

constexpr int kMx4Ppr = kMlaDk / 32;                      // 18 pieces per row
constexpr int kMx4Pieces = kMlaTile * kMx4Ppr;            // 576 per tile
constexpr int kMx4Passes = (kMx4Pieces + 255) / 256;      // 3 (the last one: threads 0..63)
constexpr int kMx4Lds = kMlaTile * kMlaLdsRow + 4 * 64 * 16;  // the image + the 4 x 1 KiB score exchange

template <typename T, typename IdxT, bool LINEAR>
__global__ __launch_bounds__(256, 3) void decode_mla_mx4_kernel(const MlaMx4Args a) {
  using vec8 = typename T::vec8;
  constexpr int KS = kMlaDk / 32;       // 18 k-steps
  constexpr int NBW = kMlaDv / 16 / 4;  // 8 d-blocks of 16 per wave
  constexpr int KSW = KS / 2;           // k-steps of this wave's score part
  constexpr int NST = kMx4Passes;
  constexpr int DEPTH = RX_MLA_MX4_DEPTH;
  __shared__ __attribute__((aligned(16))) char smem[kMx4Lds];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;

  int qb, b, split;
  {
    const int G = a.qblocks;
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    qb = j % G;
    const int pr = (j / G) * 8 + xcd;  // (request, split) pair, bound to one XCD
    if (pr >= a.bs * a.max_kv_splits) return;
    b = pr % a.bs;
    split = pr / a.bs;
  }
  int32_t seq_len;
  const IdxT* idx;
  if (a.kv_indices) {
    const int32_t beg = a.kv_indptr[b];
    seq_len = a.kv_indptr[b + 1] - beg;
    idx = reinterpret_cast<const IdxT*>(a.kv_indices) + beg;
  } else {  // IdxT == int32_t in this mode
    seq_len = static_cast<int32_t>(load_idx(a.seq_lens, b, a.sl64));
    idx = reinterpret_cast<const IdxT*>(a.req_to_token + load_idx(a.req_pool_indices, b, a.rpi64) * a.req_row_stride);
  }
  const int32_t splits = (a.num_kv_splits && a.max_kv_splits > 1) ? a.num_kv_splits[b] : 1;
  const bool single = a.max_kv_splits == 1 || splits == 1;  // (direct_single: see decode_mx4_kernel)
  const int h = qb * 16 + r;
  const bool q_valid = h < a.hq;
  if (split >= splits) return;
  int32_t lo, hi;
  split_range(seq_len, splits, split, lo, hi);
  if (hi <= lo) {
    if (single && seq_len == 0)  // empty request: define the output
      for (int i = tid; i < 16 * kMlaDv; i += 256) {
        const int q = i / kMlaDv, d = i % kMlaDv;
        if (qb * 16 + q < a.hq) a.o[b * a.o_stride_t + (qb * 16 + q) * a.o_stride_h + d] = 0;
      }
    return;
  }
  const int ntiles = (hi - lo + kMlaTile - 1) / kMlaTile;

  // ---- Q^T fragments: wave w computes token block (w & 1) over k-steps [9 (w >> 1), +9) ------------------------------
  const int ks0 = KSW * (w >> 1);
  vec8 qf[KSW];
  {
    const uint16_t* qp = a.q + b * a.q_stride_t + (q_valid ? h : 0) * a.q_stride_h + 8 * g + 32 * ks0;
#pragma unroll
    for (int s = 0; s < KSW; ++s) {
      const u32x4 raw = q_valid ? *reinterpret_cast<const u32x4*>(qp + 32 * s) : u32x4{0, 0, 0, 0};
      qf[s] = __builtin_bit_cast(vec8, raw);
    }
  }
  // Q must have landed before the loop (rx_decode_mla.hip: otherwise the loop header waits for vmcnt(0) every iteration)
  __builtin_amdgcn_s_waitcnt(0x0F70);

  // ---- staging: pieces tid + 256 i -------------------------------------------------------------------------------------
  // One VGPR per pass holds the piece's coordinate (row << 5 | chunk).  coord() hands it out OPAQUE: hipcc otherwise hoists
  // every address built from it out of the tile loop (64-bit global bases, four LDS write addresses per pass: ~30 VGPRs,
  // which at three workgroups per CU is scratch); redone per tile it is a dozen VALU per piece.
  int pc[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) {
    const int c = min(tid + 256 * i, kMx4Pieces - 1);  // the partial last pass re-reads the last piece
    pc[i] = (c / kMx4Ppr) << 5 | (c % kMx4Ppr);
  }
  auto coord = [&](int i, int& row, int& col) {
    int c = pc[i];
    asm volatile("" : "+v"(c));
    row = c >> 5;
    col = c & 31;
  };
  const bool last_pass_on = tid + 256 * (NST - 1) < kMx4Pieces;
  u32x4 dat[DEPTH][NST];
  uint32_t scl[DEPTH][NST];
  int32_t slot_n[NST];  // slots of the tile whose loads are issued next (fetched a tile early)
  auto load_slots = [&](int t) {
#pragma unroll
    for (int i = 0; i < NST; ++i) slot_n[i] = static_cast<int32_t>(idx[min(lo + t * kMlaTile + (pc[i] >> 5), hi - 1)]);
  };
  auto issue_loads = [&](u32x4 (&d)[NST], uint32_t (&s)[NST]) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {  // two independent addresses per piece
      int row, col;
      coord(i, row, col);
      const int64_t slot = slot_n[i];
      d[i] = *reinterpret_cast<const u32x4*>(a.kv.data + (slot_offset<LINEAR>(slot, a.page_size, a.kv.dps, a.kv.dts) + 16 * col));
      s[i] = *reinterpret_cast<const uint16_t*>(a.kv.scales +
                                                (slot_offset<LINEAR>(slot, a.page_size, a.kv.sps, a.kv.sts) + 2 * col));
    }
  };
  auto write_lds = [&](const u32x4 (&d)[NST], const uint32_t (&s)[NST]) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      if (i == NST - 1 && !last_pass_on) break;
      int row, col;
      coord(i, row, col);
      char* dst = smem + row * kMlaLdsRow + col * 64;
      // write j carries sub-chunk j ^ x (dword j ^ x of the piece, scale byte (j ^ x) >> 1)
      const int x = (col >> 1) & 3;
      const bool x1 = x & 1, x2 = x & 2;
      uint32_t dw[4] = {d[i][0], d[i][1], d[i][2], d[i][3]};
      const uint32_t t0 = x1 ? dw[1] : dw[0], t1 = x1 ? dw[0] : dw[1], t2 = x1 ? dw[3] : dw[2], t3 = x1 ? dw[2] : dw[3];
      dw[0] = x2 ? t2 : t0;
      dw[1] = x2 ? t3 : t1;
      dw[2] = x2 ? t0 : t2;
      dw[3] = x2 ? t1 : t3;
      const uint32_t b0 = s[i] & 0xffu, b1 = s[i] >> 8;
      const float sc[2] = {mx4_scale_f32(x2 ? b1 : b0), mx4_scale_f32(x2 ? b0 : b1)};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<u32x4*>(dst + 16 * (j ^ x)) = mx4x8_to_16<T>(dw[j], sc[j >> 1]);
    }
  };

  f32x4 oacc[NBW];
#pragma unroll
  for (int nb = 0; nb < NBW; ++nb) oacc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float xai = xai_factor(a.xai_len, seq_len);
  const bool capped = a.logit_cap > 0.f;
  const float c2 = (capped ? kLog2e : a.sm_scale * kLog2e) * xai;

  // prologue: tiles 0 .. DEPTH-1 go to sets 0 .. DEPTH-1, tile 0 is written to LDS and its set refilled with tile DEPTH;
  // invariant at iteration t: set (t+1) % DEPTH holds tile t+1, slot_n the slots of tile t+1+DEPTH
  load_slots(0);
#pragma unroll
  for (int dd = 0; dd < DEPTH; ++dd) {
    if (dd < ntiles) {
      issue_loads(dat[dd], scl[dd]);
      if (dd + 1 < ntiles) load_slots(dd + 1);
    }
  }
  write_lds(dat[0], scl[0]);
  if (DEPTH < ntiles) {
    issue_loads(dat[0], scl[0]);
    if (DEPTH + 1 < ntiles) load_slots(DEPTH + 1);
  }
  __syncthreads();

  const int qd = r >> 2, pp = r & 3;
  f32x4* const xch = reinterpret_cast<f32x4*>(smem + kMlaTile * kMlaLdsRow);
  for (int t0 = 0; t0 < ntiles; t0 += DEPTH) {
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {  // unrolled so that the register set is a compile-time index
      const int t = t0 + u;
      if (t >= ntiles) break;
      // ---- S^T = K Q^T over all 576 columns, K fragments RX_MLA_MX4_PD reads ahead of their MFMA ----------------------
      f32x4 sacc[2];
      {
        constexpr int PD = KSW < RX_MLA_MX4_PD ? KSW : RX_MLA_MX4_PD;
        u32x4 kf[KSW];
        const char* kb0 = smem + ((w & 1) * 16 + r) * kMlaLdsRow + g * 16 + ks0 * 64;
#pragma unroll
        for (int i = 0; i < PD; ++i) kf[i] = *reinterpret_cast<const u32x4*>(kb0 + i * 64);
        f32x4 part = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < KSW; ++i) {
          if (i + PD < KSW) kf[i + PD] = *reinterpret_cast<const u32x4*>(kb0 + (i + PD) * 64);
          part = T::mfma(__builtin_bit_cast(vec8, kf[i]), qf[i], part);
        }
        xch[w * 64 + lane] = part;
        __syncthreads();
        sacc[0] = xch[0 * 64 + lane] + xch[2 * 64 + lane];
        sacc[1] = xch[1 * 64 + lane] + xch[3 * 64 + lane];
      }
      // ---- online softmax (identical in all four waves) ---------------------------------------------------------------
      float sv[8];
      const int tok_base = lo + t * kMlaTile + 4 * g;
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int i = 0; i < 4; ++i) sv[bb * 4 + i] = sacc[bb][i];
      if (capped) {  // ONE wave-uniform branch around all eight scores (rx_decode_mla.hip)
#pragma unroll
        for (int j = 0; j < 8; ++j) sv[j] = a.logit_cap * tanhf(sv[j] * a.sm_scale / a.logit_cap);
      }
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int i = 0; i < 4; ++i) sv[bb * 4 + i] = (tok_base + 16 * bb + i < hi) ? sv[bb * 4 + i] : -INFINITY;
      // No row maximum on the common path (rx_decode_mla.hip): the scores are exponentiated against the STANDING running
      // max and the lane's partial row sum is the check; the max-based step runs only when a lane's sum exceeds
      // kMlaSumLimit (or is inf / NaN: the split's first tile, m = -inf).  Compared as bits: sums are never negative.
      float alpha = 1.0f, psum = 0.f;
      {
        const float m_old = m_run;
        float e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          e[j] = fast_exp2(__builtin_fmaf(sv[j], c2, -m_old));
          psum += e[j];
        }
        if (__builtin_amdgcn_ballot_w64(__builtin_bit_cast(uint32_t, psum) > __builtin_bit_cast(uint32_t, kMlaSumLimit)) != 0) {
          float mt = fmaxf(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])), fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7])));
          mt = quad_row_max(mt) * c2;
          const float m_new = fmaxf(m_old, mt);
          alpha = fast_exp2(m_old - m_new);
          m_run = m_new;
          psum = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            sv[j] = fast_exp2(__builtin_fmaf(sv[j], c2, -m_new));
            psum += sv[j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) sv[j] = e[j];
        }
      }
      l_run = l_run * alpha + psum;
      u32x4 praw;
      praw[0] = pack2<T>(sv[0], sv[1]);
      praw[1] = pack2<T>(sv[2], sv[3]);
      praw[2] = pack2<T>(sv[4], sv[5]);
      praw[3] = pack2<T>(sv[6], sv[7]);
      const vec8 pf = __builtin_bit_cast(vec8, praw);
      if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb) oacc[nb] *= alpha;
      }
      // ---- O^T[128 w + ...] += V^T P^T, V = columns [0, 512) of the image -----------------------------------------------
      {
        const char* rp0 = smem + (4 * g + qd) * kMlaLdsRow + (128 * w) * 2 + 8 * pp;
        const char* rp1 = rp0 + 16 * kMlaLdsRow;
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb) {
          const u32x2 lo2 = T::ds_read_tr(rp0 + nb * 32);
          const u32x2 hi2 = T::ds_read_tr(rp1 + nb * 32);
          const vec8 av = __builtin_bit_cast(vec8, u32x4{lo2[0], lo2[1], hi2[0], hi2[1]});
          oacc[nb] = T::mfma(av, pf, oacc[nb]);
        }
      }
      // ---- unpack the next tile into the image, refill its register set -------------------------------------------------
      __syncthreads();  // every wave has read tile t: the image may be overwritten
      if (t + 1 < ntiles) {
        write_lds(dat[(u + 1) % DEPTH], scl[(u + 1) % DEPTH]);
        if (t + 1 + DEPTH < ntiles) {
          issue_loads(dat[(u + 1) % DEPTH], scl[(u + 1) % DEPTH]);
          if (t + 2 + DEPTH < ntiles) load_slots(t + 2 + DEPTH);
        }
      }
      __syncthreads();
    }
  }

  // ---- epilogue: every wave holds the full statistics and its own 128 output columns -------------------------------------
  l_run += __shfl_xor(l_run, 16);
  l_run += __shfl_xor(l_run, 32);
  if (!q_valid) return;
  if (single) {
    float den = l_run;
    if (a.sinks) den += fast_exp2(a.sinks[h] * kLog2e - m_run);
    const float inv = a.v_scale / den;
    uint16_t* op = a.o + b * a.o_stride_t + h * a.o_stride_h + 128 * w + 4 * g;
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb) {
      u32x2 pk;
      pk[0] = pack2<T>(oacc[nb][0] * inv, oacc[nb][1] * inv);
      pk[1] = pack2<T>(oacc[nb][2] * inv, oacc[nb][3] * inv);
      *reinterpret_cast<u32x2*>(op + 16 * nb) = pk;
    }
  } else {  // a partial for the stage-2 kernels of rx_decode.hip
    const int64_t row = (static_cast<int64_t>(b) * a.hq + h) * a.max_kv_splits + split;
    const float inv = 1.0f / l_run;
    float* lp = a.attn_logits + row * kMlaDv + 128 * w + 4 * g;
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb) *reinterpret_cast<f32x4*>(lp + 16 * nb) = oacc[nb] * inv;
    if (w == 0 && g == 0) a.attn_lse[row] = m_run * kLn2 + __logf(l_run);
  }
}

// called from rx_decode_attn_mx4 (rx_kv_mx4.hip), which has checked the options a 4-bit pool does not take
int launch_decode_mla_mx4(const rx_decode_params* p, const rx_kv_mx4_scales* sc, int max_splits, hipStream_t s) {
  RX_REQUIRE(p->kv.v_buf == p->kv.k_buf && sc->v_scale_buf == sc->k_scale_buf && p->kv.v_tok_stride == p->kv.k_tok_stride &&
                 p->kv.v_page_stride == p->kv.k_page_stride && sc->v_tok_stride == sc->k_tok_stride &&
                 sc->v_page_stride == sc->k_page_stride,
             "rx_decode_attn_mx4: latent rows (576 / 512, one kv head): v_buf / v_scale_buf must alias k_buf / k_scale_buf");
  RX_REQUIRE((p->kv.k_page_stride | p->kv.k_tok_stride | (int64_t)(uintptr_t)p->kv.k_buf) % 16 == 0 &&
                 (sc->k_page_stride | sc->k_tok_stride | (int64_t)(uintptr_t)sc->k_scale_buf) % 2 == 0,
             "rx_decode_attn_mx4: latent data rows must be 16-byte aligned, scale rows 2-byte aligned");
  RX_REQUIRE((p->q_stride_t | p->q_stride_h) % 8 == 0 && ((uintptr_t)p->q & 15) == 0,
             "rx_decode_attn_mx4: q rows must be 16-byte aligned");
  RX_REQUIRE((p->o_stride_t | p->o_stride_h) % 4 == 0 && ((uintptr_t)p->o & 7) == 0,
             "rx_decode_attn_mx4: o rows must be 8-byte aligned");
  if (max_splits > 1)
    RX_REQUIRE(((uintptr_t)p->attn_logits & 15) == 0, "rx_decode_attn_mx4: attn_logits must be 16-byte aligned");
  MlaMx4Args a;
  a.q = (const uint16_t*)p->q;
  a.o = (uint16_t*)p->o;
  a.q_stride_t = p->q_stride_t; a.q_stride_h = p->q_stride_h;
  a.o_stride_t = p->o_stride_t; a.o_stride_h = p->o_stride_h;
  a.kv = mx4_pool(p->kv.k_buf, sc->k_scale_buf, p->kv.k_page_stride, p->kv.k_tok_stride, 0, sc->k_page_stride, sc->k_tok_stride, 0);
  a.page_size = p->kv.page_size;
  if ((a.page_size & (a.page_size - 1)) == 0) a.page_size = -(__builtin_ctz(a.page_size) + 1);
  a.kv_indptr = p->kv_indptr;
  a.kv_indices = p->kv_indices;
  a.req_to_token = p->req_to_token;
  a.req_row_stride = p->req_row_stride;
  a.req_pool_indices = p->req_pool_indices;
  a.rpi64 = p->req_pool_indices_is_i64;
  a.seq_lens = p->seq_lens;
  a.sl64 = p->seq_lens_is_i64;
  a.num_kv_splits = max_splits > 1 ? p->num_kv_splits : nullptr;
  a.max_kv_splits = max_splits;
  a.attn_logits = p->attn_logits;
  a.attn_lse = p->attn_lse;
  a.bs = p->bs;
  a.hq = p->num_q_heads;
  a.qblocks = (p->num_q_heads + 15) / 16;
  a.sm_scale = p->sm_scale * p->k_scale;
  a.v_scale = p->v_scale;
  a.logit_cap = p->logit_cap;
  a.sinks = p->sinks;
  a.xai_len = p->xai_temperature_len;
  const int ps = p->kv.page_size;
  const bool linear = ps == 1 || (p->kv.k_page_stride == ps * p->kv.k_tok_stride && sc->k_page_stride == ps * sc->k_tok_stride);
  const bool idx64 = p->kv_indices != nullptr && p->kv_indices_is_i64;
  const unsigned pairs = static_cast<unsigned>(a.bs) * a.max_kv_splits;
  const unsigned grid = (pairs + 7) / 8 * 8 * a.qblocks;  // whole groups of 8 pairs (one per XCD)
  note_dispatch("decode_mla_mx4_kernel<%s, %s, %s>|%s", p->dtype == RX_BF16 ? "rx::BF16" : "rx::F16", idx64 ? "long" : "int",
                tbool(linear), a.kv_indices ? "indices" : "req_to_token");
#define RX_MM4(TT, IT, LIN) hipLaunchKernelGGL((decode_mla_mx4_kernel<TT, IT, LIN>), dim3(grid), dim3(256), 0, s, a)
#define RX_MM4_GO(TT)                          \
  do {                                         \
    if (idx64) {                               \
      if (linear) RX_MM4(TT, int64_t, true);   \
      else RX_MM4(TT, int64_t, false);         \
    } else {                                   \
      if (linear) RX_MM4(TT, int32_t, true);   \
      else RX_MM4(TT, int32_t, false);         \
    }                                          \
  } while (0)
  if (p->dtype == RX_BF16) RX_MM4_GO(BF16);
  else RX_MM4_GO(F16);
#undef RX_MM4
#undef RX_MM4_GO
  return RX_OK;
}
}  // namespace rx
