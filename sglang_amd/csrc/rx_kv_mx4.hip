// The 4-bit KV pool (MXFP4, blocks of 16; include/radix_hip.h "4-bit KV pool" states the format): the quantising
// store, decode attention that reads nibbles and scale bytes straight from HBM, and the row gather of an extend's prefix.
//
// Reference: MHATokenToKVPoolFP4 (srt/mem_cache/memory_pool.py:2959-3110) with FP4MXBlock16KVQuantizeUtil
// (srt/layers/quantization/kvfp4_tensor.py:56-147), whose _get_key_buffer dequantises the whole layer per call.
//
// decode_mx4_kernel keeps the skeleton of decode_mfma_kernel (rx_decode.hip): four independent waves per workgroup,
// wave-private 32-token tiles, no barrier in the loop, S^T = K Q^T on v_mfma_f32_16x16x32, lane-local online softmax,
// P as the next B operand, V through the wave's swizzled LDS tile and ds_read_b64_tr_b16.  Its data path is its own:
//   * D = 128: a (slot, head) row is 64 data bytes + 8 scale bytes.  Lane (r, g) of a 16-token row block takes ONE
//     16-byte load, bytes 16 g .. 16 g + 15 = elements 32 g .. 32 g + 31 = scale blocks 2 g, 2 g + 1 (one 16-bit
//     load issued with the data, from an address of its own: nothing waits for the data to find its scales).
//     Dword j of the load is k-step j (elements 32 g + 8 j ..): the contraction index is free to permute, so Q uses the
//     same map, qf[s] = Q[h][32 g + 8 s .. + 8].
//   * D = 64: a row is 32 data bytes + 4 scale bytes; lane (r, g) takes one 8-byte load, elements 16 g .. 16 g + 15 =
//     exactly scale block g (a one-byte load); dword j is k-step j, qf[s] = Q[h][16 g + 8 s .. + 8].
//   * unpack in registers: four v_cvt_scalef32_pk_{bf16,f16}_fp4 per dword (op_sel picks the byte) with the block's
//     2^(scale - 127) as the f32 scale operand (scale << 23).  The result is exact, so everything downstream is the
//     16-bit kernel's arithmetic.  For V the eight elements are the 16-byte LDS chunk (32 g + 8 s) / 8.
//   * a 32-token tile is 4.5 KiB (16 KiB in the 16-bit kernel): RX_MX4_DEPTH register sets of ~20 VGPRs each keep
//     DEPTH tiles per wave in flight (4 x 8 waves x 4.5 KiB = 144 KiB per CU at two workgroups per CU).
#include "rx_common.h"
#include "rx_decode_common.h"
#include "rx_mx4_common.h"

namespace rx {

#ifndef RX_MX4_DEPTH
#define RX_MX4_DEPTH 4  // K/V register sets (tiles in flight per wave) of decode_mx4_kernel
#endif

// ---- the format (the unpack: rx_mx4_common.h) ---------------------------------------------------------------------------
// One block of 16 source elements (two 16-byte loads) -> 8 data bytes + its scale byte: batched_quantize
// (kvfp4_tensor.py:56-103) evaluated in fp32.  e = max(-33, ceil(log2(max / 6))) comes from the maximum's exponent and
// mantissa (mantissa <= 1.5: E - 2, else E - 1), the magnitude code is the count of the bounds <= |x / 2^e| (ties go UP in
// magnitude -- not the round-to-nearest-even of v_cvt_scalef32_pk_fp4_*), the sign bit is x / 2^e < 0.
template <typename T>
__device__ __forceinline__ u32x2 mx4_quant16(u32x4 lo, u32x4 hi, float scale, uint32_t& scale_byte) {
  float f[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = T::to_f32(static_cast<uint16_t>(lo[i] & 0xffffu));
    f[2 * i + 1] = T::to_f32(static_cast<uint16_t>(lo[i] >> 16));
    f[8 + 2 * i] = T::to_f32(static_cast<uint16_t>(hi[i] & 0xffffu));
    f[8 + 2 * i + 1] = T::to_f32(static_cast<uint16_t>(hi[i] >> 16));
  }
  if (scale != 1.0f) {
#pragma unroll
    for (int i = 0; i < 16; ++i) f[i] = T::to_f32(T::from_f32(f[i] / scale));  // div_ rounds to the source dtype
  }
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) mx = fmaxf(mx, fabsf(f[i]));
  const uint32_t mb = __builtin_bit_cast(uint32_t, mx);
  int e = static_cast<int>(mb >> 23) - 127 - ((mb & 0x7fffffu) <= 0x400000u ? 2 : 1);
  e = max(e, -33);  // (a zero block, or one below 6 * 2^-33: scale byte 94)
  e = min(e, 126);  // (Inf / NaN maxima are outside the contract; keep the multiplier below a finite float)
  scale_byte = static_cast<uint32_t>(e + 127);
  const float inv = __builtin_bit_cast(float, static_cast<uint32_t>(127 - e) << 23);  // 2^-e: the product is exact
  u32x2 out = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float s = f[i] * inv, m = fabsf(s);
    const uint32_t code = (m >= 0.25f) + (m >= 0.75f) + (m >= 1.25f) + (m >= 1.75f) + (m >= 2.5f) + (m >= 3.5f) + (m >= 5.0f);
    out[i >> 3] |= (code | (s < 0.f ? 8u : 0u)) << (4 * (i & 7));
  }
  return out;
}

// ---- rx_store_kv_mx4: one wave per token, one 16-element block per lane and step ---------------------------------------
// Consecutive lanes own consecutive blocks of the row: their 8-byte data stores and their scale bytes are contiguous
// inside a head (and across heads in the NHD layout).
template <typename T>
__global__ __launch_bounds__(256) void store_kv_mx4_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                           const Mx4Pool kp, const Mx4Pool vp, const void* __restrict__ loc,
                                                           int64_t n, int hkv, int dk, int dv, int64_t k_stride_t,
                                                           int64_t v_stride_t, int page_size, float k_scale, float v_scale,
                                                           int loc64, int64_t size_limit, int64_t skip_index, int32_t* err_flag) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int64_t idx = load_idx(loc, row, loc64);
  if (idx == skip_index) return;
  if (idx < 0 || idx >= size_limit) {
    if (lane == 0 && err_flag) atomicOr(err_flag, RX_DEVERR_SLOT_OOB);
    return;
  }
  const int64_t pg = idx / page_size, off = idx % page_size;
  auto put = [&](const uint16_t* src, const Mx4Pool& p, int d, float scale) {
    for (int blk = lane; blk < hkv * (d >> 4); blk += 64) {
      const int h = blk / (d >> 4), bi = blk % (d >> 4);
      const u32x4* sp = reinterpret_cast<const u32x4*>(src + 16 * blk);
      uint32_t sb;
      const u32x2 q = mx4_quant16<T>(sp[0], sp[1], scale, sb);
      *reinterpret_cast<u32x2*>(p.data + pg * p.dps + off * p.dts + h * p.dhs + 8 * bi) = q;
      p.scales[pg * p.sps + off * p.sts + h * p.shs + bi] = static_cast<uint8_t>(sb);
    }
  };
  put(k + row * k_stride_t, kp, dk, k_scale);
  put(v + row * v_stride_t, vp, dv, v_scale);
}

// ---- rx_gather_kv_mx4: rows at loc[0:n] -> dense 16-bit [n, Hkv, D] (exact) ---------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gather_kv_mx4_kernel(const Mx4Pool kp, const Mx4Pool vp, const void* __restrict__ loc,
                                                            int64_t n, int hkv, int dk, int dv, int page_size,
                                                            uint16_t* __restrict__ k_out, uint16_t* __restrict__ v_out,
                                                            int loc64, int64_t size_limit, int32_t* err_flag) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int64_t idx = load_idx(loc, row, loc64);
  const bool ok = idx >= 0 && idx < size_limit;  // a slot outside the pool: flagged, its output rows are zero
  if (!ok && lane == 0 && err_flag) atomicOr(err_flag, RX_DEVERR_SLOT_OOB);
  const int64_t pg = ok ? idx / page_size : 0, off = ok ? idx % page_size : 0;
  auto get = [&](const Mx4Pool& p, int d, uint16_t* dst) {
    for (int blk = lane; blk < hkv * (d >> 4); blk += 64) {
      const int h = blk / (d >> 4), bi = blk % (d >> 4);
      u32x4 lo = {0u, 0u, 0u, 0u}, hi = lo;
      if (ok) {
        const u32x2 raw = *reinterpret_cast<const u32x2*>(p.data + pg * p.dps + off * p.dts + h * p.dhs + 8 * bi);
        const float sc = mx4_scale_f32(p.scales[pg * p.sps + off * p.sts + h * p.shs + bi]);
        lo = mx4x8_to_16<T>(raw[0], sc);
        hi = mx4x8_to_16<T>(raw[1], sc);
      }
      u32x4* dp = reinterpret_cast<u32x4*>(dst + 16 * blk);
      dp[0] = lo;
      dp[1] = hi;
    }
  };
  get(kp, dk, k_out + row * static_cast<int64_t>(hkv) * dk);
  get(vp, dv, v_out + row * static_cast<int64_t>(hkv) * dv);
}

// ---- rx_decode_attn_mx4 ---------------------------------------------------------------------------------------------------
struct Mx4DecodeArgs {
  const uint16_t* q;
  uint16_t* o;
  int64_t q_stride_t, q_stride_h, o_stride_t, o_stride_h;
  Mx4Pool k, v;
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
  int32_t bs, hq, hkv, group, qblocks;
  float sm_scale;  // sm_scale * k_scale
  float v_scale, logit_cap;
  const float* sinks;
  int32_t xai_len;
  const int32_t* order;
  const int32_t* kv_start;  // req_to_token mode: request b attends tokens [kv_start[b], seq_len_b) only (or NULL)
  int32_t all_partials;     // extra partials wait in stage 2: a request with ONE kv split writes a partial too
};

template <typename T, int D, typename IdxT, bool LINEAR>
__global__ __launch_bounds__(256, 2) void decode_mx4_kernel(const Mx4DecodeArgs a) {
  using vec8 = typename T::vec8;
  constexpr int KS = D / 32;  // k-steps of the QK^T product = dwords of a lane's load
  constexpr int NB = D / 16;  // 16-wide d blocks of the output
  constexpr int SB = D / 64;  // scale bytes per lane and row
  using DataV = std::conditional_t<D == 128, u32x4, u32x2>;
  using ScaleV = std::conditional_t<D == 128, uint16_t, uint8_t>;
  constexpr int ROW_BYTES = D * 2;
  constexpr int TILE_BYTES = kTile * ROW_BYTES;  // = 16 * D * 4 (fp32 O^T of one wave)
  constexpr int DEPTH = RX_MX4_DEPTH;
  __shared__ __attribute__((aligned(16))) char smem[kWavesPerWG * TILE_BYTES + 2 * 4 * 16 * 4];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;

  // split is the slowest grid dimension (rx_decode.hip: the live blocks of a partly dead grid spread over the XCDs)
  int bid = blockIdx.x;
  const int qb = bid % a.qblocks;
  bid /= a.qblocks;
  const int kvh = bid % a.hkv;
  bid /= a.hkv;
  const int b = a.order ? a.order[bid % a.bs] : bid % a.bs;
  const int split = bid / a.bs;

  int32_t seq_len, full_len;  // tokens this launch attends / the request's length
  const IdxT* idx;
  if (a.kv_indices) {
    const int32_t beg = a.kv_indptr[b];
    seq_len = full_len = a.kv_indptr[b + 1] - beg;
    idx = reinterpret_cast<const IdxT*>(a.kv_indices) + beg;
  } else {  // IdxT == int32_t in this mode
    full_len = static_cast<int32_t>(load_idx(a.seq_lens, b, a.sl64));
    const int32_t start = a.kv_start ? min(max(a.kv_start[b], 0), full_len) : 0;  // (attended_len, rx_decode.hip: stage 2 counts the same)
    seq_len = full_len - start;
    idx = reinterpret_cast<const IdxT*>(a.req_to_token + load_idx(a.req_pool_indices, b, a.rpi64) * a.req_row_stride) + start;
  }
  const int32_t splits = (a.num_kv_splits && a.max_kv_splits > 1) ? a.num_kv_splits[b] : 1;
  // a request with ONE kv split writes its final output here and stage 2 leaves it alone (direct_single, rx_decode.hip):
  // an empty request inside a split batch gets the zeros it gets from the 16-bit kernels
  // (with extra partials every request's result is stage 2's: one split, or an empty suffix, leaves it the extras alone)
  const bool single = a.max_kv_splits == 1 || (splits == 1 && !a.all_partials);
  const int gq = qb * 16 + r;  // q head inside the GQA group handled by this lane
  const bool q_valid = gq < a.group;
  const int h = kvh * a.group + gq;
  if (split >= splits) return;
  int32_t lo, hi;
  split_range(seq_len, splits, split, lo, hi);
  if (hi <= lo) {
    if (single && seq_len == 0) {  // empty request: define the output
      for (int i = tid; i < 16 * D; i += 256) {
        const int q = i / D, d = i % D;
        if (qb * 16 + q >= a.group) continue;
        a.o[b * a.o_stride_t + (kvh * a.group + qb * 16 + q) * a.o_stride_h + d] = T::from_f32(0.f);
      }
    }
    return;
  }
  const int ntiles = (hi - lo + kTile - 1) / kTile;

  const uint8_t* kbase = a.k.data + kvh * a.k.dhs + (D / 8) * g;
  const uint8_t* vbase = a.v.data + kvh * a.v.dhs + (D / 8) * g;
  const uint8_t* ksbase = a.k.scales + kvh * a.k.shs + SB * g;
  const uint8_t* vsbase = a.v.scales + kvh * a.v.shs + SB * g;
  char* vt = smem + w * TILE_BYTES;  // this wave's V tile

  f32x4 oacc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) oacc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY;  // running max (log2 domain), identical in the 4 lanes of a q head
  float l_run = 0.f;        // this lane's partial row sum

  const float xai = xai_factor(a.xai_len, full_len);
  const float scale_log2 = a.sm_scale * kLog2e * xai;

  auto load_slots = [&](int t, int64_t& s0, int64_t& s1) {
    const int32_t t0 = min(lo + t * kTile + r, hi - 1);
    const int32_t t1 = min(lo + t * kTile + 16 + r, hi - 1);
    s0 = static_cast<int64_t>(idx[t0]);
    s1 = static_cast<int64_t>(idx[t1]);
  };
  // a register set: the lane's piece of two 16-token row blocks of K and V, and their scale bytes
  DataV kf[DEPTH][2], vf[DEPTH][2];
  uint32_t ksf[DEPTH][2], vsf[DEPTH][2];
  auto load_kv = [&](int64_t s0, int64_t s1, DataV (&kfs)[2], DataV (&vfs)[2], uint32_t (&kss)[2], uint32_t (&vss)[2]) {
    const int64_t sl[2] = {s0, s1};
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {  // the scale loads go out with the data: eight independent addresses
      kfs[bb] = *reinterpret_cast<const DataV*>(kbase + slot_offset<LINEAR>(sl[bb], a.page_size, a.k.dps, a.k.dts));
      kss[bb] = *reinterpret_cast<const ScaleV*>(ksbase + slot_offset<LINEAR>(sl[bb], a.page_size, a.k.sps, a.k.sts));
    }
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      vfs[bb] = *reinterpret_cast<const DataV*>(vbase + slot_offset<LINEAR>(sl[bb], a.page_size, a.v.dps, a.v.dts));
      vss[bb] = *reinterpret_cast<const ScaleV*>(vsbase + slot_offset<LINEAR>(sl[bb], a.page_size, a.v.sps, a.v.sts));
    }
  };
  // eight elements of k-step s as a 16-bit MFMA operand / LDS chunk (D = 128: dwords 0, 1 are scale block 0; 2, 3 block 1)
  auto frag16 = [&](const DataV& f, uint32_t sc, int s) -> u32x4 {
    const uint32_t byte = SB == 2 ? (sc >> (8 * (s >> 1))) & 0xffu : sc;
    return mx4x8_to_16<T>(f[s], mx4_scale_f32(byte));
  };

  // set u holds tile w + 4 (u + DEPTH k); n0/n1[u] = the slots of the tile that will refill it
  constexpr int STEP = kWavesPerWG * DEPTH;
  int64_t n0[DEPTH], n1[DEPTH], f0[DEPTH], f1[DEPTH];
#pragma unroll
  for (int u = 0; u < DEPTH; ++u) {  // the first tiles' slot ids are requested before the q rows and land with them
    n0[u] = n1[u] = f0[u] = f1[u] = 0;
    const int tt = w + kWavesPerWG * u;
    if (tt < ntiles) load_slots(tt, f0[u], f1[u]);
  }
  // ---- Q^T fragments (B operand): lane (r, g) holds Q[h][(D / 4) g + 8 s .. + 8] ----------------------------------------
  vec8 qf[KS];
  {
    const uint16_t* qp = a.q + b * a.q_stride_t + (q_valid ? h : 0) * a.q_stride_h + (D / 4) * g;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const u32x4 raw = q_valid ? *reinterpret_cast<const u32x4*>(qp + 8 * s) : u32x4{0, 0, 0, 0};
      qf[s] = __builtin_bit_cast(vec8, raw);
    }
  }
  // Q must have landed before the loop (rx_decode.hip: otherwise the loop header waits for vmcnt(0) every iteration)
  __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll
  for (int u = 0; u < DEPTH; ++u) {
    const int tt = w + kWavesPerWG * u;
    if (tt < ntiles) {
      load_kv(f0[u], f1[u], kf[u], vf[u], ksf[u], vsf[u]);
      if (tt + STEP < ntiles) load_slots(tt + STEP, n0[u], n1[u]);
    }
  }

  for (int t0 = w; t0 < ntiles; t0 += STEP) {
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {  // unrolled: the register set is a compile-time index
      const int t = t0 + kWavesPerWG * u;
      if (t >= ntiles) break;
      // ---- S^T[token][q] = K Q^T ---------------------------------------------------------------------------------------
      f32x4 sacc[2];
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        sacc[bb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s)
          sacc[bb] = T::mfma(__builtin_bit_cast(vec8, frag16(kf[u][bb], ksf[u][bb], s)), qf[s], sacc[bb]);
      }
      // ---- V tile -> LDS (row = token, swizzled 16-byte chunks) ---------------------------------------------------------
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        const int row = 16 * bb + r;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int chunk = (KS * g + s) ^ v_swizzle<D>(row);  // V[row][(D / 4) g + 8 s .. + 8)
          *reinterpret_cast<u32x4*>(vt + row * ROW_BYTES + chunk * 16) = frag16(vf[u][bb], vsf[u][bb], s);
        }
      }
      // ---- prefetch the tile that refills this set ------------------------------------------------------------------------
      if (t + STEP < ntiles) {
        load_kv(n0[u], n1[u], kf[u], vf[u], ksf[u], vsf[u]);
        if (t + 2 * STEP < ntiles) load_slots(t + 2 * STEP, n0[u], n1[u]);
      }
      // ---- online softmax on the lane ---------------------------------------------------------------------------------------
      float sv[8];
      const int tok_base = lo + t * kTile + 4 * g;
      float mt = -INFINITY;
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float x = sacc[bb][i];
          if (a.logit_cap > 0.f) {
            x = a.logit_cap * tanhf(x * a.sm_scale / a.logit_cap) * (kLog2e * xai);
          } else {
            x *= scale_log2;
          }
          x = (tok_base + 16 * bb + i < hi) ? x : -INFINITY;
          sv[bb * 4 + i] = x;
          mt = fmaxf(mt, x);
        }
      mt = quad_row_max(mt);
      const float m_new = fmaxf(m_run, mt);
      const float alpha = fast_exp2(m_run - m_new);
      m_run = m_new;
      float psum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sv[j] = fast_exp2(sv[j] - m_new);
        psum += sv[j];
      }
      l_run = l_run * alpha + psum;
      u32x4 praw;
      praw[0] = pack2<T>(sv[0], sv[1]);
      praw[1] = pack2<T>(sv[2], sv[3]);
      praw[2] = pack2<T>(sv[4], sv[5]);
      praw[3] = pack2<T>(sv[6], sv[7]);
      const vec8 pf = __builtin_bit_cast(vec8, praw);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) oacc[nb] *= alpha;

      // ---- O^T += V^T P^T, V^T fragments by transposed LDS reads ----------------------------------------------------------
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      {
        const int qd = r >> 2, pp = r & 3;
        const int row0 = 4 * g + qd;  // + 16 for the second 16-token block
        const int sw = v_swizzle<D>(row0);  // same for row0 + 16
        const char* rp0 = vt + row0 * ROW_BYTES + 8 * (pp & 1);
        const char* rp1 = rp0 + 16 * ROW_BYTES;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const int chunk = (2 * nb + (pp >> 1)) ^ sw;
          const u32x2 lo2 = T::ds_read_tr(rp0 + chunk * 16);
          const u32x2 hi2 = T::ds_read_tr(rp1 + chunk * 16);
          const u32x4 av = u32x4{lo2[0], lo2[1], hi2[0], hi2[1]};
          oacc[nb] = T::mfma(__builtin_bit_cast(vec8, av), pf, oacc[nb]);
        }
      }
    }
  }

  // ---- merge the four waves through LDS -------------------------------------------------------------------------------------
  l_run += __shfl_xor(l_run, 16);
  l_run += __shfl_xor(l_run, 32);
  float* sm_m = reinterpret_cast<float*>(smem + kWavesPerWG * TILE_BYTES);
  float* sm_l = sm_m + kWavesPerWG * 16;
  __syncthreads();  // every wave is done with its V tile
  {
    float* ot = reinterpret_cast<float*>(vt);  // [16 q][D] fp32
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) *reinterpret_cast<f32x4*>(ot + r * D + 16 * nb + 4 * g) = oacc[nb];
    if (g == 0) {
      sm_m[w * 16 + r] = m_run;
      sm_l[w * 16 + r] = l_run;
    }
  }
  __syncthreads();
  for (int i = tid; i < 16 * D; i += 256) {
    const int q = i / D, d = i % D;
    const int gq2 = qb * 16 + q;
    if (gq2 >= a.group) continue;
    const int hh = kvh * a.group + gq2;
    float mx = sm_m[q];
#pragma unroll
    for (int ww = 1; ww < kWavesPerWG; ++ww) mx = fmaxf(mx, sm_m[ww * 16 + q]);
    float lsum = 0.f, acc = 0.f;
#pragma unroll
    for (int ww = 0; ww < kWavesPerWG; ++ww) {
      const float sc = fast_exp2(sm_m[ww * 16 + q] - mx);
      lsum += sm_l[ww * 16 + q] * sc;
      acc += reinterpret_cast<const float*>(smem + ww * TILE_BYTES)[q * D + d] * sc;
    }
    if (single) {
      float den = lsum;
      if (a.sinks) den += fast_exp2(a.sinks[hh] * kLog2e - mx);
      a.o[b * a.o_stride_t + hh * a.o_stride_h + d] = T::from_f32(acc / den * a.v_scale);
    } else {  // a partial for the stage-2 kernels of rx_decode.hip
      const int64_t row = (static_cast<int64_t>(b) * a.hq + hh) * a.max_kv_splits + split;
      a.attn_logits[row * D + d] = acc / lsum;
      if (d == 0) a.attn_lse[row] = mx * kLn2 + __logf(lsum);
    }
  }
}

template <typename T, int D>
static void launch_decode_mx4(const Mx4DecodeArgs& a, bool idx64, bool linear, hipStream_t s) {
  const unsigned grid = static_cast<unsigned>(a.bs) * a.hkv * a.qblocks * a.max_kv_splits;
  note_dispatch("decode_mx4_kernel<%s, %d, %s, %s>|slots,%s", tname<T>(), D, idx64 ? "long" : "int", tbool(linear),
                a.kv_indices ? "indices" : "req_to_token");
#define RX_MX4(IDX, LIN) hipLaunchKernelGGL((decode_mx4_kernel<T, D, IDX, LIN>), dim3(grid), dim3(256), 0, s, a)
  if (idx64) {
    if (linear) RX_MX4(int64_t, true);
    else RX_MX4(int64_t, false);
  } else {
    if (linear) RX_MX4(int32_t, true);
    else RX_MX4(int32_t, false);
  }
#undef RX_MX4
}

// the layout's checks shared by the three entry points: D in units the kernels' vector accesses need
static int mx4_check_layout(const char* who, const rx_kv_layout* lay, const rx_kv_mx4_scales* sc, int dk, int dv) {
  RX_REQUIRE(lay && sc && lay->k_buf && lay->v_buf && sc->k_scale_buf && sc->v_scale_buf, "%s: null layout / buffer", who);
  RX_REQUIRE(lay->page_size >= 1, "%s: page_size < 1", who);
  RX_REQUIRE(dk > 0 && dv > 0 && dk % 16 == 0 && dv % 16 == 0, "%s: head dims must be positive multiples of 16", who);
  const int64_t all = lay->k_page_stride | lay->k_tok_stride | lay->k_head_stride | lay->v_page_stride | lay->v_tok_stride |
                      lay->v_head_stride | (uintptr_t)lay->k_buf | (uintptr_t)lay->v_buf;
  RX_REQUIRE(all % 8 == 0, "%s: data buffers and their byte strides must be multiples of 8", who);
  return RX_OK;
}

}  // namespace rx

using namespace rx;

extern "C" int rx_store_kv_mx4(const void* k, const void* v, const rx_kv_layout* lay, const rx_kv_mx4_scales* sc, const void* loc,
                               int64_t n, int num_kv_heads, int head_dim, int v_head_dim, int64_t k_stride_t, int64_t v_stride_t,
                               int src_dtype, float k_scale, float v_scale, int loc_is_i64, int64_t size_limit,
                               int64_t skip_index, int32_t* err_flag, void* stream) {
  RX_RANGE("rx_store_kv_mx4");
  RX_REQUIRE(n >= 0, "rx_store_kv_mx4: n < 0");
  if (n == 0) return RX_OK;
  RX_REQUIRE(k && v && loc, "rx_store_kv_mx4: null pointer");
  if (const int rc = mx4_check_layout("rx_store_kv_mx4", lay, sc, head_dim, v_head_dim)) return rc;
  RX_REQUIRE(src_dtype == RX_BF16 || src_dtype == RX_F16, "rx_store_kv_mx4: src_dtype %d", src_dtype);
  RX_REQUIRE(num_kv_heads > 0 && size_limit > 0, "rx_store_kv_mx4: num_kv_heads / size_limit must be positive");
  RX_REQUIRE(k_scale > 0.f && v_scale > 0.f, "rx_store_kv_mx4: scales must be > 0");
  RX_REQUIRE((k_stride_t | v_stride_t) % 8 == 0 && (((uintptr_t)k | (uintptr_t)v) % 16 == 0),
             "rx_store_kv_mx4: source rows must be 16-byte aligned");
  const Mx4Pool kp = mx4_pool(lay->k_buf, sc->k_scale_buf, lay->k_page_stride, lay->k_tok_stride, lay->k_head_stride,
                              sc->k_page_stride, sc->k_tok_stride, sc->k_head_stride);
  const Mx4Pool vp = mx4_pool(lay->v_buf, sc->v_scale_buf, lay->v_page_stride, lay->v_tok_stride, lay->v_head_stride,
                              sc->v_page_stride, sc->v_tok_stride, sc->v_head_stride);
#define RX_SQ(TT)                                                                                                           \
  hipLaunchKernelGGL(store_kv_mx4_kernel<TT>, dim3(static_cast<unsigned>((n + 3) / 4)), dim3(256), 0,                       \
                     static_cast<hipStream_t>(stream), (const uint16_t*)k, (const uint16_t*)v, kp, vp, loc, n, num_kv_heads, \
                     head_dim, v_head_dim, k_stride_t, v_stride_t, lay->page_size, k_scale, v_scale, loc_is_i64, size_limit, \
                     skip_index, err_flag)
  if (src_dtype == RX_BF16) RX_SQ(BF16);
  else RX_SQ(F16);
#undef RX_SQ
  return check_launch("rx_store_kv_mx4");
}

extern "C" int rx_gather_kv_mx4(const rx_kv_layout* lay, const rx_kv_mx4_scales* sc, const void* loc, int loc_is_i64, int64_t n,
                                int num_kv_heads, int head_dim, int v_head_dim, void* k_out, void* v_out, int dst_dtype,
                                int64_t size_limit, int32_t* err_flag, void* stream) {
  RX_RANGE("rx_gather_kv_mx4");
  RX_REQUIRE(n >= 0, "rx_gather_kv_mx4: n < 0");
  if (n == 0) return RX_OK;
  RX_REQUIRE(loc && k_out && v_out, "rx_gather_kv_mx4: null pointer");
  if (const int rc = mx4_check_layout("rx_gather_kv_mx4", lay, sc, head_dim, v_head_dim)) return rc;
  RX_REQUIRE(dst_dtype == RX_BF16 || dst_dtype == RX_F16, "rx_gather_kv_mx4: dst_dtype %d", dst_dtype);
  RX_REQUIRE(num_kv_heads > 0 && size_limit > 0, "rx_gather_kv_mx4: num_kv_heads / size_limit must be positive");
  RX_REQUIRE((((uintptr_t)k_out | (uintptr_t)v_out) % 16) == 0, "rx_gather_kv_mx4: outputs must be 16-byte aligned");
  const Mx4Pool kp = mx4_pool(lay->k_buf, sc->k_scale_buf, lay->k_page_stride, lay->k_tok_stride, lay->k_head_stride,
                              sc->k_page_stride, sc->k_tok_stride, sc->k_head_stride);
  const Mx4Pool vp = mx4_pool(lay->v_buf, sc->v_scale_buf, lay->v_page_stride, lay->v_tok_stride, lay->v_head_stride,
                              sc->v_page_stride, sc->v_tok_stride, sc->v_head_stride);
#define RX_GQ(TT)                                                                                                          \
  hipLaunchKernelGGL(gather_kv_mx4_kernel<TT>, dim3(static_cast<unsigned>((n + 3) / 4)), dim3(256), 0,                     \
                     static_cast<hipStream_t>(stream), kp, vp, loc, n, num_kv_heads, head_dim, v_head_dim, lay->page_size, \
                     (uint16_t*)k_out, (uint16_t*)v_out, loc_is_i64, size_limit, err_flag)
  if (dst_dtype == RX_BF16) RX_GQ(BF16);
  else RX_GQ(F16);
#undef RX_GQ
  return check_launch("rx_gather_kv_mx4");
}

namespace rx {
int launch_decode_mla_mx4(const rx_decode_params* p, const rx_kv_mx4_scales* sc, int max_splits, hipStream_t s);  // rx_decode_mla_mx4.hip
int decode_merge_partials(const rx_decode_params* p, void* stream);  // rx_decode.hip: stage 2, one-split requests left alone
}

// A one-tensor (latent) pool: the row [nope | rope] is ONE buffer of (rank + rope_dim) / 2 data bytes and (rank + rope_dim) / 16
// scale bytes.  Both widths are multiples of 16, so no block straddles the seam and the two-tensor kernels serve it as they
// are: "K" = the nope part, "V" = the rope part rank / 2 data bytes (rank / 16 scale bytes) further into the same row -- or
// the whole row as K and an empty V.
static int mla_pool_pair(const char* who, const rx_kv_layout* lay, const rx_kv_mx4_scales* sc, int rank, int rope_dim, Mx4Pool& kp,
                         Mx4Pool& vp) {
  RX_REQUIRE(lay && sc && lay->k_buf && sc->k_scale_buf, "%s: null layout / buffer", who);
  RX_REQUIRE(lay->page_size >= 1, "%s: page_size < 1", who);
  RX_REQUIRE(rank > 0 && rope_dim >= 0 && rank % 16 == 0 && rope_dim % 16 == 0, "%s: kv_lora_rank / rope_dim must be multiples of 16", who);
  RX_REQUIRE((lay->k_page_stride | lay->k_tok_stride | (int64_t)(uintptr_t)lay->k_buf) % 8 == 0,
             "%s: the data buffer and its byte strides must be multiples of 8", who);
  kp = mx4_pool(lay->k_buf, sc->k_scale_buf, lay->k_page_stride, lay->k_tok_stride, 0, sc->k_page_stride, sc->k_tok_stride, 0);
  vp = kp;
  vp.data += rank / 2;
  vp.scales += rank / 16;
  return RX_OK;
}

extern "C" int rx_store_mla_mx4(const void* nope_or_row, const void* rope, const rx_kv_layout* lay, const rx_kv_mx4_scales* sc,
                                const void* loc, int64_t n, int kv_lora_rank, int rope_dim, int64_t nope_stride_t,
                                int64_t rope_stride_t, int src_dtype, float scale, int loc_is_i64, int64_t size_limit,
                                int64_t skip_index, int32_t* err_flag, void* stream) {
  RX_RANGE("rx_store_mla_mx4");
  RX_REQUIRE(n >= 0, "rx_store_mla_mx4: n < 0");
  if (n == 0) return RX_OK;
  RX_REQUIRE(nope_or_row && loc, "rx_store_mla_mx4: null pointer");
  Mx4Pool kp, vp;
  if (const int rc = mla_pool_pair("rx_store_mla_mx4", lay, sc, kv_lora_rank, rope_dim, kp, vp)) return rc;
  RX_REQUIRE(src_dtype == RX_BF16 || src_dtype == RX_F16, "rx_store_mla_mx4: src_dtype %d", src_dtype);
  RX_REQUIRE(size_limit > 0 && scale > 0.f, "rx_store_mla_mx4: size_limit and scale must be positive");
  RX_REQUIRE((nope_stride_t | (rope ? rope_stride_t : 0)) % 8 == 0 && (((uintptr_t)nope_or_row | (uintptr_t)rope) % 16 == 0),
             "rx_store_mla_mx4: source rows must be 16-byte aligned");
  // rope == NULL: nope_or_row is the whole (rank + rope_dim)-wide row
  const int dk = rope ? kv_lora_rank : kv_lora_rank + rope_dim, dv = rope ? rope_dim : 0;
#define RX_SQ(TT)                                                                                                              \
  hipLaunchKernelGGL(store_kv_mx4_kernel<TT>, dim3(static_cast<unsigned>((n + 3) / 4)), dim3(256), 0,                          \
                     static_cast<hipStream_t>(stream), (const uint16_t*)nope_or_row, (const uint16_t*)rope, kp, vp, loc, n, 1, dk, \
                     dv, nope_stride_t, rope_stride_t, lay->page_size, scale, scale, loc_is_i64, size_limit, skip_index, err_flag)
  if (src_dtype == RX_BF16) RX_SQ(BF16);
  else RX_SQ(F16);
#undef RX_SQ
  return check_launch("rx_store_mla_mx4");
}

extern "C" int rx_gather_mla_mx4(const rx_kv_layout* lay, const rx_kv_mx4_scales* sc, const void* loc, int loc_is_i64, int64_t n,
                                 int kv_lora_rank, int rope_dim, void* nope_out, void* rope_out, int dst_dtype, int64_t size_limit,
                                 int32_t* err_flag, void* stream) {
  RX_RANGE("rx_gather_mla_mx4");
  RX_REQUIRE(n >= 0, "rx_gather_mla_mx4: n < 0");
  if (n == 0) return RX_OK;
  RX_REQUIRE(loc && nope_out && (rope_out || rope_dim == 0), "rx_gather_mla_mx4: null pointer");
  Mx4Pool kp, vp;
  if (const int rc = mla_pool_pair("rx_gather_mla_mx4", lay, sc, kv_lora_rank, rope_dim, kp, vp)) return rc;
  RX_REQUIRE(dst_dtype == RX_BF16 || dst_dtype == RX_F16, "rx_gather_mla_mx4: dst_dtype %d", dst_dtype);
  RX_REQUIRE(size_limit > 0, "rx_gather_mla_mx4: size_limit must be positive");
  RX_REQUIRE((((uintptr_t)nope_out | (uintptr_t)rope_out) % 16) == 0, "rx_gather_mla_mx4: outputs must be 16-byte aligned");
#define RX_GQ(TT)                                                                                                            \
  hipLaunchKernelGGL(gather_kv_mx4_kernel<TT>, dim3(static_cast<unsigned>((n + 3) / 4)), dim3(256), 0,                       \
                     static_cast<hipStream_t>(stream), kp, vp, loc, n, 1, kv_lora_rank, rope_dim, lay->page_size,            \
                     (uint16_t*)nope_out, (uint16_t*)rope_out, loc_is_i64, size_limit, err_flag)
  if (dst_dtype == RX_BF16) RX_GQ(BF16);
  else RX_GQ(F16);
#undef RX_GQ
  return check_launch("rx_gather_mla_mx4");
}

static int decode_attn_mx4_impl(const rx_decode_params* p, const rx_kv_mx4_scales* sc, void* stream) {
  RX_REQUIRE(p, "rx_decode_attn_mx4: params is null");
  RX_REQUIRE(sc, "rx_decode_attn_mx4: scales is null");
  RX_REQUIRE(p->bs >= 0, "rx_decode_attn_mx4: bs < 0");
  if (p->bs == 0) return RX_OK;
  RX_REQUIRE(kv_strides_fit_u31(p->kv) && kv_strides_fit_u31(*sc),
             "rx_decode_attn_mx4: per-page / per-token byte strides of the data and scale buffers must lie in [0, 2^31)");
  RX_REQUIRE(p->q && p->o, "rx_decode_attn_mx4: null q / o");
  RX_REQUIRE(p->num_q_heads > 0 && p->num_kv_heads > 0 && p->num_q_heads % p->num_kv_heads == 0,
             "rx_decode_attn_mx4: Hq=%d must be a positive multiple of Hkv=%d", p->num_q_heads, p->num_kv_heads);
  RX_REQUIRE(p->dtype == RX_BF16 || p->dtype == RX_F16, "rx_decode_attn_mx4: dtype %d", p->dtype);
  const int dk = p->head_dim, dv = p->v_head_dim;
  const bool mla = dk == 576 && dv == 512 && p->num_kv_heads == 1;  // latent rows: decode_mla_mx4_kernel
  if (!mla && !(dk == dv && (dk == 64 || dk == 128)))
    return fail(RX_ERR_UNSUPPORTED, "rx_decode_attn_mx4: head dims %d / %d (64 or 128, or latent rows 576 / 512 with one kv head)",
                dk, dv);
#define RX_MX4_NO(cond, what) \
  if (cond) return fail(RX_ERR_UNSUPPORTED, "rx_decode_attn_mx4: " what " is not supported on a 4-bit pool")
  RX_MX4_NO(p->k_new || p->v_new, "the fused store (k_new / v_new)");
  RX_MX4_NO(p->rope_cos_sin, "fused RoPE (rope_cos_sin)");
  RX_MX4_NO(p->score_bias, "score_bias");
  RX_MX4_NO(p->split_items, "split_items");
  RX_MX4_NO(p->unit_desc || p->unit_first_slots, "unit_desc / unit_first_slots");
  RX_MX4_NO(p->merge_counters, "merge_counters");
  RX_MX4_NO(p->stages != 0, "stages 1 / 2");
#undef RX_MX4_NO
  if (const int rc = mx4_check_layout("rx_decode_attn_mx4", &p->kv, sc, dk, dv)) return rc;
  const bool mode_a = p->kv_indices != nullptr;
  if (mode_a) {
    RX_REQUIRE(p->kv_indptr, "rx_decode_attn_mx4: kv_indices given without kv_indptr");
  } else {
    RX_REQUIRE(p->req_to_token && p->req_pool_indices && p->seq_lens,
               "rx_decode_attn_mx4: neither kv_indices nor req_to_token/req_pool_indices/seq_lens");
  }
  const int max_splits = (p->max_kv_splits < 1 || !p->num_kv_splits) ? 1 : p->max_kv_splits;
  // shared-prefix (cascade) decode: the suffix [kv_start[b], seq_len_b) of the req_to_token rows, and the chunk partials of
  // phase 1 (rx_extend_attn_mx4) merged by stage 2 -- every request writes its partials then, sinks join once, there
  const int num_extra = p->num_extra_partials > 0 ? p->num_extra_partials : 0;
  if (p->kv_start || num_extra) {
    if (mla) return fail(RX_ERR_UNSUPPORTED, "rx_decode_attn_mx4: kv_start / extra partials are not supported on latent rows (576 / 512)");
    if (p->kv_start && mode_a)
      return fail(RX_ERR_UNSUPPORTED, "rx_decode_attn_mx4: kv_start applies to the req_to_token lookup only (with kv_indices, "
                  "build the list with rx_build_kv_indices' kv_start)");
    if (p->kv_start && p->xai_temperature_len > 0)
      return fail(RX_ERR_UNSUPPORTED, "rx_decode_attn_mx4: xai_temperature_len with kv_start is not supported on a 4-bit pool");
    if (num_extra)
      RX_REQUIRE(p->extra_o && p->extra_lse && max_splits > 1,
                 "rx_decode_attn_mx4: extra partials need extra_o, extra_lse and max_kv_splits > 1 (stage 2 merges them)");
  }
  if (max_splits > 1)
    RX_REQUIRE(p->attn_logits && p->attn_lse, "rx_decode_attn_mx4: max_kv_splits=%d needs attn_logits and attn_lse", max_splits);
  // one (D / 8)-byte load per lane and row, D / 64 scale bytes beside it; 16-byte q loads
  const int64_t dall = p->kv.k_page_stride | p->kv.k_tok_stride | p->kv.k_head_stride | p->kv.v_page_stride |
                       p->kv.v_tok_stride | p->kv.v_head_stride | (uintptr_t)p->kv.k_buf | (uintptr_t)p->kv.v_buf;
  const int64_t sall = sc->k_page_stride | sc->k_tok_stride | sc->k_head_stride | sc->v_page_stride | sc->v_tok_stride |
                       sc->v_head_stride | (uintptr_t)sc->k_scale_buf | (uintptr_t)sc->v_scale_buf;
  RX_REQUIRE(mla || (dall % (dk / 8) == 0 && sall % (dk / 64) == 0),
             "rx_decode_attn_mx4: data rows must be %d-byte aligned, scale rows %d-byte aligned", dk / 8, dk / 64);
  RX_REQUIRE((p->q_stride_t | p->q_stride_h) % 8 == 0 && ((uintptr_t)p->q & 15) == 0,
             "rx_decode_attn_mx4: q rows must be 16-byte aligned");
  auto s = static_cast<hipStream_t>(stream);
  if (mla) {
    if (const int rc = launch_decode_mla_mx4(p, sc, max_splits, s)) return rc;
  } else {
  Mx4DecodeArgs a;
  a.q = (const uint16_t*)p->q;
  a.o = (uint16_t*)p->o;
  a.q_stride_t = p->q_stride_t; a.q_stride_h = p->q_stride_h;
  a.o_stride_t = p->o_stride_t; a.o_stride_h = p->o_stride_h;
  a.k = mx4_pool(p->kv.k_buf, sc->k_scale_buf, p->kv.k_page_stride, p->kv.k_tok_stride, p->kv.k_head_stride, sc->k_page_stride,
                 sc->k_tok_stride, sc->k_head_stride);
  a.v = mx4_pool(p->kv.v_buf, sc->v_scale_buf, p->kv.v_page_stride, p->kv.v_tok_stride, p->kv.v_head_stride, sc->v_page_stride,
                 sc->v_tok_stride, sc->v_head_stride);
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
  a.hkv = p->num_kv_heads;
  a.group = p->num_q_heads / p->num_kv_heads;
  a.qblocks = (a.group + 15) / 16;
  a.sm_scale = p->sm_scale * p->k_scale;
  a.v_scale = p->v_scale;
  a.logit_cap = p->logit_cap;
  a.sinks = p->sinks;
  a.xai_len = p->xai_temperature_len;
  a.order = p->request_order;
  a.kv_start = p->kv_start;
  a.all_partials = num_extra > 0;
  const int ps = p->kv.page_size;
  const bool linear = ps == 1 || (p->kv.k_page_stride == ps * p->kv.k_tok_stride && p->kv.v_page_stride == ps * p->kv.v_tok_stride &&
                                  sc->k_page_stride == ps * sc->k_tok_stride && sc->v_page_stride == ps * sc->v_tok_stride);
  const bool idx64 = mode_a && p->kv_indices_is_i64;
  if (p->dtype == RX_BF16) {
    if (dk == 64) launch_decode_mx4<BF16, 64>(a, idx64, linear, s);
    else launch_decode_mx4<BF16, 128>(a, idx64, linear, s);
  } else {
    if (dk == 64) launch_decode_mx4<F16, 64>(a, idx64, linear, s);
    else launch_decode_mx4<F16, 128>(a, idx64, linear, s);
  }
  }
  if (const int rc = check_launch("rx_decode_attn_mx4")) return rc;
  if (max_splits == 1) return RX_OK;
  // the partials have the 16-bit kernels' layout: the existing stage-2 kernels merge them.  Stage 2 never reads the pool,
  // so the call carries the buffers' addresses only.
  rx_decode_params m = *p;
  m.kv.page_size = 1;
  m.kv.k_page_stride = m.kv.k_tok_stride = m.kv.k_head_stride = 0;
  m.kv.v_page_stride = m.kv.v_tok_stride = m.kv.v_head_stride = 0;
  m.kv.kv_fp8 = 0;
  m.max_kv_splits = max_splits;
  m.request_order = nullptr;
  m.partial_pairs_hint = 0;
  m.stages = 2;
  return decode_merge_partials(&m, stream);
}

extern "C" int rx_decode_attn_mx4(const rx_decode_params* p, const rx_kv_mx4_scales* sc, void* stream) {
  RX_RANGE("rx_decode_attn_mx4");
  return rx::dump_on_error("decode_attn_mx4", decode_attn_mx4_impl(p, sc, stream), p, p ? sizeof(*p) : 0);
}
