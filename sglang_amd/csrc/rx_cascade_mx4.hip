// Phase 1 of shared-prefix (cascade) decode over the 4-bit KV pool (MXFP4, blocks of 16; include/radix_hip.h "4-bit KV
// pool"): a chunk of the packed shared prefix attended by ALL member queries as the M dimension, 16-bit partial outputs and an
// fp32 LSE out.  The skip-extend, not-causal form of rx_extend_attn_mx4: the keys are the chunk only and every row sees all of
// it.  extend_mx4_kernel (rx_extend_mx4.hip) serves that form too, but is built for a FEW rows: its workgroup is one 64-row
// block, so 1024 rows per kv head (256 requests x G = 4) unpack the whole chunk sixteen times.
// MEASURED: this kernel takes 1.11-1.13x extend_mx4_kernel's time on identical phase-1 arguments at 256 and at
// 1024 rows per kv head, so option cascade_mx4 defaults to 0 and the kernel runs only when it is set to 1.
//
// cascade_mx4_kernel<T, D, IdxT, LINEAR>:
//   * Work split.  Workgroup = 4 waves = one (pseudo-request = prefix chunk, kv head, block of 128 packed ROWS); row r =
//     (member r / G, q head r % G of the kv head's group), G = Hq / Hkv at run time, as extend_mx4_kernel packs them.  A kv
//     head's bytes are fetched and unpacked once per 128 rows.  Wave w owns rows 32 w .. 32 w + 31 as TWO 16-row blocks over
//     every token of a 64-token tile: every K fragment and every V^T fragment read from LDS feeds two v_mfma_f32_16x16x32.
//   * Staging.  The 256 threads stage a tile as extend_mx4_kernel's prefix tiles: thread = (token tid / 4, quarter tid % 4 of
//     the row), D = 128: ONE 16-byte data load + one 16-bit scale-pair load from an address of its own (D = 64: 8 bytes + one
//     scale byte), for K and for V.  TWO register sets: while tile t is computed from the image, tile t + 1 goes from one set
//     into the other half of the image and that set is refilled with tile t + 3; tile t + 2 is in flight in the other set and
//     the slot ids of tile t + 4 are requested.  mx4x8_to_16 unpacks a dword into one 16-byte image chunk, exactly.
//   * The image is rx_extend.hip's (row = token, 16-byte chunk c at c ^ v_swizzle<D>(row)), double-buffered K | V, written
//     with extend_mx4_kernel's rotation (lane (row, q) writes chunk k ^ rot in step k); K A-fragments by ds_read_b128,
//     V^T by ds_read_b64_tr_b16.  One barrier per tile.
//   * S^T = K Q^T and O^T += V^T P^T; softmax lane-local (lane = one row of a block, 8 tokens of a 32-token half) with exp2 and
//     the plain running max; P rounded to T is the next B operand.  No new-token tiles, no causal mask: the only mask is the
//     chunk's last tile (kv_len % 64) and its branch is taken on that tile only.  k_scale is folded into the score scale,
//     v_scale applied once in the epilogue.  An empty chunk or row: zeros, lse = -inf.
#include <type_traits>

#include "rx_common.h"
#include "rx_decode_common.h"
#include "rx_mx4_common.h"

namespace rx {

constexpr int kCascTile = 64;   // tokens per staged tile
constexpr int kCascRows = 128;  // rows per workgroup: 4 waves x 2 blocks of 16

template <typename T, int D, typename IdxT, bool LINEAR>
__global__ __launch_bounds__(256, 2) void cascade_mx4_kernel(const Mx4ExtendArgs a) {
  using vec8 = typename T::vec8;
  constexpr int KS = D / 32;                // k-steps of the QK^T product
  constexpr int NB = D / 16;                // 16-wide d blocks of the output
  constexpr int RB = 2;                     // 16-row blocks per wave
  constexpr int ROW_BYTES = D * 2;          // image row
  constexpr int CPR = ROW_BYTES / 16;       // 16-byte chunks per image row
  constexpr int CPT = CPR / 4;              // chunks per staging thread (a quarter row) = dwords of its packed load
  constexpr int SB = D / 64;                // scale bytes per staging thread
  constexpr int TILE_BYTES = kCascTile * ROW_BYTES;
  using DataV = std::conditional_t<D == 128, u32x4, u32x2>;
  using ScaleV = std::conditional_t<D == 128, uint16_t, uint8_t>;
  using Set0 = std::integral_constant<int, 0>;
  using Set1 = std::integral_constant<int, 1>;
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];  // [buf][K | V]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;

  int bid = blockIdx.x;
  const int mb = bid % a.mblocks;
  bid /= a.mblocks;
  const int kvh = bid % a.hkv;
  const int req = bid / a.hkv;
  const int G = a.group;

  const int64_t qo0 = load_idx(a.qo_indptr, req, a.qo64);
  const int32_t E = static_cast<int32_t>(load_idx(a.qo_indptr, req + 1, a.qo64) - qo0);
  const int32_t kv0 = a.kv_indptr[req];
  const int32_t p_len = a.kv_indptr[req + 1] - kv0;  // tokens of this chunk
  const int32_t R = E * G;                           // query rows of this (chunk, kv head)
  const int32_t rb0 = mb * kCascRows;
  if (rb0 >= R) return;  // workgroup-uniform
  const int32_t rbase = rb0 + 16 * RB * w;
  const bool active = rbase < R;  // inactive waves still stage tiles and hit the barriers
  const IdxT* idx = reinterpret_cast<const IdxT*>(a.kv_indices) + kv0;

  // this lane's row of each block: a row past the end repeats the last one (computed, never stored)
  int32_t row[RB], m[RB], h[RB];
  vec8 qf[RB][KS];  // Q^T fragments (B operand): lane (r, g) holds Q[m][h][32 s + 8 g .. + 8]
#pragma unroll
  for (int k = 0; k < RB; ++k) {
    row[k] = rbase + 16 * k + r;
    const int32_t rowc = min(row[k], R - 1);
    m[k] = rowc / G;
    h[k] = kvh * G + rowc % G;
    const uint16_t* qp = a.q + (qo0 + m[k]) * a.q_stride_t + h[k] * a.q_stride_h + 8 * g;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[k][s] = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(qp + 32 * s));
  }
  // Q must have landed before the loop (rx_extend.hip: otherwise the loop header waits for vmcnt(0) every iteration)
  __builtin_amdgcn_s_waitcnt(0x0F70);

  const int nt = (p_len + kCascTile - 1) / kCascTile;

  // ---- cooperative staging: thread -> (token st_row of the tile, quarter sq of its row) ---------------------------------------
  const int st_row = tid >> 2, sq = tid & 3;
  const int rot = D == 128 ? ((sq ^ (sq >> 1)) & 1) : (sq & 1);  // step k carries chunk k ^ rot of the quarter (rx_extend_mx4.hip)
  const uint8_t* kdat = a.k.data + kvh * a.k.dhs + (D / 8) * sq;
  const uint8_t* vdat = a.v.data + kvh * a.v.dhs + (D / 8) * sq;
  const uint8_t* ksca = a.k.scales + kvh * a.k.shs + SB * sq;
  const uint8_t* vsca = a.v.scales + kvh * a.v.shs + SB * sq;

  int64_t slot = 0;  // the staged token's KV slot, of the tile whose loads go out next
  auto load_slot = [&](int t) __attribute__((always_inline)) { slot = static_cast<int64_t>(idx[min(t * kCascTile + st_row, p_len - 1)]); };
  DataV pk_k[2], pk_v[2];   // two register sets of packed quarter rows ...
  uint32_t sc_k[2], sc_v[2];  // ... and their scale bytes
  auto issue_loads = [&](auto set) __attribute__((always_inline)) {  // the scale loads go out with the data: four independent addresses
    constexpr int S = decltype(set)::value;
    pk_k[S] = *reinterpret_cast<const DataV*>(kdat + slot_offset<LINEAR>(slot, a.page_size, a.k.dps, a.k.dts));
    sc_k[S] = *reinterpret_cast<const ScaleV*>(ksca + slot_offset<LINEAR>(slot, a.page_size, a.k.sps, a.k.sts));
    pk_v[S] = *reinterpret_cast<const DataV*>(vdat + slot_offset<LINEAR>(slot, a.page_size, a.v.dps, a.v.dts));
    sc_v[S] = *reinterpret_cast<const ScaleV*>(vsca + slot_offset<LINEAR>(slot, a.page_size, a.v.sps, a.v.sts));
  };
  // chunk k of a packed quarter row as its 16-byte image chunk (D = 128: dwords 0, 1 are scale block 0; 2, 3 block 1)
  auto unpack = [&](const DataV& f, uint32_t sc, int k) __attribute__((always_inline)) -> u32x4 {
    const uint32_t dw = rot ? f[k ^ 1] : f[k];
    const uint32_t byte = SB == 2 ? (sc >> (8 * (k >> 1))) & 0xffu : sc;  // (k ^ rot) >> 1 == k >> 1
    return mx4x8_to_16<T>(dw, mx4_scale_f32(byte));
  };
  auto write_lds = [&](int t, auto set) __attribute__((always_inline)) {
    constexpr int S = decltype(set)::value;
    char* kt = smem + (t & 1) * 2 * TILE_BYTES + st_row * ROW_BYTES;
    char* vt = kt + TILE_BYTES;
    const int sw = v_swizzle<D>(st_row);
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int off = (((CPT * sq + (k ^ rot)) ^ sw) & (CPR - 1)) * 16;
      *reinterpret_cast<u32x4*>(kt + off) = unpack(pk_k[S], sc_k[S], k);
      *reinterpret_cast<u32x4*>(vt + off) = unpack(pk_v[S], sc_v[S], k);
    }
  };

  f32x4 oacc[RB][NB];
  float m_run[RB], l_run[RB];  // running max (log2 domain, identical in the 4 lanes of a row) / this lane's partial row sum
#pragma unroll
  for (int k = 0; k < RB; ++k) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) oacc[k][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    m_run[k] = -INFINITY;
    l_run[k] = 0.f;
  }

  // ---- prologue: tile 0 into the image, tiles 1 and 2 into the two register sets, tile 3's slot ids requested -----------------
  if (nt > 0) {
    load_slot(0);
    issue_loads(Set0{});
    if (nt > 1) {
      load_slot(1);
      issue_loads(Set1{});
    }
    if (nt > 2) load_slot(2);
    write_lds(0, Set0{});
    if (nt > 2) {
      issue_loads(Set0{});
      if (nt > 3) load_slot(3);
    }
  }
  __syncthreads();

  const int swr = v_swizzle<D>(r);  // swizzle of rows 16 k + r
  const int qd = r >> 2, pp = r & 3;
  const int vrow0 = 4 * g + qd;  // V^T read: row inside a 16-token block
  const int swv = v_swizzle<D>(vrow0);
  const bool capped = a.logit_cap > 0.f;
  const float cs = a.sm_scale * a.k_scale;
  const float cap_in = capped ? cs / a.logit_cap * (2.0f * kLog2e) : 0.f, cap_out = a.logit_cap * kLog2e;

  auto compute = [&](int t) __attribute__((always_inline)) {
    const char* kt = smem + (t & 1) * 2 * TILE_BYTES;
    const char* vt = kt + TILE_BYTES;
#pragma unroll
    for (int hh = 0; hh < kCascTile / 32; ++hh) {
      const int n0 = t * kCascTile + 32 * hh;  // first token of this 32-token half
      if (n0 >= p_len) continue;               // past the chunk's end (workgroup-uniform)
      __builtin_amdgcn_sched_barrier(0);  // (one half's fragments at a time: the next half's reads stay below this point)
      // ---- S^T[token][row] = K Q^T: one K fragment, both row blocks ----------------------------------------------------------
      f32x4 sacc[RB][2];
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
        for (int k = 0; k < RB; ++k) sacc[k][bb] = f32x4{0.f, 0.f, 0.f, 0.f};
        const char* krow = kt + (32 * hh + 16 * bb + r) * ROW_BYTES;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int chunk = ((4 * s + g) ^ swr) & (CPR - 1);
          const vec8 ka = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(krow + chunk * 16));
#pragma unroll
          for (int k = 0; k < RB; ++k) sacc[k][bb] = T::mfma(ka, qf[k][s], sacc[k][bb]);
        }
      }
      // ---- V^T fragments: read behind the softmax, four d blocks at a time (all of them at once, or any of them across the
      // softmax, do not fit 256 VGPRs beside two row blocks at D = 128: 9-21 spilled registers)
      const char* rp0 = vt + (32 * hh + vrow0) * ROW_BYTES + 8 * (pp & 1);
      const char* rp1 = rp0 + 16 * ROW_BYTES;
      u32x2 vlo[NB], vhi[NB];
      auto read_vt = [&](int nb) __attribute__((always_inline)) {
        const int chunk = ((2 * nb + (pp >> 1)) ^ swv) & (CPR - 1);
        vlo[nb] = T::ds_read_tr(rp0 + chunk * 16);
        vhi[nb] = T::ds_read_tr(rp1 + chunk * 16);
      };
      // ---- online softmax (lane = one row of each block, 8 tokens); the mask on the chunk's last tile only --------------------
      const bool full = n0 + 32 <= p_len;
      vec8 pf[RB];
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        float sv[8];
        float mt = -INFINITY;
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float x = sacc[k][bb][i];
            if (capped) {  // cap * tanh(x cs / cap), tanh(y) = 1 - 2 / (exp2(2 y log2 e) + 1): branch-free, saturates to +-1
              const float e = fast_exp2(x * cap_in);
              x = cap_out * (1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f));
            } else {
              x *= cs * kLog2e;
            }
            if (!full) x = (n0 + 16 * bb + 4 * g + i < p_len) ? x : -INFINITY;
            sv[bb * 4 + i] = x;
            mt = fmaxf(mt, x);
          }
        mt = quad_row_max(mt);
        const float m_new = fmaxf(m_run[k], mt);  // finite: token n0 is inside the chunk and visible to every row
        const float alpha = fast_exp2(m_run[k] - m_new);
        m_run[k] = m_new;
        float psum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          sv[j] = fast_exp2(sv[j] - m_new);
          psum += sv[j];
        }
        l_run[k] = l_run[k] * alpha + psum;
        u32x4 praw;
        praw[0] = pack2<T>(sv[0], sv[1]);
        praw[1] = pack2<T>(sv[2], sv[3]);
        praw[2] = pack2<T>(sv[4], sv[5]);
        praw[3] = pack2<T>(sv[6], sv[7]);
        pf[k] = __builtin_bit_cast(vec8, praw);
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {  // rescale O only when some row's max moved
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) oacc[k][nb] *= alpha;
        }
      }
      // ---- O^T += V^T P^T: one V^T fragment, both row blocks ---------------------------------------------------------------
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (nb % 4 == 0) {  // four d blocks' fragments at a time, fenced: the scheduler otherwise hoists all sixteen reads
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = nb; j < nb + 4; ++j) read_vt(j);
        }
        const vec8 av = __builtin_bit_cast(vec8, u32x4{vlo[nb][0], vlo[nb][1], vhi[nb][0], vhi[nb][1]});
#pragma unroll
        for (int k = 0; k < RB; ++k) oacc[k][nb] = T::mfma(av, pf[k], oacc[k][nb]);
      }
    }
  };
  // one tile: compute it from the image, move tile t + 1 from its register set into the other half, refill that set with
  // tile t + 3 (tile t + 2 stays in flight in the other set), request tile t + 4's slot ids
  auto step = [&](int t, auto next) __attribute__((always_inline)) {
    if (active) compute(t);
    if (t + 1 < nt) {
      write_lds(t + 1, next);
      if (t + 3 < nt) {
        issue_loads(next);
        if (t + 4 < nt) load_slot(t + 4);
      }
    }
    __syncthreads();
  };
  for (int t = 0; t < nt; t += 2) {  // unrolled by two: the register set is a compile-time index
    step(t, Set1{});
    if (t + 1 < nt) step(t + 1, Set0{});
  }

  // ---- epilogue: lane (r, g) holds O[row][16 nb + 4 g .. + 4] of each block ---------------------------------------------------
  if (!active) return;
#pragma unroll
  for (int k = 0; k < RB; ++k) {
    float l = l_run[k];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (row[k] >= R) continue;
    const float inv = l > 0.f ? a.v_scale / l : 0.f;  // an empty chunk: zeros, lse = -inf
    uint16_t* op = a.o + (qo0 + m[k]) * a.o_stride_t + h[k] * a.o_stride_h + 4 * g;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      u32x2 pk;
      pk[0] = pack2<T>(oacc[k][nb][0] * inv, oacc[k][nb][1] * inv);
      pk[1] = pack2<T>(oacc[k][nb][2] * inv, oacc[k][nb][3] * inv);
      *reinterpret_cast<u32x2*>(op + 16 * nb) = pk;
    }
    if (a.lse && g == 0)
      a.lse[(qo0 + m[k]) * a.lse_stride_t + h[k] * a.lse_stride_h] = l > 0.f ? m_run[k] * kLn2 + __logf(l) : -INFINITY;
  }
}

// the skip-extend, not-causal form of rx_extend_attn_mx4 (rx_extend_mx4.hip validated the call and filled `a`)
template <typename T, int D>
static void launch_cascade(Mx4ExtendArgs a, int64_t max_rows, bool idx64, bool linear, hipStream_t s) {
  a.mblocks = static_cast<int32_t>((max_rows + kCascRows - 1) / kCascRows);
  const unsigned grid = static_cast<unsigned>(a.bs) * a.hkv * a.mblocks;
  note_dispatch("cascade_mx4_kernel<%s, %d, %s, %s>|g%d", tname<T>(), D, idx64 ? "long" : "int", tbool(linear), a.group);
#define RX_CMX4(IDX, LIN) hipLaunchKernelGGL((cascade_mx4_kernel<T, D, IDX, LIN>), dim3(grid), dim3(256), 0, s, a)
  if (idx64) {
    if (linear) RX_CMX4(int64_t, true);
    else RX_CMX4(int64_t, false);
  } else {
    if (linear) RX_CMX4(int32_t, true);
    else RX_CMX4(int32_t, false);
  }
#undef RX_CMX4
}

void launch_cascade_mx4(const Mx4ExtendArgs& a, int64_t max_rows, bool bf16, int d, bool idx64, bool linear, hipStream_t s) {
  if (bf16) {
    if (d == 64) launch_cascade<BF16, 64>(a, max_rows, idx64, linear, s);
    else launch_cascade<BF16, 128>(a, max_rows, idx64, linear, s);
  } else {
    if (d == 64) launch_cascade<F16, 64>(a, max_rows, idx64, linear, s);
    else launch_cascade<F16, 128>(a, max_rows, idx64, linear, s);
  }
}

}  // namespace rx
