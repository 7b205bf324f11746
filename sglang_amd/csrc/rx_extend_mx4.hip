// Extend attention over the 4-bit KV pool (MXFP4, blocks of 16; include/radix_hip.h "4-bit KV pool"): the cached prefix is
// read as packed nibbles + scale bytes straight from the pool, the new tokens' K / V as the 16-bit k_extend / v_extend rows,
// in ONE pass with one output rounding.  Replaces rx_gather_kv_mx4 (a dense 16-bit copy of every prefix row) + the 16-bit
// extend on that copy: 144 B per cached token and kv head at D = 128 instead of 144 read + 512 written + 512 read.
//
// extend_mx4_kernel<T, D, IdxT, LINEAR>:
//   * Work split.  Workgroup = 4 waves = one (request, kv head, block of 64 query ROWS); row r = (token r / G, q head r % G
//     of the kv head's group), G = Hq / Hkv at run time: a short extend's few tokens x G heads fill the MFMA's 16 columns
//     and a kv head's packed bytes are fetched and unpacked once per row block, not once per q head.  Wave w owns rows
//     16 w .. 16 w + 15 over every token of a tile; causality is per row from its token index.
//   * Tiles of 64 tokens, staged by the 256 threads (thread = token tid / 4, quarter tid % 4 of the row), one tile ahead in
//     registers, into a double-buffered 16-bit K | V image, one barrier per tile.  Tiles run [prefix ... | new tokens ...];
//     the diagonal tile is the last one.  The compute loop reads the image only and does not know where a tile came from.
//       - prefix tile, D = 128: the thread takes ONE 16-byte data load (elements 32 q .. 32 q + 31 of the row) and one
//         16-bit scale-pair load from an address of its own, issued with the data (D = 64: 8 bytes + one scale byte), for K
//         and for V; slot ids are fetched one tile further ahead.  mx4x8_to_16 (v_cvt_scalef32_pk_*_fp4, scale byte << 23)
//         unpacks a dword into one 16-byte image chunk, exactly.
//       - new-token tile: the same quarter of the 16-bit row, D / 32 16-byte loads through k_extend / v_extend's strides.
//   * The image is rx_extend.hip's: row = token, 16-byte chunk c at c ^ v_swizzle<D>(row).  The readers are that kernel's
//     (K A-fragments by ds_read_b128 at chunk (4 s + g) ^ swz, V^T by ds_read_b64_tr_b16), so what round 3 established for
//     them holds unchanged.  The WRITER differs: neighbouring lanes own neighbouring quarters of one row, 64 B apart, so
//     eight lanes writing "their k-th chunk" would cover two rows x four quarters = eight chunks that fold onto FOUR
//     16-byte bank groups of the 32 banks a ds_write_b128 group of eight lanes sees (quarters q and q + 2 of a 256-byte row
//     are 128 B apart).  Lane (row, q) therefore writes chunk k ^ rot in step k, rot = (q ^ (q >> 1)) & 1 at D = 128 and q & 1
//     at D = 64: quarters 128 B apart now differ in bit 0 of the chunk, rows differ through the swizzle (bit 1 at D = 128,
//     bit 0 ^ rot at D = 64), and the eight lanes cover eight distinct bank groups; the same holds for sixteen contiguous
//     lanes over 64 banks.  A prefix tile pays one v_cndmask per dword for the rotation, a new-token tile nothing (its
//     loads are issued in the rotated order).
//   * S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_16x16x32; softmax lane-local (lane = one row, 8 tokens of a 32-token
//     half) with exp2 and a running max; P rounded to T is the next B operand.  k_scale / v_scale apply to the prefix part
//     (the extend contract of rx_extend_attn): k_scale folded into sm_scale there, v_scale into P before its rounding.
#include "rx_common.h"
#include "rx_decode_common.h"
#include "rx_mx4_common.h"

namespace rx {

constexpr int kMx4Tile = 64;  // tokens per staged tile = rows per workgroup

template <typename T, int D, typename IdxT, bool LINEAR>
__global__ __launch_bounds__(256, 2) void extend_mx4_kernel(const Mx4ExtendArgs a) {
  using vec8 = typename T::vec8;
  constexpr int KS = D / 32;                // k-steps of the QK^T product
  constexpr int NB = D / 16;                // 16-wide d blocks of the output
  constexpr int ROW_BYTES = D * 2;          // image row
  constexpr int CPR = ROW_BYTES / 16;       // 16-byte chunks per image row
  constexpr int CPT = CPR / 4;              // chunks per staging thread (a quarter row) = dwords of its packed load
  constexpr int SB = D / 64;                // scale bytes per staging thread
  constexpr int TILE_BYTES = kMx4Tile * ROW_BYTES;
  using DataV = std::conditional_t<D == 128, u32x4, u32x2>;
  using ScaleV = std::conditional_t<D == 128, uint16_t, uint8_t>;
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
  const int32_t p_len = a.kv_indptr[req + 1] - kv0;  // prefix length
  const int32_t R = E * G;                           // query rows of this (request, kv head)
  const int32_t rb0 = mb * kMx4Tile;
  if (rb0 >= R) return;  // workgroup-uniform
  const int32_t rbase = rb0 + 16 * w;
  const bool active = rbase < R;  // inactive waves still stage tiles and hit the barriers
  const IdxT* idx = reinterpret_cast<const IdxT*>(a.kv_indices) + kv0;

  // this lane's row: a row past the end repeats the last one (computed, never stored)
  const int32_t row = rbase + r;
  const int32_t rowc = min(row, R - 1);
  const int32_t m = rowc / G;              // token inside the extend part
  const int32_t h = kvh * G + rowc % G;    // q head

  // ---- Q^T fragments (B operand): lane (r, g) holds Q[m][h][32 s + 8 g .. + 8] ------------------------------------------------
  vec8 qf[KS];
  {
    const uint16_t* qp = a.q + (qo0 + m) * a.q_stride_t + h * a.q_stride_h + 8 * g;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(qp + 32 * s));
  }
  // Q must have landed before the loop (rx_extend.hip: otherwise the loop header waits for vmcnt(0) every iteration)
  __builtin_amdgcn_s_waitcnt(0x0F70);

  // keys: [prefix 0 .. p_len) | new tokens 0 .. n_end); causal: a row sees new tokens n <= its own
  const int32_t n_end_wg = a.skip_extend ? 0 : (a.causal ? min(R - 1, rb0 + kMx4Tile - 1) / G + 1 : E);
  const int32_t n_end_w = a.skip_extend ? 0 : (a.causal ? min(R - 1, rbase + 15) / G + 1 : E);
  const int32_t tok_lo_w = rbase / G;  // the wave's first token: new tokens up to it are visible to every row of the wave
  const int nt1 = (p_len + kMx4Tile - 1) / kMx4Tile;
  const int nt2 = (n_end_wg + kMx4Tile - 1) / kMx4Tile;
  const int nt = nt1 + nt2;

  // ---- cooperative staging: thread -> (token st_row of the tile, quarter sq of its row) ---------------------------------------
  const int st_row = tid >> 2, sq = tid & 3;
  const int rot = D == 128 ? ((sq ^ (sq >> 1)) & 1) : (sq & 1);  // step k carries chunk k ^ rot of the quarter (header)
  const uint8_t* kdat = a.k.data + kvh * a.k.dhs + (D / 8) * sq;
  const uint8_t* vdat = a.v.data + kvh * a.v.dhs + (D / 8) * sq;
  const uint8_t* ksca = a.k.scales + kvh * a.k.shs + SB * sq;
  const uint8_t* vsca = a.v.scales + kvh * a.v.shs + SB * sq;
  const uint16_t* kext = a.k_ext + qo0 * a.k_stride_t + kvh * a.k_stride_h + 8 * CPT * sq;
  const uint16_t* vext = a.v_ext + qo0 * a.v_stride_t + kvh * a.v_stride_h + 8 * CPT * sq;

  int64_t slot = 0;  // prefix tile: the token's KV slot; new-token tile: its row inside the extend part
  auto load_slot = [&](int t) {
    if (t < nt1) slot = static_cast<int64_t>(idx[min(t * kMx4Tile + st_row, p_len - 1)]);
    else slot = min((t - nt1) * kMx4Tile + st_row, n_end_wg - 1);
  };
  DataV pk_k, pk_v;          // a prefix tile's packed quarter rows ...
  uint32_t sc_k = 0, sc_v = 0;  // ... and their scale bytes
  u32x4 stg_k[CPT], stg_v[CPT];  // a new-token tile's 16-bit quarter rows, in write order
  auto issue_loads = [&](int t) {
    if (t < nt1) {  // the scale loads go out with the data: four independent addresses
      pk_k = *reinterpret_cast<const DataV*>(kdat + slot_offset<LINEAR>(slot, a.page_size, a.k.dps, a.k.dts));
      sc_k = *reinterpret_cast<const ScaleV*>(ksca + slot_offset<LINEAR>(slot, a.page_size, a.k.sps, a.k.sts));
      pk_v = *reinterpret_cast<const DataV*>(vdat + slot_offset<LINEAR>(slot, a.page_size, a.v.dps, a.v.dts));
      sc_v = *reinterpret_cast<const ScaleV*>(vsca + slot_offset<LINEAR>(slot, a.page_size, a.v.sps, a.v.sts));
    } else {
      const uint16_t* kp = kext + mul_u32(slot, a.k_stride_t);
      const uint16_t* vp = vext + mul_u32(slot, a.v_stride_t);
#pragma unroll
      for (int k = 0; k < CPT; ++k) {
        stg_k[k] = *reinterpret_cast<const u32x4*>(kp + 8 * (k ^ rot));
        stg_v[k] = *reinterpret_cast<const u32x4*>(vp + 8 * (k ^ rot));
      }
    }
  };
  // chunk j of a packed quarter row as its 16-byte image chunk (D = 128: dwords 0, 1 are scale block 0; 2, 3 block 1)
  auto unpack = [&](const DataV& f, uint32_t sc, int k) -> u32x4 {
    const uint32_t dw = rot ? f[k ^ 1] : f[k];
    const uint32_t byte = SB == 2 ? (sc >> (8 * (k >> 1))) & 0xffu : sc;  // (k ^ rot) >> 1 == k >> 1
    return mx4x8_to_16<T>(dw, mx4_scale_f32(byte));
  };
  auto write_lds = [&](int t) {
    char* kt = smem + (t & 1) * 2 * TILE_BYTES + st_row * ROW_BYTES;
    char* vt = kt + TILE_BYTES;
    const int sw = v_swizzle<D>(st_row);
    const bool prefix = t < nt1;  // workgroup-uniform
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int off = (((CPT * sq + (k ^ rot)) ^ sw) & (CPR - 1)) * 16;
      *reinterpret_cast<u32x4*>(kt + off) = prefix ? unpack(pk_k, sc_k, k) : stg_k[k];
      *reinterpret_cast<u32x4*>(vt + off) = prefix ? unpack(pk_v, sc_v, k) : stg_v[k];
    }
  };

  f32x4 oacc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) oacc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY;  // running max (log2 domain), identical in the 4 lanes of a row
  float l_run = 0.f;        // this lane's partial row sum

  // ---- prologue: tile 0 into the image, tile 1 into registers, tile 2's slot ids requested ------------------------------------
  if (nt > 0) {
    load_slot(0);
    issue_loads(0);
    if (nt > 1) load_slot(1);
    write_lds(0);
    if (nt > 1) {
      issue_loads(1);
      if (nt > 2) load_slot(2);
    }
  }
  __syncthreads();

  const int swr = v_swizzle<D>(r);  // swizzle of rows 16 k + r
  const int qd = r >> 2, pp = r & 3;
  const int vrow0 = 4 * g + qd;  // V^T read: row inside a 16-token block
  const int swv = v_swizzle<D>(vrow0);
  const bool capped = a.logit_cap > 0.f;

  for (int t = 0; t < nt; ++t) {
    const char* kt = smem + (t & 1) * 2 * TILE_BYTES;
    const char* vt = kt + TILE_BYTES;
    const bool prefix = t < nt1;
    const int tile_n0 = (prefix ? t : t - nt1) * kMx4Tile;
    const int32_t lim = prefix ? p_len : n_end_w;
    const float cs = prefix ? a.sm_scale * a.k_scale : a.sm_scale;
    const float vs = prefix ? a.v_scale : 1.0f;
    if (active) {
#pragma unroll
      for (int hh = 0; hh < kMx4Tile / 32; ++hh) {
        const int n0 = tile_n0 + 32 * hh;  // first token of this 32-token half
        if (n0 >= lim) continue;           // nothing visible to this wave (wave-uniform)
        // ---- S^T[token][row] = K Q^T ----------------------------------------------------------------------------------------
        f32x4 sacc[2];
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
          sacc[bb] = f32x4{0.f, 0.f, 0.f, 0.f};
          const char* krow = kt + (32 * hh + 16 * bb + r) * ROW_BYTES;
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const int chunk = ((4 * s + g) ^ swr) & (CPR - 1);
            const vec8 ka = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4*>(krow + chunk * 16));
            sacc[bb] = T::mfma(ka, qf[s], sacc[bb]);
          }
        }
        // ---- V^T fragments: issued before the softmax so the LDS round trip hides under it ----------------------------------
        const char* rp0 = vt + (32 * hh + vrow0) * ROW_BYTES + 8 * (pp & 1);
        const char* rp1 = rp0 + 16 * ROW_BYTES;
        u32x2 vlo[NB], vhi[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const int chunk = ((2 * nb + (pp >> 1)) ^ swv) & (CPR - 1);
          vlo[nb] = T::ds_read_tr(rp0 + chunk * 16);
          vhi[nb] = T::ds_read_tr(rp1 + chunk * 16);
        }
        // ---- masks + online softmax (lane = one row, 8 tokens) --------------------------------------------------------------
        const bool full = prefix ? (n0 + 32 <= p_len) : (n0 + 32 <= n_end_w && (!a.causal || n0 + 31 <= tok_lo_w));
        float sv[8];
        float mt = -INFINITY;
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float x = sacc[bb][i];
            x = capped ? a.logit_cap * tanhf(x * cs / a.logit_cap) * kLog2e : x * (cs * kLog2e);
            if (!full) {
              const int n = n0 + 16 * bb + 4 * g + i;
              const bool keep = prefix ? n < p_len : (n < n_end_w && (!a.causal || n <= m));
              x = keep ? x : -INFINITY;
            }
            sv[bb * 4 + i] = x;
            mt = fmaxf(mt, x);
          }
        mt = quad_row_max(mt);
        const float m_new = fmaxf(m_run, mt);
        const float m_ref = m_new == -INFINITY ? 0.f : m_new;  // (a row with nothing visible so far: p = 0, no NaN)
        const float alpha = fast_exp2(m_run - m_ref);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          sv[j] = fast_exp2(sv[j] - m_ref);
          psum += sv[j];
        }
        l_run = l_run * alpha + psum;
        if (vs != 1.0f) {  // per-tensor V scale of the cached part (wave-uniform)
#pragma unroll
          for (int j = 0; j < 8; ++j) sv[j] *= vs;
        }
        u32x4 praw;
        praw[0] = pack2<T>(sv[0], sv[1]);
        praw[1] = pack2<T>(sv[2], sv[3]);
        praw[2] = pack2<T>(sv[4], sv[5]);
        praw[3] = pack2<T>(sv[6], sv[7]);
        const vec8 pf = __builtin_bit_cast(vec8, praw);
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {  // rescale O only when some row's max moved
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) oacc[nb] *= alpha;
        }
        // ---- O^T += V^T P^T ---------------------------------------------------------------------------------------------------
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const vec8 av = __builtin_bit_cast(vec8, u32x4{vlo[nb][0], vlo[nb][1], vhi[nb][0], vhi[nb][1]});
          oacc[nb] = T::mfma(av, pf, oacc[nb]);
        }
      }
    }
    // ---- stage the next tile: registers (loaded one tile ago) -> the other image ---------------------------------------------
    if (t + 1 < nt) {
      write_lds(t + 1);
      if (t + 2 < nt) {
        issue_loads(t + 2);
        if (t + 3 < nt) load_slot(t + 3);
      }
    }
    __syncthreads();
  }

  // ---- epilogue: lane (r, g) holds O[row][16 nb + 4 g .. + 4] -------------------------------------------------------------------
  if (!active || row >= R) return;
  float l = l_run;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const float inv = l > 0.f ? 1.0f / l : 0.f;  // a row with no visible key: zeros, lse = -inf
  uint16_t* op = a.o + (qo0 + m) * a.o_stride_t + h * a.o_stride_h + 4 * g;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    u32x2 pk;
    pk[0] = pack2<T>(oacc[nb][0] * inv, oacc[nb][1] * inv);
    pk[1] = pack2<T>(oacc[nb][2] * inv, oacc[nb][3] * inv);
    *reinterpret_cast<u32x2*>(op + 16 * nb) = pk;
  }
  if (a.lse && g == 0)
    a.lse[(qo0 + m) * a.lse_stride_t + h * a.lse_stride_h] = l > 0.f ? m_run * kLn2 + __logf(l) : -INFINITY;
}

template <typename T, int D>
static void launch_extend_mx4(const Mx4ExtendArgs& a, bool idx64, bool linear, hipStream_t s) {
  const unsigned grid = static_cast<unsigned>(a.bs) * a.hkv * a.mblocks;
  note_dispatch("extend_mx4_kernel<%s, %d, %s, %s>|g%d", tname<T>(), D, idx64 ? "long" : "int", tbool(linear), a.group);
#define RX_EMX4(IDX, LIN) hipLaunchKernelGGL((extend_mx4_kernel<T, D, IDX, LIN>), dim3(grid), dim3(256), 0, s, a)
  if (idx64) {
    if (linear) RX_EMX4(int64_t, true);
    else RX_EMX4(int64_t, false);
  } else {
    if (linear) RX_EMX4(int32_t, true);
    else RX_EMX4(int32_t, false);
  }
#undef RX_EMX4
}

void launch_cascade_mx4(const Mx4ExtendArgs& a, int64_t max_rows, bool bf16, int d, bool idx64, bool linear, hipStream_t s);  // rx_cascade_mx4.hip

}  // namespace rx

using namespace rx;

static int extend_attn_mx4_impl(const rx_extend_params* p, const rx_kv_mx4_scales* sc, void* stream) {
  RX_REQUIRE(p, "rx_extend_attn_mx4: params is null");
  RX_REQUIRE(sc, "rx_extend_attn_mx4: scales is null");
  if (p->skip_prefix) {  // nothing is read from the pool: the 16-bit entry's call, without the byte layout
    rx_extend_params f = *p;
    f.kv = rx_kv_layout{};
    f.kv.page_size = 1;
    return rx_extend_attn(&f, stream);
  }
  RX_REQUIRE(p->bs >= 0 && p->max_extend_len >= 0, "rx_extend_attn_mx4: negative sizes");
  if (p->bs == 0 || p->max_extend_len == 0) return RX_OK;
  RX_REQUIRE(kv_strides_fit_u31(p->kv) && kv_strides_fit_u31(*sc) &&
                 (p->skip_extend || (stride_fits_u31(p->k_stride_t) && stride_fits_u31(p->v_stride_t))),
             "rx_extend_attn_mx4: per-page / per-token strides of the data and scale buffers (bytes) and of "
             "k_extend / v_extend (elements) must lie in [0, 2^31)");
  RX_REQUIRE(p->q && p->o, "rx_extend_attn_mx4: null q / o");
  RX_REQUIRE(p->skip_extend || (p->k_extend && p->v_extend), "rx_extend_attn_mx4: null k_extend / v_extend");
  RX_REQUIRE(p->qo_indptr && p->kv_indptr && p->kv_indices, "rx_extend_attn_mx4: null qo_indptr / kv_indptr / kv_indices");
  RX_REQUIRE(p->num_q_heads > 0 && p->num_kv_heads > 0 && p->num_q_heads % p->num_kv_heads == 0,
             "rx_extend_attn_mx4: Hq=%d must be a positive multiple of Hkv=%d", p->num_q_heads, p->num_kv_heads);
  RX_REQUIRE(p->dtype == RX_BF16 || p->dtype == RX_F16, "rx_extend_attn_mx4: dtype %d", p->dtype);
  const int dk = p->head_dim, dv = p->v_head_dim;
  if (dk == 576 && dv == 512)
    return fail(RX_ERR_UNSUPPORTED, "rx_extend_attn_mx4: latent rows (head dims 576 / 512) are not supported: gather them (rx_gather_mla_mx4)");
  if (!(dk == dv && (dk == 64 || dk == 128)))
    return fail(RX_ERR_UNSUPPORTED, "rx_extend_attn_mx4: head dims %d / %d (head_dim == v_head_dim in {64, 128})", dk, dv);
#define RX_EMX4_NO(cond, what) \
  if (cond) return fail(RX_ERR_UNSUPPORTED, "rx_extend_attn_mx4: " what " is not supported on a 4-bit pool")
  RX_EMX4_NO(p->custom_mask, "custom_mask");
  RX_EMX4_NO(p->sliding_window_size > 0, "sliding_window_size");
  RX_EMX4_NO(p->sinks, "sinks");
  RX_EMX4_NO(p->xai_temperature_len > 0, "xai_temperature_len");
  RX_EMX4_NO(p->score_bias, "score_bias");
  RX_EMX4_NO(p->unified_prefix_lens, "unified_prefix_lens");
  RX_EMX4_NO(p->q_pack > 1, "q_pack > 1 (the kernel packs its rows by itself)");
  RX_EMX4_NO(p->window_kv_offsets, "window_kv_offsets");
#undef RX_EMX4_NO
  RX_REQUIRE(p->kv.k_buf && p->kv.v_buf && sc->k_scale_buf && sc->v_scale_buf, "rx_extend_attn_mx4: null pool buffer");
  RX_REQUIRE(p->kv.page_size >= 1, "rx_extend_attn_mx4: page_size < 1");
  // one (D / 8)-byte load per staging thread and row, D / 64 scale bytes beside it; 16-byte q / k / v chunks, 8-byte o stores
  const int64_t dall = p->kv.k_page_stride | p->kv.k_tok_stride | p->kv.k_head_stride | p->kv.v_page_stride |
                       p->kv.v_tok_stride | p->kv.v_head_stride | (uintptr_t)p->kv.k_buf | (uintptr_t)p->kv.v_buf;
  const int64_t sall = sc->k_page_stride | sc->k_tok_stride | sc->k_head_stride | sc->v_page_stride | sc->v_tok_stride |
                       sc->v_head_stride | (uintptr_t)sc->k_scale_buf | (uintptr_t)sc->v_scale_buf;
  if (dall % (dk / 8) != 0 || sall % (dk / 64) != 0)
    return fail(RX_ERR_UNSUPPORTED, "rx_extend_attn_mx4: data rows must be %d-byte aligned, scale rows %d-byte aligned", dk / 8,
                dk / 64);
  const int64_t oall = p->q_stride_t | p->q_stride_h | p->o_stride_t | p->o_stride_h |
                       (p->skip_extend ? 0 : p->k_stride_t | p->k_stride_h | p->v_stride_t | p->v_stride_h);
  if (oall % 8 != 0) return fail(RX_ERR_UNSUPPORTED, "rx_extend_attn_mx4: q / k / v / o strides must be multiples of 8 elements");
  RX_REQUIRE((((uintptr_t)p->q | (p->skip_extend ? 0 : (uintptr_t)p->k_extend | (uintptr_t)p->v_extend)) & 15) == 0 &&
                 ((uintptr_t)p->o & 7) == 0,
             "rx_extend_attn_mx4: q / k_extend / v_extend must be 16-byte and o 8-byte aligned");
  RX_REQUIRE(!p->lse || ((uintptr_t)p->lse & 3) == 0, "rx_extend_attn_mx4: misaligned lse");
  Mx4ExtendArgs a;
  a.q = (const uint16_t*)p->q;
  a.k_ext = (const uint16_t*)p->k_extend;
  a.v_ext = (const uint16_t*)p->v_extend;
  a.o = (uint16_t*)p->o;
  a.q_stride_t = p->q_stride_t; a.q_stride_h = p->q_stride_h;
  a.k_stride_t = p->k_stride_t; a.k_stride_h = p->k_stride_h;
  a.v_stride_t = p->v_stride_t; a.v_stride_h = p->v_stride_h;
  a.o_stride_t = p->o_stride_t; a.o_stride_h = p->o_stride_h;
  a.k = mx4_pool(p->kv.k_buf, sc->k_scale_buf, p->kv.k_page_stride, p->kv.k_tok_stride, p->kv.k_head_stride, sc->k_page_stride,
                 sc->k_tok_stride, sc->k_head_stride);
  a.v = mx4_pool(p->kv.v_buf, sc->v_scale_buf, p->kv.v_page_stride, p->kv.v_tok_stride, p->kv.v_head_stride, sc->v_page_stride,
                 sc->v_tok_stride, sc->v_head_stride);
  const int ps = p->kv.page_size;
  a.page_size = (ps & (ps - 1)) == 0 ? -(__builtin_ctz(ps) + 1) : ps;
  a.qo_indptr = p->qo_indptr;
  a.qo64 = p->qo_indptr_is_i64;
  a.kv_indptr = p->kv_indptr;
  a.kv_indices = p->kv_indices;
  a.lse = p->lse;
  a.lse_stride_t = p->lse_stride_t;
  a.lse_stride_h = p->lse_stride_h;
  a.bs = p->bs;
  a.hkv = p->num_kv_heads;
  a.group = p->num_q_heads / p->num_kv_heads;
  a.mblocks = static_cast<int32_t>((static_cast<int64_t>(p->max_extend_len) * a.group + kMx4Tile - 1) / kMx4Tile);
  a.sm_scale = p->sm_scale;
  a.k_scale = p->k_scale;
  a.v_scale = p->v_scale;
  a.logit_cap = p->logit_cap;
  a.causal = p->is_causal;
  a.skip_extend = p->skip_extend;
  const bool linear = ps == 1 || (p->kv.k_page_stride == ps * p->kv.k_tok_stride && p->kv.v_page_stride == ps * p->kv.v_tok_stride &&
                                  sc->k_page_stride == ps * sc->k_tok_stride && sc->v_page_stride == ps * sc->v_tok_stride);
  const bool idx64 = p->kv_indices_is_i64 != 0;
  auto s = static_cast<hipStream_t>(stream);
  if (p->skip_extend && !p->is_causal && options().cascade_mx4) {
    // the chunk-of-a-shared-prefix form (every row sees all of the prefix, many rows) on cascade_mx4_kernel, 128 rows per workgroup
    // (opt-in: extend_mx4_kernel measured 0.89x its time on this form)
    launch_cascade_mx4(a, static_cast<int64_t>(p->max_extend_len) * a.group, p->dtype == RX_BF16, dk, idx64, linear, s);
    return check_launch("rx_extend_attn_mx4");
  }
  if (p->dtype == RX_BF16) {
    if (dk == 64) launch_extend_mx4<BF16, 64>(a, idx64, linear, s);
    else launch_extend_mx4<BF16, 128>(a, idx64, linear, s);
  } else {
    if (dk == 64) launch_extend_mx4<F16, 64>(a, idx64, linear, s);
    else launch_extend_mx4<F16, 128>(a, idx64, linear, s);
  }
  return check_launch("rx_extend_attn_mx4");
}

extern "C" int rx_extend_attn_mx4(const rx_extend_params* p, const rx_kv_mx4_scales* sc, void* stream) {
  RX_RANGE("rx_extend_attn_mx4");
  return rx::dump_on_error("extend_attn_mx4", extend_attn_mx4_impl(p, sc, stream), p, p ? sizeof(*p) : 0);
}
