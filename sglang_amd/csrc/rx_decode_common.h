// Device helpers shared by the decode attention kernels (rx_decode.hip, rx_kv_mx4.hip): the tile geometry, the split
// ranges of the kv-split schedule, slot addressing and the V tile's LDS swizzle.
#pragma once
#include "rx_common.h"

namespace rx {

// Grok temperature factor of a request (decode_attention.py:156-160): the single query sits at seq_len-1
__device__ __forceinline__ float xai_factor(int32_t xai_len, int32_t seq_len) {
  const int32_t qidx = seq_len - 1;
  if (xai_len <= 0 || qidx <= xai_len) return 1.0f;
  return __log2f(static_cast<float>(qidx)) / __log2f(static_cast<float>(xai_len));
}

constexpr int kMinBlockKV = 32;  // decode_attention.py:36 (_MIN_BLOCK_KV)
constexpr int kTile = 32;        // tokens per wave tile (K of the PV MFMA)
constexpr int kWavesPerWG = 4;

// XOR swizzle of the 16-byte chunk index inside a V row of the LDS tile.  Makes both the
// ds_write_b128 of 8 consecutive rows and the ds_read_b64_tr_b16 of an 8-row x 32-byte
// window conflict-free (bank = addr/4 mod 32 for writes, mod 64 for tr reads).
template <int D>
__device__ __forceinline__ int v_swizzle(int row) {
  if constexpr (D == 64) return row & 7;
  return ((row & 7) << 1) | ((row >> 2) & 1);
}

template <bool LINEAR>
__device__ __forceinline__ int64_t slot_offset(int64_t slot, int32_t page_size,
                                               int64_t page_stride, int64_t tok_stride) {
  if constexpr (LINEAR) return mul_u32(slot, tok_stride);
  // page_size < 0 encodes a power-of-two page: -(log2(page) + 1)  (shift/mask instead of div/mod)
  if (page_size < 0) {
    const int sh = -page_size - 1;
    return mul_u32(slot >> sh, page_stride) + mul_u32(slot & ((1 << sh) - 1), tok_stride);
  }
  return (slot / page_size) * page_stride + (slot % page_size) * tok_stride;
}

__device__ __forceinline__ void split_range(int32_t seq_len, int32_t splits, int32_t split,
                                            int32_t& lo, int32_t& hi) {
  // decode_attention.py:466-472
  const int32_t per =
      ((seq_len + splits - 1) / splits + kMinBlockKV - 1) / kMinBlockKV * kMinBlockKV;
  lo = per * split;
  hi = min(lo + per, seq_len);
}

}  // namespace rx
