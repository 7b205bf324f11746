// The 4-bit (MXFP4 block-16) format's device helpers shared by rx_kv_mx4.hip and rx_decode_mla_mx4.hip: the exact
// unpack in registers and the (data, scales) buffer pair.  include/radix_hip.h "4-bit KV pool" states the format.
#pragma once
#include "rx_common.h"

namespace rx {

// 2^(scale byte - 127) as the f32 operand of the scaled converts
__device__ __forceinline__ float mx4_scale_f32(uint32_t byte) { return __builtin_bit_cast(float, byte << 23); }

// one dword = eight e2m1 nibbles (element 2 i in the low nibble of byte i) -> eight 16-bit floats of T, times `scale`
template <typename T>
__device__ __forceinline__ u32x4 mx4x8_to_16(uint32_t dw, float scale) {
  u32x4 out;
  if constexpr (__is_same(typename T::scalar, __bf16)) {
    out[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 0));
    out[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 1));
    out[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 2));
    out[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 3));
  } else {
    out[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(dw, scale, 0));
    out[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(dw, scale, 1));
    out[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(dw, scale, 2));
    out[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(dw, scale, 3));
  }
  return out;
}

struct Mx4Pool {  // a data buffer and its scale buffer, byte strides
  uint8_t* data;
  uint8_t* scales;
  int64_t dps, dts, dhs;  // data page / token / head stride
  int64_t sps, sts, shs;  // scales
};

inline Mx4Pool mx4_pool(const void* data, const void* scales, int64_t dps, int64_t dts, int64_t dhs, int64_t sps, int64_t sts,
                        int64_t shs) {
  Mx4Pool p;
  p.data = static_cast<uint8_t*>(const_cast<void*>(data));
  p.scales = static_cast<uint8_t*>(const_cast<void*>(scales));
  p.dps = dps; p.dts = dts; p.dhs = dhs;
  p.sps = sps; p.sts = sts; p.shs = shs;
  return p;
}

// rx_extend_attn_mx4's launch arguments: extend_mx4_kernel (rx_extend_mx4.hip) and cascade_mx4_kernel (rx_cascade_mx4.hip)
struct Mx4ExtendArgs {
  const uint16_t* q;
  const uint16_t* k_ext;
  const uint16_t* v_ext;
  uint16_t* o;
  int64_t q_stride_t, q_stride_h, k_stride_t, k_stride_h, v_stride_t, v_stride_h, o_stride_t, o_stride_h;
  Mx4Pool k, v;
  int32_t page_size;  // >= 1, or -(log2(page) + 1) for a power-of-two page (slot_offset)
  const void* qo_indptr;
  int32_t qo64;
  const int32_t* kv_indptr;
  const void* kv_indices;
  float* lse;
  int64_t lse_stride_t, lse_stride_h;
  int32_t bs, hkv, group, mblocks;
  float sm_scale, k_scale, v_scale, logit_cap;
  int32_t causal, skip_extend;
};

}  // namespace rx
