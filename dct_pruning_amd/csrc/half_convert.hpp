// half_convert.hpp - the exact upcast of a 2-byte element, shared by the units that read fp16 / bf16 maps (half.hip, nhwc.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dctscore.h"

namespace {

// the low 16 bits of `bits` as an fp16 (DT == DCTS_DTYPE_F16) or bfloat16 element, exactly, in fp32
template <int DT>
__device__ __forceinline__ float half_to_float(unsigned bits) {
  if constexpr (DT == DCTS_DTYPE_F16) {
    const unsigned short h = (unsigned short)bits;
    return (float)__builtin_bit_cast(_Float16, h);
  } else {
    return __builtin_bit_cast(float, bits << 16);
  }
}

}  // namespace
