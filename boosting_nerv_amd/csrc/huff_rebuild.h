// huff_rebuild.h -- the de-quantisation of one 8-bit code of a post-hoc quantised tensor, shared by every kernel that writes one
// (huff.hip, huffz.hip, hufft.hip): the product and the sum as two IEEE fp32 operations, the expression hnerv_utils.quant_tensor and
// quant_tensor_sparse call `rebuilt` (see codec.hip on the pragma).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float rebuild1(float mn, float sc, unsigned q) {
#pragma clang fp contract(off)
    const float p = sc * (float)q;
    return mn + p;
}
