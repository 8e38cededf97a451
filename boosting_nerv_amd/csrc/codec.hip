// codec.hip -- the two device passes of the bitstream decoder (boosting_nerv_amd/codec.py).
//
// bnerv_dequant_table: the integer symbols the host rANS decoder produced, de-quantised straight into the model's parameter tensors
// (and, for HNeRV_Boost, into the [N, C, h, w] tensor of frame embeddings):  out[i] = float(q[i]) * scale  [+ beta].  These are the
// expressions the quantisers of the compression path evaluate with stock ops (lib/transform_ops.py: Scale_T `quant * scale`,
// ScaleBeta_T `quant * scale + beta`): ONE fp32 multiply and ONE fp32 add, never a fused multiply-add, so a decoded model holds the bits
// the encoder's evaluation ran with.  Up to BNERV_CEM_MAX_TENSORS tensors share a launch and every tensor is cut into chunks of
// BNERV_DEQUANT_CHUNK elements, one 256-thread block each (grid = chunks of the largest tensor x tensors; blocks beyond a tensor's end
// return) -- the grid of cem.hip.
//
// bnerv_frame_to_u8: a decoded frame batch [B, 3, H, W] fp32 planar -> [B, H, W, 3] uint8 interleaved, u = (uint8)(clamp(x, 0, 1) * 255 + 0.5)
// with the multiply and the add rounded separately (train_nerv_all._save_images: stock ops, four launches and a permuted copy).  A pure
// stream, 12 bytes in and 3 bytes out per pixel, no LDS: a thread takes 4 consecutive pixels -- three 16-byte plane loads, twelve bytes
// packed into three dwords.
#include "common.h"

namespace {

constexpr int DQ_CHUNK = BNERV_DEQUANT_CHUNK, DQ_THREADS = 256;
typedef int i32x4 __attribute__((ext_vector_type(4)));

// The products and sums below are written as plain operators under `fp contract(off)`: that pragma is what keeps the compiler from fusing them
// (the __fmul_rn / __fadd_rn of the HIP headers are inline `x * y` / `x + y` compiled with contraction allowed, and were fused into v_fma_f32).

__device__ __forceinline__ float dequant1(int q, float s, float b, bool has_beta) {
#pragma clang fp contract(off)
    const float v = (float)q * s;
    return has_beta ? v + b : v;
}

__global__ __launch_bounds__(DQ_THREADS) void dequant_table_kernel(const bnerv_dequant_chunk ck) {
    const bnerv_dequant_item it = ck.it[blockIdx.y];
    const int n = it.n, i0 = blockIdx.x * DQ_CHUNK, i1 = min(n, i0 + DQ_CHUNK);
    if (i0 >= n) return;
    const float s = it.scale[0];
    const bool has_beta = it.beta != nullptr;
    const float b = has_beta ? it.beta[0] : 0.0f;
    // 16-byte form: both operands start on a 16-byte boundary and n % 4 == 0 (i0 is a multiple of the chunk, so every quad is whole)
    const bool vec = (n % 4 == 0) && ((reinterpret_cast<uintptr_t>(it.q) | reinterpret_cast<uintptr_t>(it.out)) & 15) == 0;
    if (vec) {
        for (int i = i0 + (int)threadIdx.x * 4; i < i1; i += DQ_THREADS * 4) {
            const i32x4 q = *reinterpret_cast<const i32x4*>(it.q + i);
            *reinterpret_cast<f32x4*>(it.out + i) = f32x4{dequant1(q[0], s, b, has_beta), dequant1(q[1], s, b, has_beta),
                                                          dequant1(q[2], s, b, has_beta), dequant1(q[3], s, b, has_beta)};
        }
    } else {
        for (int i = i0 + (int)threadIdx.x; i < i1; i += DQ_THREADS) it.out[i] = dequant1(it.q[i], s, b, has_beta);
    }
}

__device__ __forceinline__ unsigned to_u8(float x) {
#pragma clang fp contract(off)
    const float v = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
    const float m = v * 255.0f;
    return (unsigned)(int)(m + 0.5f);                                // in [0.5, 255.5]: truncation lands in 0 .. 255
}

// grid = (blocks over one frame, B).  vec: one thread per quad of pixels (HW % 4 == 0, x on a 16-byte and out on a 4-byte boundary: every plane
// starts on a 16-byte boundary and the 12 output bytes of a quad start on a dword);  otherwise one thread per pixel
__global__ __launch_bounds__(256) void frame_to_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, const int HW, const int vec) {
    const int stride = (int)gridDim.x * 256;
    const float* src = x + (size_t)blockIdx.y * 3 * HW;
    unsigned char* dst = out + (size_t)blockIdx.y * 3 * HW;
    if (vec) {
        for (int p = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4; p < HW; p += stride * 4) {
            const f32x4 r = *reinterpret_cast<const f32x4*>(src + p), gr = *reinterpret_cast<const f32x4*>(src + HW + p),
                        bl = *reinterpret_cast<const f32x4*>(src + 2 * (size_t)HW + p);
            unsigned r_[4], g_[4], b_[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { r_[k] = to_u8(r[k]); g_[k] = to_u8(gr[k]); b_[k] = to_u8(bl[k]); }
            unsigned* d = reinterpret_cast<unsigned*>(dst + (size_t)p * 3);
            d[0] = r_[0] | (g_[0] << 8) | (b_[0] << 16) | (r_[1] << 24);
            d[1] = g_[1] | (b_[1] << 8) | (r_[2] << 16) | (g_[2] << 24);
            d[2] = b_[2] | (r_[3] << 8) | (g_[3] << 16) | (b_[3] << 24);
        }
    } else {
        for (int p = (int)blockIdx.x * 256 + (int)threadIdx.x; p < HW; p += stride) {
            unsigned char* d = dst + (size_t)p * 3;
            d[0] = (unsigned char)to_u8(src[p]);
            d[1] = (unsigned char)to_u8(src[HW + p]);
            d[2] = (unsigned char)to_u8(src[2 * (size_t)HW + p]);
        }
    }
}

}  // namespace

extern "C" int bnerv_dequant_table(void* stream, const bnerv_dequant_chunk* ck) {
    BNERV_REQUIRE(ck && ck->n_items > 0 && ck->n_items <= BNERV_CEM_MAX_TENSORS, "dequant_table: bad chunk");
    int max_n = 1;
    for (int i = 0; i < ck->n_items; ++i) {
        const bnerv_dequant_item& it = ck->it[i];
        BNERV_REQUIRE(it.q && it.out && it.scale && it.n > 0, "dequant_table: item %d incomplete", i);
        BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(it.q) | reinterpret_cast<uintptr_t>(it.out) | reinterpret_cast<uintptr_t>(it.scale) |
                        reinterpret_cast<uintptr_t>(it.beta)) & 3) == 0, "dequant_table: item %d is not 4-byte aligned", i);
        max_n = it.n > max_n ? it.n : max_n;
    }
    hipLaunchKernelGGL(dequant_table_kernel, dim3(cdiv(max_n, DQ_CHUNK), ck->n_items), dim3(DQ_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *ck);
    BNERV_LAUNCH_CHECK("dequant_table");
    return BNERV_OK;
}

extern "C" int bnerv_frame_to_u8(void* stream, const float* x, unsigned char* out, int B, int H, int W) {
    BNERV_REQUIRE(x && out, "frame_to_u8: null args");
    BNERV_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (size_t)H * W <= 0x7fffffffu / 4, "frame_to_u8: B=%d H=%d W=%d", B, H, W);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0, "frame_to_u8: x is not 4-byte aligned");
    const int HW = H * W;
    const int vec = (HW % 4 == 0) && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    const int blocks = cdiv(vec ? HW / 4 : HW, 256);
    hipLaunchKernelGGL(frame_to_u8_kernel, dim3(blocks > 16384 ? 16384 : blocks, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, out, HW, vec);
    BNERV_LAUNCH_CHECK("frame_to_u8");
    return BNERV_OK;
}
