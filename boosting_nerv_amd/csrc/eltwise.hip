// eltwise.hip -- streaming helpers: the output head's backward, the GELU of the HNeRV baseline, and the inpainting mask passes.
//
// bnerv_tanh_grad: gt = g * d/dv [tanh(v) * 0.5 + 0.5] written out once, with its per-channel sums (the head's bias gradient) as per-block
// partials.  OutImg (reference model_blocks.py:57-63) maps the head conv's output v to img = tanh(v) * 0.5 + 0.5, so with t = 2 img - 1 the
// factor is 0.5 (1 - t^2) -- the same expression as the conv kernels' IN_TANHGRAD prologue (conv_common.h xform1).  HNeRV_Boost's 3x3
// head (38 -> 3, model_hnerv.py:214) takes its weight gradient with the roles of input and gradient SWAPPED (ops._HeadTanh.backward: M = the
// 38 input channels, N = 3 couts x 9 taps instead of 3 of 16 MFMA rows), which needs gt as a plain tensor.
#include "common.h"

namespace {
constexpr int TG_PER_BLOCK = 8192;      // elements of one plane per block (256 threads x 8 float4)

__global__ __launch_bounds__(256) void tanh_grad_kernel(const float* __restrict__ g, const float* __restrict__ img, float* __restrict__ gt,
                                                        float* __restrict__ part, int C, int HW, int nblk, const int vec) {
    __shared__ float s_red[4];
    const int bc = blockIdx.y, blk = blockIdx.x;
    const size_t base = (size_t)bc * HW;
    const int e0 = blk * TG_PER_BLOCK;
    float acc = 0.f;
    if (vec) {
#pragma unroll
        for (int u = 0; u < TG_PER_BLOCK / 1024; ++u) {
            const int e = e0 + (u * 256 + (int)threadIdx.x) * 4;
            if (e < HW) {
                const f32x4 gv = *reinterpret_cast<const f32x4*>(g + base + e), iv = *reinterpret_cast<const f32x4*>(img + base + e);
                f32x4 r;
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float t = 2.0f * iv[k] - 1.0f; r[k] = gv[k] * 0.5f * (1.0f - t * t); }
                *reinterpret_cast<f32x4*>(gt + base + e) = r;
                acc += (r[0] + r[1]) + (r[2] + r[3]);
            }
        }
    } else {
        for (int e = e0 + (int)threadIdx.x; e < min(HW, e0 + TG_PER_BLOCK); e += 256) {
            const float t = 2.0f * img[base + e] - 1.0f;
            const float r = g[base + e] * 0.5f * (1.0f - t * t);
            gt[base + e] = r;
            acc += r;
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int b = bc / C, c = bc - b * C;
        part[((size_t)b * nblk + blk) * C + c] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    }
}

// y = gelu(u), gp = gelu'(u) (gp may be NULL), in place allowed; and du = g * gp: the GELU of the HNeRV baseline's 1x1 / 3x3 stages
// (NeRVBlock, model_blocks.py:34-46 with act = 'gelu') around the existing EP_BIAS (+ PixelShuffle) convolutions.
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* __restrict__ u, float* __restrict__ y, float* __restrict__ gp, const size_t n, const int vec) {
    const size_t stride = (size_t)gridDim.x * 256;
    if (vec) {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n / 4; i += stride) {
            f32x4 h, g;
            gelu_pair4_f(reinterpret_cast<const f32x4*>(u)[i], &h, &g);
            reinterpret_cast<f32x4*>(y)[i] = h;
            if (gp) reinterpret_cast<f32x4*>(gp)[i] = g;
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            float h, g;
            gelu_pair_f(u[i], &h, &g);
            y[i] = h;
            if (gp) gp[i] = g;
        }
    }
}
__global__ __launch_bounds__(256) void mul_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, const size_t n, const int vec) {
    const size_t stride = (size_t)gridDim.x * 256;
    if (vec) {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n / 4; i += stride)
            reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(a)[i] * reinterpret_cast<const f32x4*>(b)[i];
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = a[i] * b[i];
    }
}
static int stream_grid(size_t n) { const size_t b = (n + 1023) / 1024; return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b)); }

// ---- inpainting: an [H, W] mask broadcast over the B * C planes of a frame (reference train_nerv_all.py:343 loss_fn(out * mask, gt * mask),
// hnerv_utils.py:59-84 TransformInput).  A flat grid of (plane, block of IP_PER_BLOCK elements of the plane); every product is ONE fp32
// multiply, so the loss kernels behind see the bits torch's `x * mask` gives them.  vec: every plane starts on a 16-byte boundary.
constexpr int IP_PER_BLOCK = 4096;      // 256 threads x 4 float4

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }      // (a NaN stays a NaN, as torch.clamp)

// OP 0: gt_m = img * mask (+ inp = clamp(img * mask, 0, 1) when inp != NULL);  OP 1: pred_m = pred * mask, part = block sum of (pred - gt)^2;
// OP 2: g *= mask in place.  a: img | pred | g;  b: gt (OP 1);  o0: gt_m | pred_m | g;  o1: inp (OP 0)
// (a and o0 are the same buffer in OP 2: neither is __restrict__; every thread reads its elements before it writes them)
template <int OP>
__global__ __launch_bounds__(256) void inpaint_kernel(const float* a, const float* __restrict__ b, const float* __restrict__ mask,
                                                      float* o0, float* __restrict__ o1, double* __restrict__ part, const int HW,
                                                      const int nblk, const int vec) {
    const int bc = (int)blockIdx.x / nblk, blk = (int)blockIdx.x - bc * nblk;
    const size_t base = (size_t)bc * HW;
    const int e0 = blk * IP_PER_BLOCK;
    double acc = 0.0;
    if (vec) {
#pragma unroll
        for (int u = 0; u < IP_PER_BLOCK / 1024; ++u) {
            const int e = e0 + (u * 256 + (int)threadIdx.x) * 4;
            if (e < HW) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(a + base + e), mv = *reinterpret_cast<const f32x4*>(mask + e);
                const f32x4 r = av * mv;
                *reinterpret_cast<f32x4*>(o0 + base + e) = r;
                if (OP == 0 && o1) *reinterpret_cast<f32x4*>(o1 + base + e) = f32x4{clamp01(r[0]), clamp01(r[1]), clamp01(r[2]), clamp01(r[3])};
                if (OP == 1) {
                    const f32x4 d = av - *reinterpret_cast<const f32x4*>(b + base + e);
                    acc += ((double)d[0] * (double)d[0] + (double)d[1] * (double)d[1]) + ((double)d[2] * (double)d[2] + (double)d[3] * (double)d[3]);
                }
            }
        }
    } else {
        for (int e = e0 + (int)threadIdx.x; e < min(HW, e0 + IP_PER_BLOCK); e += 256) {
            const float av = a[base + e];
            const float r = av * mask[e];
            o0[base + e] = r;
            if (OP == 0 && o1) o1[base + e] = clamp01(r);
            if (OP == 1) {
                const float d = av - b[base + e];
                acc += (double)d * (double)d;
            }
        }
    }
    if (OP == 1) {
        __shared__ double s_red[4];
        acc = wave_sum_d(acc);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) part[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);      // [b][c * nblk + blk]
    }
}

// one wave per sample: lane l adds partials l, l + 64, ..., then a wave tree -- fixed order; psnr_fn_single (hnerv_utils.py:400-403)
__global__ __launch_bounds__(64) void inpaint_psnr_kernel(const double* __restrict__ part, float* __restrict__ psnr, const int stride, const int n_part,
                                                          const int n_per_sample) {
    const int b = blockIdx.x;
    double s2 = 0.0;
    for (int k = threadIdx.x; k < n_part; k += 64) s2 += part[(size_t)b * n_part + k];
    s2 = wave_sum_d(s2);
    if (threadIdx.x == 0) {
        const float mse = (float)(s2 / (double)n_per_sample);
        psnr[(size_t)b * stride] = -10.0f * log10f(mse + 1e-9f);
    }
}

static int inpaint_dims_ok(int B, int C, int HW) { return B > 0 && C > 0 && HW > 0 && (size_t)B * C * cdiv(HW, IP_PER_BLOCK) <= 0x7fffffffu; }
static int inpaint_vec(int HW, const void* p0, const void* p1, const void* p2, const void* p3, const void* p4) {
    return (HW % 4 == 0) && ((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2) |
                              reinterpret_cast<uintptr_t>(p3) | reinterpret_cast<uintptr_t>(p4)) & 15) == 0;
}
}  // namespace

extern "C" int bnerv_inpaint_head(void* stream, const float* img, const float* mask, float* inp, float* gt_m, int B, int C, int HW) {
    BNERV_REQUIRE(img && mask && gt_m, "inpaint_head: null args");
    BNERV_REQUIRE(inpaint_dims_ok(B, C, HW), "inpaint_head: B=%d C=%d HW=%d", B, C, HW);
    const int nblk = cdiv(HW, IP_PER_BLOCK);
    hipLaunchKernelGGL(inpaint_kernel<0>, dim3(B * C * nblk), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), img, (const float*)nullptr, mask, gt_m, inp,
                       (double*)nullptr, HW, nblk, inpaint_vec(HW, img, mask, gt_m, inp, nullptr));
    BNERV_LAUNCH_CHECK("inpaint_head");
    return BNERV_OK;
}

extern "C" size_t bnerv_inpaint_ws_bytes(int B, int C, int HW) {
    return inpaint_dims_ok(B, C, HW) ? (size_t)B * C * cdiv(HW, IP_PER_BLOCK) * sizeof(double) : 0;
}

extern "C" int bnerv_inpaint_pred(void* stream, const float* pred, const float* gt, const float* mask, float* pred_m, void* ws, size_t ws_bytes,
                                  int B, int C, int HW) {
    BNERV_REQUIRE(pred && gt && mask && pred_m && ws, "inpaint_pred: null args");
    BNERV_REQUIRE(inpaint_dims_ok(B, C, HW), "inpaint_pred: B=%d C=%d HW=%d", B, C, HW);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "inpaint_pred: ws must be 8-byte aligned (doubles)");
    if (ws_bytes < bnerv_inpaint_ws_bytes(B, C, HW)) return bnerv_set_error(BNERV_E_WS, "inpaint_pred: workspace %zu < %zu", ws_bytes, bnerv_inpaint_ws_bytes(B, C, HW));
    const int nblk = cdiv(HW, IP_PER_BLOCK);
    hipLaunchKernelGGL(inpaint_kernel<1>, dim3(B * C * nblk), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), pred, gt, mask, pred_m, (float*)nullptr,
                       reinterpret_cast<double*>(ws), HW, nblk, inpaint_vec(HW, pred, gt, mask, pred_m, nullptr));
    BNERV_LAUNCH_CHECK("inpaint_pred");
    return BNERV_OK;
}

extern "C" int bnerv_inpaint_psnr(void* stream, const void* ws, size_t ws_bytes, float* psnr, int stride, int B, int C, int HW) {
    BNERV_REQUIRE(ws && psnr && stride > 0, "inpaint_psnr: bad args");
    BNERV_REQUIRE(inpaint_dims_ok(B, C, HW), "inpaint_psnr: B=%d C=%d HW=%d", B, C, HW);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "inpaint_psnr: ws must be 8-byte aligned (doubles)");
    if (ws_bytes < bnerv_inpaint_ws_bytes(B, C, HW)) return bnerv_set_error(BNERV_E_WS, "inpaint_psnr: workspace %zu < %zu", ws_bytes, bnerv_inpaint_ws_bytes(B, C, HW));
    hipLaunchKernelGGL(inpaint_psnr_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const double*>(ws), psnr, stride,
                       C * cdiv(HW, IP_PER_BLOCK), C * HW);
    BNERV_LAUNCH_CHECK("inpaint_psnr");
    return BNERV_OK;
}

extern "C" int bnerv_inpaint_grad(void* stream, float* g, const float* mask, int B, int C, int HW) {
    BNERV_REQUIRE(g && mask, "inpaint_grad: null args");
    BNERV_REQUIRE(inpaint_dims_ok(B, C, HW), "inpaint_grad: B=%d C=%d HW=%d", B, C, HW);
    const int nblk = cdiv(HW, IP_PER_BLOCK);
    hipLaunchKernelGGL(inpaint_kernel<2>, dim3(B * C * nblk), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, (const float*)nullptr, mask, g, (float*)nullptr,
                       (double*)nullptr, HW, nblk, inpaint_vec(HW, g, mask, nullptr, nullptr, nullptr));
    BNERV_LAUNCH_CHECK("inpaint_grad");
    return BNERV_OK;
}

extern "C" int bnerv_gelu_fwd(void* stream, const float* u, float* y, float* gp, size_t n) {
    BNERV_REQUIRE(u && y && n > 0, "gelu_fwd: bad args");
    const int vec = (n % 4 == 0) && ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gp)) & 15) == 0;
    hipLaunchKernelGGL(gelu_fwd_kernel, dim3(stream_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), u, y, gp, n, vec);
    BNERV_LAUNCH_CHECK("gelu_fwd");
    return BNERV_OK;
}

extern "C" int bnerv_mul(void* stream, const float* a, const float* b, float* out, size_t n) {
    BNERV_REQUIRE(a && b && out && n > 0, "mul: bad args");
    const int vec = (n % 4 == 0) && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    hipLaunchKernelGGL(mul_kernel, dim3(stream_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, b, out, n, vec);
    BNERV_LAUNCH_CHECK("mul");
    return BNERV_OK;
}

extern "C" int bnerv_tanh_grad_blocks(int HW) { return HW > 0 ? cdiv(HW, TG_PER_BLOCK) : 0; }

// gt [B, C, HW] = g * 0.5 (1 - (2 img - 1)^2); part [B * bnerv_tanh_grad_blocks(HW)][C]: per-block channel sums of gt, to be summed over
// their first index (bnerv_reduce_slabs / _deferred with n_slabs = B * blocks, count = C) into the bias gradient
extern "C" int bnerv_tanh_grad(void* stream, const float* g, const float* img, float* gt, float* part, int B, int C, int HW) {
    BNERV_REQUIRE(g && img && gt && part && B > 0 && C > 0 && HW > 0, "tanh_grad: bad args");
    BNERV_REQUIRE((size_t)B * C <= 65535, "tanh_grad: B * C too large");
    // float4 form: every plane starts on a 16-byte boundary (HW % 4 == 0 and aligned tensors); otherwise the scalar loop
    const int vec = (HW % 4 == 0) && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(gt)) & 15) == 0;
    const int nblk = cdiv(HW, TG_PER_BLOCK);
    hipLaunchKernelGGL(tanh_grad_kernel, dim3(nblk, B * C), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, img, gt, part, C, HW, nblk, vec);
    BNERV_LAUNCH_CHECK("tanh_grad");
    return BNERV_OK;
}
