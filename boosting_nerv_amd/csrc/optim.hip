// optim.hip -- fused multi-tensor Adan / Adam step, the device-side global-norm gradient clip in front of it, and the flat-bucket
// gather/scatter used by the data-parallel exchange.
//
// Adan semantics follow the reference's default path exactly (optimizer.py:296-362 `_multi_tensor_adan`, called from
// Adan.step optimizer.py:125-235 with betas (0.98, 0.92, 0.99), eps 1e-8, weight_decay 0, no clipping), one pass over
// p, g, exp_avg, exp_avg_sq, exp_avg_diff, neg_pre_grad = 6 reads + 5 writes of 4 B per parameter (44 B/param),
// instead of ~17 torch._foreach launches.  The operation ORDER of the reference is kept so the result matches the
// foreach path to fp32 rounding:
//     g *= clip;  t = neg_pre_grad + g (= g - g_prev);  m = m*b1 + (1-b1) g;  d = d*b2 + (1-b2) t;
//     t = t*b2 + g;  n = n*b3 + (1-b3) t*t;  denom = sqrt(n)/sqrt(bc3) + eps;
//     p -= (lr/bc1) m/denom;  p -= (lr*b2/bc2) d/denom;  p /= (1 + lr*wd);  neg_pre_grad = -g
#include "common.h"
#include "sidejob.h"

namespace {
__device__ __forceinline__ int cdiv_dev(int a, int b) { return (a + b - 1) / b; }

// bstart[t] = first block of tensor t in the flat grid (tensor t owns min(ceil(n_t / 1024), 1024) blocks): a (blocks of the largest
// tensor) x (tensors) grid launched 48 x 1024 blocks for the chunk that holds the 1.1 M-element stem matrix, ~1500 of them with work
struct AdanArgs { bnerv_adan_chunk c; bnerv_adan_hyper h; int bstart[BNERV_ADAN_MAX_TENSORS + 1]; };

__global__ __launch_bounds__(256) void adan_kernel(const AdanArgs a) {
    int t = 0;
    for (int hi = a.c.n_tensors; hi - t > 1;) {            // (uniform: scalar loads from the kernel arguments)
        const int mid = (t + hi) >> 1;
        if ((int)blockIdx.x >= a.bstart[mid]) t = mid; else hi = mid;
    }
    const int bx = (int)blockIdx.x - a.bstart[t], gx = a.bstart[t + 1] - a.bstart[t];
    const int n = a.c.n[t];
    float* __restrict__ p = a.c.p[t];
    const float* __restrict__ g = a.c.g[t];
    float* __restrict__ m = a.c.exp_avg[t];
    float* __restrict__ v = a.c.exp_avg_sq[t];
    float* __restrict__ d = a.c.exp_avg_diff[t];
    float* __restrict__ ng = a.c.neg_pre_grad[t];
    const float lr = a.h.sched_dev[0], bc1 = a.h.sched_dev[1], bc2 = a.h.sched_dev[2], bc3s = a.h.sched_dev[3];
    const bool first = a.h.sched_dev[4] != 0.f;
    const float b1 = a.h.beta1, b2 = a.h.beta2, b3 = a.h.beta3, eps = a.h.eps, wd = a.h.weight_decay, clip = a.h.clip_global_grad_norm;
    const float step_size = lr / bc1, step_size_diff = lr * b2 / bc2;
    for (int i = bx * 256 + threadIdx.x; i < n; i += gx * 256) {
        const float gi = g[i] * clip;
        float t0 = (first ? -gi : ng[i]) + gi;                       // g - g_prev   (0 on the first step)
        const float mi = m[i] * b1 + (1.0f - b1) * gi;
        const float di = d[i] * b2 + (1.0f - b2) * t0;
        t0 = t0 * b2 + gi;
        const float vi = v[i] * b3 + (1.0f - b3) * (t0 * t0);
        const float denom = sqrtf(vi) / bc3s + eps;
        float pi = p[i];
        if (a.h.no_prox) {
            pi *= (1.0f - lr * wd);
            pi += -step_size * (mi / denom);
            pi += -step_size_diff * (di / denom);
        } else {
            pi += -step_size * (mi / denom);
            pi += -step_size_diff * (di / denom);
            pi /= (1.0f + lr * wd);
        }
        p[i] = pi; m[i] = mi; v[i] = vi; d[i] = di; ng[i] = -gi;
    }
}

__device__ __forceinline__ void adan_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            float* __restrict__ d, float* __restrict__ ng, int n, int bx, int gx, const bnerv_adan_hyper& h) {
    const float lr = h.sched_dev[0], bc1 = h.sched_dev[1], bc2 = h.sched_dev[2], bc3s = h.sched_dev[3];
    const bool first = h.sched_dev[4] != 0.f;
    const float b1 = h.beta1, b2 = h.beta2, b3 = h.beta3, eps = h.eps, wd = h.weight_decay, clip = h.clip_global_grad_norm;
    const float step_size = lr / bc1, step_size_diff = lr * b2 / bc2;
    for (int i = bx * 256 + threadIdx.x; i < n; i += gx * 256) {
        const float gi = g[i] * clip;
        float t0 = (first ? -gi : ng[i]) + gi;                       // g - g_prev   (0 on the first step)
        const float mi = m[i] * b1 + (1.0f - b1) * gi;
        const float di = d[i] * b2 + (1.0f - b2) * t0;
        t0 = t0 * b2 + gi;
        const float vi = v[i] * b3 + (1.0f - b3) * (t0 * t0);
        const float denom = sqrtf(vi) / bc3s + eps;
        float pi = p[i];
        if (h.no_prox) {
            pi *= (1.0f - lr * wd);
            pi += -step_size * (mi / denom);
            pi += -step_size_diff * (di / denom);
        } else {
            pi += -step_size * (mi / denom);
            pi += -step_size_diff * (di / denom);
            pi /= (1.0f + lr * wd);
        }
        p[i] = pi; m[i] = mi; v[i] = vi; d[i] = di; ng[i] = -gi;
    }
}

// table form: the tensor of a block is found by bisection over bstart in device memory (uniform addresses: scalar loads)
__global__ __launch_bounds__(256) void adan_table_kernel(const bnerv_adan_entry* __restrict__ tab, const int n_tensors, const bnerv_adan_hyper h) {
    int t = 0;
    for (int hi = n_tensors; hi - t > 1;) {
        const int mid = (t + hi) >> 1;
        if ((int)blockIdx.x >= tab[mid].bstart) t = mid; else hi = mid;
    }
    const bnerv_adan_entry e = tab[t];
    const int gx = min(cdiv_dev(e.n, 256 * 4), 1024);
    adan_update(e.p, e.g, e.exp_avg, e.exp_avg_sq, e.exp_avg_diff, e.neg_pre_grad, e.n, (int)blockIdx.x - e.bstart, gx, h);
}

// Fused Adam (torch.optim.Adam defaults: no weight decay, no amsgrad; torch/optim/adam.py _single_tensor_adam order of operations):
//   m = m + (1 - b1) (g - m);  v = v b2 + (1 - b2) g g;  denom = sqrt(v) / sqrt(bc2) + eps;  p = p - (lr / bc1) (m / denom)
// sched_dev = {lr, bias_correction1, sqrt(bias_correction2), 1 - b1, 1 - b2}: read from device memory, so a captured step replays with a moving
// step count.  The two complements come from the host, rounded from their float64 values as torch's kernels receive them (1.0f - 0.999f is
// 4.7e-5 off 0.001).
// Same device table as the Adan table form (exp_avg_diff / neg_pre_grad unused).
__global__ __launch_bounds__(256) void adam_table_kernel(const bnerv_adan_entry* __restrict__ tab, const int n_tensors, const bnerv_adan_hyper h) {
#pragma clang fp contract(off)
    int t = 0;
    for (int hi = n_tensors; hi - t > 1;) {
        const int mid = (t + hi) >> 1;
        if ((int)blockIdx.x >= tab[mid].bstart) t = mid; else hi = mid;
    }
    const bnerv_adan_entry e = tab[t];
    const int gx = min(cdiv_dev(e.n, 256 * 4), 1024), bx = (int)blockIdx.x - e.bstart;
    const float lr = h.sched_dev[0], bc1 = h.sched_dev[1], bc2s = h.sched_dev[2], omb1 = h.sched_dev[3], omb2 = h.sched_dev[4];
    const float b2 = h.beta2, eps = h.eps;
    const float step_size = lr / bc1;
    float* __restrict__ p = e.p;
    const float* __restrict__ g = e.g;
    float* __restrict__ m = e.exp_avg;
    float* __restrict__ v = e.exp_avg_sq;
    for (int i = bx * 256 + threadIdx.x; i < e.n; i += gx * 256) {
        const float gi = g[i];
        const float mi = m[i] + omb1 * (gi - m[i]);
        const float vi = v[i] * b2 + omb2 * (gi * gi);
        const float denom = sqrtf(vi) / bc2s + eps;
        p[i] = p[i] + (-step_size) * (mi / denom);
        m[i] = mi; v[i] = vi;
    }
}

// Global-norm gradient clip over the same device table (torch.nn.utils.clip_grad_norm_ with its defaults; reference train_nerv_all.py:346-347):
//   total = sqrt(sum g^2);  coef = min(1, max_norm / (total + 1e-6));  g *= coef
// Two launches with the block partition of the optimizer kernels above, no atomics: each block leaves the sum of squares of its slice as one
// double, then every block re-adds ALL partials in one fixed order (lane l adds l, l + 64, ..., then a wave tree, as cem.hip's chunk_total),
// so all blocks scale by the same bits.  A gradient may start at any 4-byte boundary: 16-byte loads over the aligned body, the (at most three)
// elements before and after it go to the first block of the tensor.
struct GradSpan { int head, nq, tail0; };      // [0, head) | nq quads from head | [tail0, n)
__device__ __forceinline__ GradSpan grad_span(const float* g, int n) {
    GradSpan s;
    s.head = min(n, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) >> 2);
    s.nq = (n - s.head) >> 2;
    s.tail0 = s.head + s.nq * 4;
    return s;
}
__device__ __forceinline__ int table_tensor(const bnerv_adan_entry* __restrict__ tab, int n_tensors) {
    int t = 0;
    for (int hi = n_tensors; hi - t > 1;) {
        const int mid = (t + hi) >> 1;
        if ((int)blockIdx.x >= tab[mid].bstart) t = mid; else hi = mid;
    }
    return t;
}

__global__ __launch_bounds__(256) void grad_sqsum_table_kernel(const bnerv_adan_entry* __restrict__ tab, const int n_tensors, double* __restrict__ part) {
    __shared__ double red[4];
    const bnerv_adan_entry e = tab[table_tensor(tab, n_tensors)];
    const int gx = min(cdiv_dev(e.n, 256 * 4), 1024), bx = (int)blockIdx.x - e.bstart;
    const float* __restrict__ g = e.g;
    const GradSpan s = grad_span(g, e.n);
    const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g + s.head);
    double acc = 0.0;
    for (int i = bx * 256 + threadIdx.x; i < s.nq; i += gx * 256) {
        const f32x4 v = g4[i];
        acc += ((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1]) + ((double)v[2] * (double)v[2] + (double)v[3] * (double)v[3]);
    }
    if (bx == 0) {
        const int k = (int)threadIdx.x, edge = s.head + (e.n - s.tail0);      // <= 6 elements
        if (k < edge) {
            const float v = g[k < s.head ? k : s.tail0 + (k - s.head)];
            acc += (double)v * (double)v;
        }
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void grad_scale_table_kernel(const bnerv_adan_entry* __restrict__ tab, const int n_tensors, const double* __restrict__ part,
                                                               const int n_part, const float max_norm, float* __restrict__ out) {
    __shared__ float s_coef;
    if (threadIdx.x < 64) {
        double t = 0.0;
        for (int c = threadIdx.x; c < n_part; c += 64) t += part[c];
        t = wave_sum_d(t);
        if (threadIdx.x == 0) {
            const float total = (float)sqrt(t);
            const float coef = fminf(1.0f, max_norm / (total + 1e-6f));
            s_coef = coef;
            if (blockIdx.x == 0) { out[0] = total; out[1] = coef; }
        }
    }
    __syncthreads();
    const float coef = s_coef;
    const bnerv_adan_entry e = tab[table_tensor(tab, n_tensors)];
    const int gx = min(cdiv_dev(e.n, 256 * 4), 1024), bx = (int)blockIdx.x - e.bstart;
    float* __restrict__ g = const_cast<float*>(e.g);
    const GradSpan s = grad_span(g, e.n);
    f32x4* __restrict__ g4 = reinterpret_cast<f32x4*>(g + s.head);
    for (int i = bx * 256 + threadIdx.x; i < s.nq; i += gx * 256) g4[i] = g4[i] * coef;
    if (bx == 0) {
        const int k = (int)threadIdx.x, edge = s.head + (e.n - s.tail0);
        if (k < edge) g[k < s.head ? k : s.tail0 + (k - s.head)] *= coef;
    }
}

__global__ __launch_bounds__(256) void fetch_frame_kernel(const float* __restrict__ clip, const double* __restrict__ norms, const float* __restrict__ sel,
                                                          const int n_frames, const size_t frame_elems, float* __restrict__ dst, double* __restrict__ dst_norm) {
    fetch_frame_body(clip, norms, sel, n_frames, frame_elems, dst, dst_norm, (int)blockIdx.x, (int)gridDim.x);
}

struct BucketArgs { bnerv_bucket_chunk c; float* bucket; float scale; int to_bucket; int bstart[BNERV_ADAN_MAX_TENSORS * 2 + 1]; };

__global__ __launch_bounds__(256) void bucket_kernel(const BucketArgs a) {
    int t = 0;                                             // flat grid, as adan_kernel
    for (int hi = a.c.n_tensors; hi - t > 1;) {
        const int mid = (t + hi) >> 1;
        if ((int)blockIdx.x >= a.bstart[mid]) t = mid; else hi = mid;
    }
    const int bx = (int)blockIdx.x - a.bstart[t], gx = a.bstart[t + 1] - a.bstart[t];
    const int n = a.c.n[t];
    float* __restrict__ x = a.c.t[t];
    float* __restrict__ bk = a.bucket + a.c.off[t];
    for (int i = bx * 256 + threadIdx.x; i < n; i += gx * 256) {
        if (a.to_bucket) bk[i] = x[i] * a.scale;
        else x[i] = bk[i] * a.scale;
    }
}

}  // namespace

extern "C" int bnerv_adan_multi_tensor(void* stream, const bnerv_adan_chunk* chunk, const bnerv_adan_hyper* h) {
    BNERV_REQUIRE(chunk && h && h->sched_dev, "adan_multi_tensor: null args");
    BNERV_REQUIRE(chunk->n_tensors > 0 && chunk->n_tensors <= BNERV_ADAN_MAX_TENSORS, "adan_multi_tensor: n_tensors=%d", chunk->n_tensors);
    AdanArgs a;
    a.c = *chunk;
    a.h = *h;
    int blocks = 0;
    for (int i = 0; i < chunk->n_tensors; ++i) {
        BNERV_REQUIRE(chunk->p[i] && chunk->g[i] && chunk->exp_avg[i] && chunk->exp_avg_sq[i] && chunk->exp_avg_diff[i] && chunk->neg_pre_grad[i] && chunk->n[i] > 0,
                      "adan_multi_tensor: bad tensor %d", i);
        int gx = cdiv(chunk->n[i], 256 * 4);
        if (gx > 1024) gx = 1024;
        a.bstart[i] = blocks;
        blocks += gx;
    }
    for (int i = chunk->n_tensors; i <= BNERV_ADAN_MAX_TENSORS; ++i) a.bstart[i] = blocks;
    hipLaunchKernelGGL(adan_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    BNERV_LAUNCH_CHECK("adan");
    return BNERV_OK;
}

extern "C" int bnerv_adan_table_blocks(int n) {
    if (n <= 0) return 0;
    const int gx = cdiv(n, 256 * 4);
    return gx > 1024 ? 1024 : gx;
}

extern "C" int bnerv_adan_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, const bnerv_adan_hyper* h) {
    BNERV_REQUIRE(table_dev && h && h->sched_dev, "adan_table: null args");
    BNERV_REQUIRE(n_tensors > 0 && total_blocks > 0, "adan_table: n_tensors=%d total_blocks=%d", n_tensors, total_blocks);
    hipLaunchKernelGGL(adan_table_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev, n_tensors, *h);
    BNERV_LAUNCH_CHECK("adan_table");
    return BNERV_OK;
}

extern "C" int bnerv_adam_table_blocks(int n) { return bnerv_adan_table_blocks(n); }

extern "C" int bnerv_adam_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, const bnerv_adan_hyper* h) {
    BNERV_REQUIRE(table_dev && h && h->sched_dev, "adam_table: null args");
    BNERV_REQUIRE(n_tensors > 0 && total_blocks > 0, "adam_table: n_tensors=%d total_blocks=%d", n_tensors, total_blocks);
    BNERV_REQUIRE(h->beta1 >= 0.f && h->beta1 < 1.f && h->beta2 >= 0.f && h->beta2 < 1.f && h->eps >= 0.f, "adam_table: bad hyper-parameters");
    hipLaunchKernelGGL(adam_table_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev, n_tensors, *h);
    BNERV_LAUNCH_CHECK("adam_table");
    return BNERV_OK;
}

extern "C" int bnerv_grad_sqsum_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, double* partials) {
    BNERV_REQUIRE(table_dev && partials, "grad_sqsum_table: null args");
    BNERV_REQUIRE(n_tensors > 0 && total_blocks > 0, "grad_sqsum_table: n_tensors=%d total_blocks=%d", n_tensors, total_blocks);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "grad_sqsum_table: partials must be 8-byte aligned (doubles)");
    hipLaunchKernelGGL(grad_sqsum_table_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev, n_tensors, partials);
    BNERV_LAUNCH_CHECK("grad_sqsum_table");
    return BNERV_OK;
}

extern "C" int bnerv_grad_scale_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, const double* partials,
                                      int n_partials, float max_norm, float* out) {
    BNERV_REQUIRE(table_dev && partials && out, "grad_scale_table: null args");
    BNERV_REQUIRE(n_tensors > 0 && total_blocks > 0 && n_partials >= total_blocks, "grad_scale_table: n_tensors=%d total_blocks=%d n_partials=%d",
                  n_tensors, total_blocks, n_partials);
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "grad_scale_table: partials must be 8-byte aligned (doubles)");
    BNERV_REQUIRE(max_norm >= 0.f, "grad_scale_table: max_norm=%g", (double)max_norm);
    hipLaunchKernelGGL(grad_scale_table_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev, n_tensors, partials, n_partials, max_norm, out);
    BNERV_LAUNCH_CHECK("grad_scale_table");
    return BNERV_OK;
}

extern "C" int bnerv_fetch_frame(void* stream, const float* clip, const double* norms, const float* sel_dev, int n_frames, size_t frame_elems,
                                 float* dst_img, double* dst_norm) {
    BNERV_REQUIRE(clip && sel_dev && dst_img && n_frames > 0 && frame_elems > 0, "fetch_frame: bad args");
    BNERV_REQUIRE((reinterpret_cast<uintptr_t>(clip) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst_img) & 15) == 0, "fetch_frame: clip and dst_img must be 16-byte aligned");
    BNERV_REQUIRE(frame_elems % 4 == 0 || n_frames == 1, "fetch_frame: frame_elems must be a multiple of 4 when n_frames > 1 (16-byte aligned frames)");
    const size_t n4 = frame_elems / 4;
    int blocks = (int)((n4 + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(fetch_frame_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, clip, norms, sel_dev, n_frames, frame_elems, dst_img, dst_norm);
    BNERV_LAUNCH_CHECK("fetch_frame");
    return BNERV_OK;
}

static int bucket_launch(void* stream, const bnerv_bucket_chunk* c, float* bucket, float scale, int to_bucket) {
    BNERV_REQUIRE(c && bucket && c->n_tensors > 0 && c->n_tensors <= BNERV_ADAN_MAX_TENSORS * 2, "bucket: bad args");
    BucketArgs a;
    a.c = *c; a.bucket = bucket; a.scale = scale; a.to_bucket = to_bucket;
    int blocks = 0;
    for (int i = 0; i < c->n_tensors; ++i) {
        BNERV_REQUIRE(c->t[i] && c->n[i] > 0 && c->off[i] >= 0, "bucket: bad tensor %d", i);
        int gx = cdiv(c->n[i], 256 * 4);
        if (gx > 1024) gx = 1024;
        a.bstart[i] = blocks;
        blocks += gx;
    }
    for (int i = c->n_tensors; i <= BNERV_ADAN_MAX_TENSORS * 2; ++i) a.bstart[i] = blocks;
    hipLaunchKernelGGL(bucket_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    BNERV_LAUNCH_CHECK("bucket");
    return BNERV_OK;
}

extern "C" int bnerv_bucket_gather(void* stream, const bnerv_bucket_chunk* c, float* bucket, float scale) {
    return bucket_launch(stream, c, bucket, scale, 1);
}
extern "C" int bnerv_bucket_scatter(void* stream, const bnerv_bucket_chunk* c, const float* bucket, float scale) {
    return bucket_launch(stream, c, const_cast<float*>(bucket), scale, 0);
}
