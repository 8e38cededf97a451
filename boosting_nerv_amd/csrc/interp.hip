// interp.hip -- frame embeddings of an interpolation file: the rows a file does not store, derived from the rows it stores.
//
// bnerv_embed_expand: out [N, P] from src [S, P] under a per-row plan (ia, ib, w) (hnerv_utils.interp_plan).  A stored
// frame copies its row; a derived frame blends the rows of its nearest stored neighbours in time.  The reference forms the embedding of a
// held-out frame as 0.5 * (encoder(pre) + encoder(post)) (model_hnerv.py:82, :237); here L and R are rows of ONE table -- the encoder's
// outputs in evaluation, the de-quantised embeddings in a decoder -- and the same launch serves both, which is why a decoded held-out frame
// equals the evaluated one bit for bit.  The arithmetic is fixed so that a numpy fp32 restatement gives the same bits
// (hnerv_utils.embed_expand_reference):
//   ia == ib   out = L
//   w == 0.5f  out = 0.5f * (L + R)                                  (the reference's expression)
//   otherwise  out = (1.0f - w) * L + w * R, every product and the sum rounded on its own: no fused contraction (expand1 below)
// Streaming: grid (ceil(P / EX_TILE), N), a block reads its row's plan entry once (uniform over the block), no LDS, no atomics.
#include "common.h"

namespace {
constexpr int EX_TILE = 1024;           // elements of one row per block (256 threads x one float4)

struct ExpandEntry { int ia, ib; float w; };      // bnerv_interp_entry

// One element.  Plain operators under `fp contract(off)`: the pragma is what keeps the two products and the sum apart (the __fmul_rn /
// __fadd_rn of the HIP headers are inline `x * y` / `x + y` compiled with contraction allowed; codec.hip has the same note).
__device__ __forceinline__ float expand1(const float l, const float r, const float w, const float u, const int mode) {
#pragma clang fp contract(off)
    if (mode == 0) return l;
    if (mode == 1) return 0.5f * (l + r);
    const float a = u * l, b = w * r;
    return a + b;
}

__global__ __launch_bounds__(256) void embed_expand_kernel(const float* __restrict__ src, const ExpandEntry* __restrict__ plan, float* __restrict__ out,
                                                           const int S, const int P, const int vec) {
    const int t = blockIdx.y;
    const ExpandEntry e = plan[t];
    if (e.ia < 0 || e.ia >= S || e.ib < 0 || e.ib >= S) return;      // (the host validates the plan; a bad entry must not become a wild read)
    const float* __restrict__ L = src + (size_t)e.ia * P;
    const float* __restrict__ R = src + (size_t)e.ib * P;
    float* __restrict__ o = out + (size_t)t * P;
    const int mode = e.ia == e.ib ? 0 : (e.w == 0.5f ? 1 : 2);
    const float w = e.w, u = 1.0f - e.w;
    if (vec) {
        const int i = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
        if (i >= P) return;
        const f32x4 l = *reinterpret_cast<const f32x4*>(L + i);
        f32x4 v = l;
        if (mode) {
            const f32x4 r = *reinterpret_cast<const f32x4*>(R + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = expand1(l[k], r[k], w, u, mode);
        }
        *reinterpret_cast<f32x4*>(o + i) = v;
    } else {
        const int e0 = (int)blockIdx.x * EX_TILE;
        for (int i = e0 + (int)threadIdx.x; i < min(P, e0 + EX_TILE); i += 256) {
            const float l = L[i];
            o[i] = expand1(l, mode ? R[i] : l, w, u, mode);
        }
    }
}
}  // namespace

extern "C" int bnerv_embed_expand(void* stream, const float* src, const bnerv_interp_entry* plan_dev, float* out, int S, int N, int P) {
    static_assert(sizeof(ExpandEntry) == sizeof(bnerv_interp_entry) && sizeof(ExpandEntry) == 12, "plan entry layout");
    BNERV_REQUIRE(src && plan_dev && out, "embed_expand: null args");
    BNERV_REQUIRE(S > 0 && N > 0 && P > 0 && N <= 65535, "embed_expand: S=%d N=%d P=%d (1 <= N <= 65535 rows)", S, N, P);
    BNERV_REQUIRE(P <= (1 << 30), "embed_expand: P=%d: a row of more than 2^30 elements", P);      // (the element index of a row is an int)
    BNERV_REQUIRE(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(plan_dev)) & 3) == 0,
                  "embed_expand: src, out and the plan must be 4-byte aligned");
    // float4 form: every row of both tables starts on a 16-byte boundary (P % 4 == 0 and aligned bases); otherwise the scalar loop
    const int vec = (P % 4 == 0) && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    hipLaunchKernelGGL(embed_expand_kernel, dim3(cdiv(P, EX_TILE), N), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src,
                       reinterpret_cast<const ExpandEntry*>(plan_dev), out, S, P, vec);
    BNERV_LAUNCH_CHECK("embed_expand");
    return BNERV_OK;
}
