// ssim_body.h -- the two tile bodies of the SSIM / MS-SSIM terms: the statistics (forward) and the adjoint filter with the chain (backward).
// Included by loss.hip inside its anonymous namespace, after SsimArgs / CoarseChain / Win / pk2 / pk_fma (one translation unit).
//
// Both bodies are bound by instruction issue, so what they are built around is the number of issued instructions per 16 x 32 tile:
//   * window loads as 16-byte accesses: 11 quads per window row (44 columns from a column that is a multiple of 4) when W % 4 == 0 and
//     every plane base is 16-byte aligned -- 4 (forward) / 6 (backward) loads per thread instead of 20 / 15.  Anything else takes the scalar
//     form, which leaves the SAME numbers in LDS;
//   * strips along the filter direction: a thread owns SSIM_STRIP consecutive outputs, reads their SSIM_STRIP + 10 inputs ONCE and feeds
//     every input to the (up to four) outputs it is a tap of.  Each output still sees its taps in the order k = 0 .. 10 with the same fma,
//     so every number keeps its bits; the forward products x x, y y, x y are formed once per input instead of once per tap;
//   * epilogues on 4 adjacent pixels: 16-byte stores of the statistic gradients, 16-byte accesses of X, Y and the gradient, and on an even
//     pyramid one gather per distinct coarse cell (2 + 1 + 1 + 1) instead of one per pixel and level.
//
// LDS pitches (MI355X: 64 banks of 4 bytes; ds_read_b64 is served per 32-lane half on banks (a / 4) % 64, ds_read_b32 per half on
// (a / 4) % 32, every store on (a / 4) % 32):
//   * the loaded windows (sXY, sG01, sG2) have SSIM_LP = 44 columns: rows start 16-byte aligned, so a quad is committed with 16-byte
//     stores; they are only READ by the vertical pass, whose lanes walk consecutive columns of one row (consecutive banks at any pitch;
//     the one seam per wave where a strip ends, 42 columns, is a 2-way conflict on at most 10 lanes);
//   * the vertical pass's outputs (sV*, sA*) have SSIM_VP = 43 columns.  The horizontal pass reads them with lane = 8 * row + quad: the 8
//     quads of a row are 4 columns apart -- packed pairs: 8 banks apart, covering bank residues {0, 1} mod 8 of all 64 banks; single maps: 4
//     banks apart, residue 0 mod 4 of the 32 -- and the 4 rows of a 32-lane half must fall on the four different residues.  A packed row is
//     86 banks = 6 mod 8 (rows at 0, 6, 4, 2), a single row 43 = 3 mod 4 (rows at 0, 3, 2, 1): conflict-free for every tap offset, which no
//     EVEN pitch is (42 puts rows 0 and 2 of a half on the same banks).
//     MEASURED, and not what the map above promises: the compiler pairs the reads of two neighbouring columns into ds_read2_b64 / ds_read2_b32
//     (8-byte alignment is all an odd pitch gives it), which are served in 16-lane groups on banks (a / 4) % 32 -- two rows of 8 quads, whose
//     8-bank steps hit only 4 distinct banks: 2-way.  SQ_LDS_BANK_CONFLICT is 32 % of the LDS-active cycles of the C1 statistics launch (0 before)
//     while the LDS-active cycles themselves fell by 27 % and the launch is not LDS-bound (profiles/ssim_filter.md); an even pitch would add the
//     row conflict on top.  Left as it is.
constexpr int SSIM_STRIP = 4;                          // outputs per thread along the filter direction
constexpr int SSIM_SIN = SSIM_STRIP + HW_;             // 14 inputs per strip
constexpr int SSIM_WH = STH + HW_, SSIM_WW = STW + HW_;  // 26 x 42 window / statistic-gradient region
constexpr int SSIM_NQ = 11, SSIM_LP = 4 * SSIM_NQ;     // quads per window row; pitch of the loaded windows
constexpr int SSIM_VP = 43;                            // pitch of the vertical pass's outputs
constexpr int SSIM_VT = (STH / SSIM_STRIP) * SSIM_WW;  // 168 threads of the vertical pass
constexpr int SSIM_HT = STH * (STW / SSIM_STRIP);      // 128 threads of the horizontal pass
static_assert(STH % SSIM_STRIP == 0 && STW % SSIM_STRIP == 0 && SSIM_STRIP == 4 && SSIM_VT <= 256 && STH * STW == 512, "thread maps of ssim_body.h");
static_assert(SSIM_LP >= SSIM_WW + 2 && SSIM_VP >= SSIM_WW, "LDS pitches of ssim_body.h");

// A scheduling fence every 4 inputs of a strip.  Without it the compiler issues the LDS reads of all 14 inputs first (70 live registers in
// the forward passes: 96 - 106 VGPRs, 4 - 5 waves per SIMD); with it the bodies stay at the 7 waves per SIMD their LDS allows.
#define SSIM_STREAM_FENCE(j) do { if (((j) & 3) == 3) { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } } while (0)
// The finished sums of a strip, pinned where the stream ends.  The epilogues branch (uniformly) per pixel, and the compiler otherwise sinks each
// pixel's taps into that pixel's first block, which keeps all 14 inputs alive across the four epilogues.
#define SSIM_PIN(x) asm volatile("" : "+v"(x))

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- forward: per-tile sum of cs (LAST=false) or ssim (LAST=true) over the valid region ----
// The filter passes run on PACKED pairs of maps (v_pk_fma_f32: two fused multiply-adds per issued instruction): (x, y) live interleaved in
// LDS, so a tap is pk_fma(g, (x, y)), pk_fma(g, (x x, y y)), fma(g, x y); the second pass reads (v0, v1), (v2, v3), v4 likewise.  Every lane
// of a packed operation is the same IEEE fma in the same tap order as the scalar form: the numbers keep their bits.
constexpr int SSIM_FWD_LDS = 2 * SSIM_WH * SSIM_LP + 5 * STH * SSIM_VP;      // floats: 22912 bytes, 7 blocks per CU as before
__device__ __forceinline__ void ssim_fwd_body(const SsimArgs& a, const bool LAST, const int bx, const int by, const int bc, const int nbc) {
#pragma clang fp contract(off)                           // the SSIM algebra as written (products rounded, then added -- as the reference's tensor ops do), identical in every instantiation; the filter taps are explicit fmas
    __shared__ __attribute__((aligned(16))) float sl[SSIM_FWD_LDS];
    __shared__ float red[4];
    pk2 (*sXY)[SSIM_LP] = reinterpret_cast<pk2 (*)[SSIM_LP]>(sl);
    pk2 (*sV01)[SSIM_VP] = reinterpret_cast<pk2 (*)[SSIM_VP]>(sl + 2 * SSIM_WH * SSIM_LP);
    pk2 (*sV23)[SSIM_VP] = reinterpret_cast<pk2 (*)[SSIM_VP]>(sl + 2 * SSIM_WH * SSIM_LP + 2 * STH * SSIM_VP);
    float (*sV4)[SSIM_VP] = reinterpret_cast<float (*)[SSIM_VP]>(sl + 2 * SSIM_WH * SSIM_LP + 4 * STH * SSIM_VP);
    float* sT = sl;                                      // the tile's 512 per-pixel terms, over sXY once the vertical pass is done with it
    const int tid = threadIdx.x;
    const int oy0 = by * STH, ox0 = bx * STW;
    const size_t plane = (size_t)a.H * a.W;
    const float* X = a.X + (size_t)bc * plane;
    const float* Y = a.Y + (size_t)bc * plane;
    const bool wide = (a.W & 3) == 0 && aligned16(a.X) && aligned16(a.Y) && (a.G == nullptr || aligned16(a.G));
    if (wide) {                                          // the whole window in flight (4 16-byte loads per thread), then the LDS stores
        constexpr int NQ = SSIM_WH * SSIM_NQ, NLD = (NQ + 255) / 256;
        float4 lx[NLD], ly[NLD];
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int q = tid + u * 256;
            const int r = q / SSIM_NQ, c4 = q - r * SSIM_NQ;
            const int y = oy0 + r, x = ox0 + 4 * c4;
            lx[u] = float4{0.f, 0.f, 0.f, 0.f}; ly[u] = float4{0.f, 0.f, 0.f, 0.f};
            if (q < NQ && y < a.H && x < a.W) {          // (W % 4 == 0: a quad is inside the image or outside it)
                lx[u] = *reinterpret_cast<const float4*>(X + (size_t)y * a.W + x);
                ly[u] = *reinterpret_cast<const float4*>(Y + (size_t)y * a.W + x);
            }
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int q = tid + u * 256;
            const int r = q / SSIM_NQ, c4 = q - r * SSIM_NQ;
            if (q < NQ) {
                float4* d = reinterpret_cast<float4*>(&sXY[r][4 * c4]);
                d[0] = float4{lx[u].x, ly[u].x, lx[u].y, ly[u].y};
                d[1] = float4{lx[u].z, ly[u].z, lx[u].w, ly[u].w};
            }
        }
    } else {                                             // element by element (10 loads per thread): the same window
        constexpr int NLD = (SSIM_WH * SSIM_WW + 255) / 256;
        pk2 ld[NLD];
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * 256;
            const int r = i / SSIM_WW, c = i - r * SSIM_WW;
            const int y = oy0 + r, x = ox0 + c;
            const bool in = i < SSIM_WH * SSIM_WW && y < a.H && x < a.W;
            ld[u] = pk2{in ? X[(size_t)y * a.W + x] : 0.f, in ? Y[(size_t)y * a.W + x] : 0.f};
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * 256;
            const int r = i / SSIM_WW, c = i - r * SSIM_WW;
            if (i < SSIM_WH * SSIM_WW) sXY[r][c] = ld[u];
        }
    }
    __syncthreads();
    // vertical (along H) first, as the reference filters dim 2 then dim 3: a thread owns one column and 4 output rows
    if (tid < SSIM_VT) {
        const int s = tid / SSIM_WW, c = tid - s * SSIM_WW, r0 = s * SSIM_STRIP;
        pk2 v01[SSIM_STRIP], v23[SSIM_STRIP];
        float v4[SSIM_STRIP];
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) { v01[o] = pk2{0.f, 0.f}; v23[o] = pk2{0.f, 0.f}; v4[o] = 0.f; }
#pragma unroll
        for (int j = 0; j < SSIM_SIN; ++j) {
            const pk2 xy = sXY[r0 + j][c];
            const pk2 sq = xy * xy;
            const float p = xy.x * xy.y;
#pragma unroll
            for (int o = 0; o < SSIM_STRIP; ++o) {
                const int k = j - o;                     // input row r0 + j is tap k of output row r0 + o
                if (k >= 0 && k < WS_) {
                    const float g = a.win.g[k];
                    const pk2 gg = {g, g};
                    v01[o] = pk_fma(gg, xy, v01[o]); v23[o] = pk_fma(gg, sq, v23[o]); v4[o] = fmaf(g, p, v4[o]);
                }
            }
            SSIM_STREAM_FENCE(j);
        }
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) { sV01[r0 + o][c] = v01[o]; sV23[r0 + o][c] = v23[o]; sV4[r0 + o][c] = v4[o]; }
    }
    __syncthreads();
    const int Hv = a.H - HW_, Wv = a.W - HW_;
    // horizontal: a thread owns 4 adjacent outputs of a row, then their SSIM algebra
    if (tid < SSIM_HT) {
        const int r = tid >> 3, c0 = (tid & 7) * SSIM_STRIP;
        pk2 m[SSIM_STRIP], e[SSIM_STRIP];
        float exy[SSIM_STRIP];
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) { m[o] = pk2{0.f, 0.f}; e[o] = pk2{0.f, 0.f}; exy[o] = 0.f; }
#pragma unroll
        for (int j = 0; j < SSIM_SIN; ++j) {
            const pk2 i01 = sV01[r][c0 + j], i23 = sV23[r][c0 + j];
            const float i4 = sV4[r][c0 + j];
#pragma unroll
            for (int o = 0; o < SSIM_STRIP; ++o) {
                const int k = j - o;
                if (k >= 0 && k < WS_) {
                    const float g = a.win.g[k];
                    const pk2 gg = {g, g};
                    m[o] = pk_fma(gg, i01, m[o]); e[o] = pk_fma(gg, i23, e[o]); exy[o] = fmaf(g, i4, exy[o]);
                }
            }
            SSIM_STREAM_FENCE(j);
        }
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) { SSIM_PIN(m[o]); SSIM_PIN(e[o]); SSIM_PIN(exy[o]); }
        const bool rowv = oy0 + r < Hv;
        float dm[SSIM_STRIP], dxx[SSIM_STRIP], dxy[SSIM_STRIP], term[SSIM_STRIP];
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) {
            dm[o] = 0.f; dxx[o] = 0.f; dxy[o] = 0.f;
            {   // (unconditionally -- a pixel outside the valid region is neither summed nor stored: under a per-pixel branch the compiler
                // sinks that pixel's 33 taps into it and keeps all 14 inputs, 70 registers, alive across the four)
                const float m1 = m[o].x, m2 = m[o].y, exx = e[o].x, eyy = e[o].y;
                const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
                const float s1 = exx - m11, s2 = eyy - m22, s12 = exy[o] - m12;
                const float B2 = s1 + s2 + a.C2;
                const float cs = (2.f * s12 + a.C2) / B2;
                float lum = 1.f;
                if (LAST) { lum = (2.f * m12 + a.C1) / (m11 + m22 + a.C1); term[o] = lum * cs; }
                else term[o] = cs;
                if (a.G) {
                    // the statistic gradients take 1 / B2 (and 1 / B1) through v_rcp_f32 (1 ulp) -- three IEEE divisions were a quarter of this
                    // pass's instructions; the VALUE path (cs, lum) keeps the exact quotient
                    const float dxy0 = 2.f * __builtin_amdgcn_rcpf(B2);
                    dm[o] = dxy0 * (m1 * cs - m2); dxx[o] = -0.5f * cs * dxy0; dxy[o] = dxy0;
                    if (LAST) {
                        const float B1 = m11 + m22 + a.C1;
                        dm[o] = (2.f * __builtin_amdgcn_rcpf(B1)) * (m2 - m1 * lum) * cs + lum * dm[o];
                        dxx[o] *= lum; dxy[o] *= lum;
                    }
                }
            }
        }
        *reinterpret_cast<float4*>(sT + r * STW + c0) = float4{term[0], term[1], term[2], term[3]};
        if (a.G && rowv) {
            const size_t o0 = (size_t)bc * plane + (size_t)(oy0 + r) * a.W + (ox0 + c0);
            const size_t mstride = (size_t)nbc * plane;
            if (wide && ox0 + c0 + SSIM_STRIP - 1 < Wv) {
                *reinterpret_cast<float4*>(a.G + o0) = float4{dm[0], dm[1], dm[2], dm[3]};
                *reinterpret_cast<float4*>(a.G + mstride + o0) = float4{dxx[0], dxx[1], dxx[2], dxx[3]};
                *reinterpret_cast<float4*>(a.G + 2 * mstride + o0) = float4{dxy[0], dxy[1], dxy[2], dxy[3]};
            } else {
#pragma unroll
                for (int o = 0; o < SSIM_STRIP; ++o)
                    if (ox0 + c0 + o < Wv) { a.G[o0 + o] = dm[o]; a.G[mstride + o0 + o] = dxx[o]; a.G[2 * mstride + o0 + o] = dxy[o]; }
            }
        }
    }
    __syncthreads();
    // the tile's sum with the ownership it always had -- thread t adds outputs t and t + 256, invalid ones skipped -- so the partial keeps its bits
    float acc = 0.f;
    for (int i = tid; i < STH * STW; i += 256) {
        const int r = i / STW, c = i - r * STW;
        if (oy0 + r < Hv && ox0 + c < Wv) acc += sT[i];
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) a.partial[(size_t)bc * (a.tiles_x * a.tiles_y) + by * a.tiles_x + bx] = red[0] + red[1] + red[2] + red[3];
}

// ---- backward from the stored statistic gradients: adjoint of the separable "valid" filter over the 3 maps, then
//      dX = coef * (A0 + 2 x A1 + y A2) [+ 0.25 * d(coarser level)] [+ L1/L2 terms at level 0].  ~6x less arithmetic than
//      recomputing the statistics on a 36x52 window per tile.
// The region is held from column px0 - 12 (a multiple of 4: 11 quads per row); its columns 0 and 1 are loaded by the wide form only and
// read by nobody.  The adjoint taps run HW_ - k, so a strip walks its inputs from the last to the first: tap order k = 0 .. 10 per output.
constexpr int SSIM_BWD_LDS = 3 * SSIM_WH * SSIM_LP + 3 * STH * SSIM_VP;      // floats: 21984 bytes, 7 blocks per CU as before
// `lds`: SSIM_BWD_LDS floats of the caller's LDS (16-byte aligned) -- a pointer so that a kernel whose blocks run EITHER this body or an FFT
// body (loss_coarse_kernel) can give both the same allocation: two static arrays would add up and halve the blocks per CU
template <bool LEVEL0>
__device__ __forceinline__ void ssim_bwd_body(const SsimArgs& a, const CoarseChain* cc, float* lds, const int bx, const int by, const int bc, const int nbc) {
    pk2 (*sG01)[SSIM_LP] = reinterpret_cast<pk2 (*)[SSIM_LP]>(lds);                          // packed pairs of maps, as in the forward pass
    pk2 (*sA01)[SSIM_VP] = reinterpret_cast<pk2 (*)[SSIM_VP]>(lds + 2 * SSIM_WH * SSIM_LP);
    float (*sG2)[SSIM_LP] = reinterpret_cast<float (*)[SSIM_LP]>(lds + 2 * SSIM_WH * SSIM_LP + 2 * STH * SSIM_VP);
    float (*sA2)[SSIM_VP] = reinterpret_cast<float (*)[SSIM_VP]>(lds + 3 * SSIM_WH * SSIM_LP + 2 * STH * SSIM_VP);
    const int tid = threadIdx.x;
    const int py0 = by * STH, px0 = bx * STW;
    const int wy0 = py0 - HW_, wx0 = px0 - HW_;
    const int Hv = a.H - HW_, Wv = a.W - HW_;
    const size_t plane = (size_t)a.H * a.W, mstride = (size_t)nbc * plane;
    const float* Gp = a.G + (size_t)bc * plane;
    const bool wide = (a.W & 3) == 0 && aligned16(a.X) && aligned16(a.Y) && aligned16(a.G) && aligned16(a.dX);
    if (wide) {                                          // the whole region of the three maps in flight (6 16-byte loads per thread), then the LDS stores
        constexpr int NQ = SSIM_WH * SSIM_NQ, NLD = (NQ + 255) / 256;
        float4 l0[NLD], l1[NLD], l2[NLD];
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int q = tid + u * 256;
            const int r = q / SSIM_NQ, c4 = q - r * SSIM_NQ;
            const int oy = wy0 + r, ox = px0 - 12 + 4 * c4;
            l0[u] = float4{0.f, 0.f, 0.f, 0.f}; l1[u] = l0[u]; l2[u] = l0[u];
            if (q < NQ && oy >= 0 && oy < Hv && ox >= 0 && ox < Wv) {         // (ox + 3 < W: the quad is memory of this row; what lies past Wv is dropped below)
                const size_t o = (size_t)oy * a.W + ox;
                l0[u] = *reinterpret_cast<const float4*>(Gp + o);
                l1[u] = *reinterpret_cast<const float4*>(Gp + mstride + o);
                l2[u] = *reinterpret_cast<const float4*>(Gp + 2 * mstride + o);
                if (ox + 1 >= Wv) { l0[u].y = 0.f; l1[u].y = 0.f; l2[u].y = 0.f; }
                if (ox + 2 >= Wv) { l0[u].z = 0.f; l1[u].z = 0.f; l2[u].z = 0.f; }
                if (ox + 3 >= Wv) { l0[u].w = 0.f; l1[u].w = 0.f; l2[u].w = 0.f; }
            }
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int q = tid + u * 256;
            const int r = q / SSIM_NQ, c4 = q - r * SSIM_NQ;
            if (q < NQ) {
                float4* d = reinterpret_cast<float4*>(&sG01[r][4 * c4]);
                d[0] = float4{l0[u].x, l1[u].x, l0[u].y, l1[u].y};
                d[1] = float4{l0[u].z, l1[u].z, l0[u].w, l1[u].w};
                *reinterpret_cast<float4*>(&sG2[r][4 * c4]) = l2[u];
            }
        }
    } else {                                             // element by element (15 loads per thread): the same region, from column px0 - 10
        constexpr int NLD = (SSIM_WH * SSIM_WW + 255) / 256;
        float l0[NLD], l1[NLD], l2[NLD];
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * 256;
            const int r = i / SSIM_WW, c = i - r * SSIM_WW;
            const int oy = wy0 + r, ox = wx0 + c;
            l0[u] = 0.f; l1[u] = 0.f; l2[u] = 0.f;
            if (i < SSIM_WH * SSIM_WW && oy >= 0 && oy < Hv && ox >= 0 && ox < Wv) {
                const size_t o = (size_t)oy * a.W + ox;
                l0[u] = Gp[o]; l1[u] = Gp[mstride + o]; l2[u] = Gp[2 * mstride + o];
            }
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * 256;
            const int r = i / SSIM_WW, c = i - r * SSIM_WW;
            if (i < SSIM_WH * SSIM_WW) { sG01[r][c + 2] = pk2{l0[u], l1[u]}; sG2[r][c + 2] = l2[u]; }
        }
    }
    __syncthreads();
    if (tid < SSIM_VT) {                                 // vertical: one column, 4 output rows
        const int s = tid / SSIM_WW, c = tid - s * SSIM_WW, r0 = s * SSIM_STRIP;
        pk2 a01[SSIM_STRIP];
        float a2[SSIM_STRIP];
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) { a01[o] = pk2{0.f, 0.f}; a2[o] = 0.f; }
#pragma unroll
        for (int j = SSIM_SIN - 1; j >= 0; --j) {
            const pk2 g01 = sG01[r0 + j][c + 2];
            const float g2 = sG2[r0 + j][c + 2];
#pragma unroll
            for (int o = 0; o < SSIM_STRIP; ++o) {
                const int k = HW_ - (j - o);             // input row r0 + j is tap k of output row r0 + o (row + HW_ - k)
                if (k >= 0 && k < WS_) {
                    const float g = a.win.g[k];
                    a01[o] = pk_fma(pk2{g, g}, g01, a01[o]);
                    a2[o] = fmaf(g, g2, a2[o]);
                }
            }
            SSIM_STREAM_FENCE(j);
        }
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) { sA01[r0 + o][c] = a01[o]; sA2[r0 + o][c] = a2[o]; }
    }
    __syncthreads();
    if (tid >= SSIM_HT) return;                          // (no barrier below)
    const int r = tid >> 3, c0 = (tid & 7) * SSIM_STRIP;
    const int y = py0 + r, x0 = px0 + c0;
    if (y >= a.H || x0 >= a.W) return;
    pk2 a01[SSIM_STRIP];
    float a2[SSIM_STRIP];
#pragma unroll
    for (int o = 0; o < SSIM_STRIP; ++o) { a01[o] = pk2{0.f, 0.f}; a2[o] = 0.f; }
#pragma unroll
    for (int j = SSIM_SIN - 1; j >= 0; --j) {            // horizontal: 4 adjacent outputs of a row
        const pk2 i01 = sA01[r][c0 + j];
        const float i2 = sA2[r][c0 + j];
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) {
            const int k = HW_ - (j - o);
            if (k >= 0 && k < WS_) {
                const float g = a.win.g[k];
                a01[o] = pk_fma(pk2{g, g}, i01, a01[o]);
                a2[o] = fmaf(g, i2, a2[o]);
            }
        }
        SSIM_STREAM_FENCE(j);
    }
#pragma unroll
    for (int o = 0; o < SSIM_STRIP; ++o) { SSIM_PIN(a01[o]); SSIM_PIN(a2[o]); }
    const float coef = a.coef ? a.coef[bc] : a.coef_k;
    const float* Xr = a.X + (size_t)bc * plane + (size_t)y * a.W + x0;
    const float* Yr = a.Y + (size_t)bc * plane + (size_t)y * a.W + x0;
    float* dst = a.dX + ((size_t)bc * a.H + y) * a.W + x0;
    const bool accum = LEVEL0 && a.acc;
    float xv[SSIM_STRIP], yv[SSIM_STRIP], old[SSIM_STRIP], res[SSIM_STRIP];
    if (wide) {                                          // (W % 4 == 0: all four pixels are inside the image)
        const float4 xq = *reinterpret_cast<const float4*>(Xr), yq = *reinterpret_cast<const float4*>(Yr);
        xv[0] = xq.x; xv[1] = xq.y; xv[2] = xq.z; xv[3] = xq.w;
        yv[0] = yq.x; yv[1] = yq.y; yv[2] = yq.z; yv[3] = yq.w;
        old[0] = 0.f; old[1] = 0.f; old[2] = 0.f; old[3] = 0.f;
        if (accum) { const float4 dq = *reinterpret_cast<const float4*>(dst); old[0] = dq.x; old[1] = dq.y; old[2] = dq.z; old[3] = dq.w; }
    } else {
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) {
            const bool in = x0 + o < a.W;
            xv[o] = in ? Xr[o] : 0.f; yv[o] = in ? Yr[o] : 0.f; old[o] = (in && accum) ? dst[o] : 0.f;
        }
    }
    // even pyramid: the coarser levels stored only their OWN terms; d_k = own_k + 0.25 d_{k+1} is evaluated here, innermost first,
    // exactly as the level-by-level launches did (0.25 * is exact), so the gradient keeps its bits.  Where no level is padded the four
    // pixels (x0 is a multiple of 4) lie in two cells of level 1 and ONE cell of every coarser level: 5 gathers instead of 16
    const bool chain = LEVEL0 && cc != nullptr && cc->n > 0;
    bool chain_even = chain;
    float own1[2] = {0.f, 0.f}, ownk[LV];
#pragma unroll
    for (int k = 0; k < LV; ++k) ownk[k] = 0.f;
    if (chain) {
#pragma unroll
        for (int k = 0; k < LV - 1; ++k) if (k < cc->n && (cc->ph[k] | cc->pw[k])) chain_even = false;
        if (chain_even) {                                // (every level above the last is even: x0 + 3 < W, and cell (y >> k, x >> k) exists)
#pragma unroll
            for (int k = 1; k < LV; ++k) {
                if (k > cc->n) continue;
                const float* p = cc->own[k] + ((size_t)bc * cc->H[k] + (y >> k)) * cc->W[k] + (x0 >> k);
                if (k == 1) { own1[0] = p[0]; own1[1] = p[1]; }
                else ownk[k] = p[0];
            }
        }
    }
#pragma unroll
    for (int o = 0; o < SSIM_STRIP; ++o) {
        const int x = x0 + o;
        const float a0 = a01[o].x, a1 = a01[o].y;
        float d = coef * (a0 + 2.f * xv[o] * a1 + yv[o] * a2[o]);
        if (a.dcoarse && x < a.W) d += 0.25f * a.dcoarse[((size_t)bc * a.Hc + (y + a.ph) / 2) * a.Wc + (x + a.pw) / 2];
        if (chain) {
            float dc = 0.f;
            if (chain_even) {
#pragma unroll
                for (int k = LV - 1; k >= 1; --k) {
                    if (k > cc->n) continue;
                    const float ov = k == 1 ? own1[o >> 1] : ownk[k];
                    dc = (k == cc->n) ? ov : ov + 0.25f * dc;
                }
            } else if (x < a.W) {                        // a padded level somewhere: pixel (y, x) of level k lies in cell ((y + ph) / 2, (x + pw) / 2)
                int yk[LV], xk[LV];
                yk[0] = y; xk[0] = x;
#pragma unroll
                for (int k = 1; k < LV; ++k) { yk[k] = (yk[k - 1] + cc->ph[k - 1]) >> 1; xk[k] = (xk[k - 1] + cc->pw[k - 1]) >> 1; }
#pragma unroll
                for (int k = LV - 1; k >= 1; --k) {
                    if (k > cc->n) continue;
                    const float ov = cc->own[k][((size_t)bc * cc->H[k] + yk[k]) * cc->W[k] + xk[k]];
                    dc = (k == cc->n) ? ov : ov + 0.25f * dc;
                }
            }
            d += 0.25f * dc;
        }
        if (LEVEL0) {
            const float df = xv[o] - yv[o];
            const float sg = (df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f);
            d += a.k_l1 * sg + a.k_l2 * df;
        }
        res[o] = accum ? d + old[o] : d;
    }
    if (wide) *reinterpret_cast<float4*>(dst) = float4{res[0], res[1], res[2], res[3]};
    else {
#pragma unroll
        for (int o = 0; o < SSIM_STRIP; ++o) if (x0 + o < a.W) dst[o] = res[o];
    }
}
