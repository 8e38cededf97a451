// fft_body.h -- the mixed-radix LDS FFT of the spectral loss term: plans and their device tables, butterflies, stages, and the row /
// column transform bodies.  Included by loss.hip inside its unnamed namespace, after common.h; the __global__ wrappers stay there.
#pragma once
// =====================================================================================================================
// mixed-radix FFT in LDS
// =====================================================================================================================
constexpr int MAXRAD = 16;
struct FftPlan { int N, nrad; int rad[MAXRAD]; const float2* tw; const int* pos; };   // tw[k] = exp(-2*pi*i*k/N)
// pos[f] = buffer position that holds frequency f after the in-place DIF forward (mixed-radix digit reversal)

std::mutex g_tw_mutex;
std::map<int, float2*> g_tw;

static const float2* get_twiddles(int N) {
    std::lock_guard<std::mutex> lk(g_tw_mutex);
    auto it = g_tw.find(N);
    if (it != g_tw.end()) return it->second;
    float2* h = (float2*)malloc(sizeof(float2) * N);
    for (int k = 0; k < N; ++k) {
        const double ang = -2.0 * M_PI * (double)k / (double)N;
        h[k].x = (float)cos(ang);
        h[k].y = (float)sin(ang);
    }
    float2* d = nullptr;
    if (hipMalloc(&d, sizeof(float2) * N) != hipSuccess) { free(h); return nullptr; }
    if (hipMemcpy(d, h, sizeof(float2) * N, hipMemcpyHostToDevice) != hipSuccess) { free(h); (void)hipFree(d); return nullptr; }
    free(h);
    g_tw[N] = d;
    return d;
}

std::map<int, int*> g_pos;
// forward DIF with radices [R, rest] on size Ns: frequency k = q + R*k' ends up in sub-block q (size M = Ns/R) at the position
// the rest of the plan gives k'  =>  pos(k) = (k % R) * M + pos_rest(k / R)
static const int* get_positions(const FftPlan& pl) {
    std::lock_guard<std::mutex> lk(g_tw_mutex);
    auto it = g_pos.find(pl.N);
    if (it != g_pos.end()) return it->second;
    std::vector<int> h(pl.N);
    for (int f = 0; f < pl.N; ++f) {
        int k = f, Ns = pl.N, p = 0;
        for (int st = 0; st < pl.nrad; ++st) {
            const int R = pl.rad[st], M = Ns / R;
            p += (k % R) * M;
            k /= R;
            Ns = M;
        }
        h[f] = p;
    }
    int* d = nullptr;
    if (hipMalloc(&d, sizeof(int) * pl.N) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), sizeof(int) * pl.N, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    g_pos[pl.N] = d;
    return d;
}

// maxr: the largest prime the caller's kernels hold register arrays for (butterfly_generic<.., MAXR>)
static bool make_plan(int N, FftPlan* p, int maxr = BNERV_FFT_MAX_RADIX) {
    p->N = N; p->nrad = 0;
    int n = N;
    auto push = [&](int r) { if (p->nrad < MAXRAD) p->rad[p->nrad++] = r; };
    while (n % 4 == 0) { push(4); n /= 4; }
    while (n % 2 == 0) { push(2); n /= 2; }
    while (n % 3 == 0) { push(3); n /= 3; }
    while (n % 5 == 0) { push(5); n /= 5; }
    for (int r = 7; r <= maxr && n > 1; r += 2)
        while (n % r == 0) { push(r); n /= r; }
    if (n != 1 || p->nrad >= MAXRAD) return false;
    if (N == 1) { p->nrad = 0; }
    p->tw = get_twiddles(N);
    p->pos = get_positions(*p);
    return p->tw != nullptr && p->pos != nullptr;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return float2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) { return float2{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }   // a * conj(b)

// One butterfly of radix R at sub-transform size Ns (M = Ns/R) on the in-place buffer.
//  forward (DIF):  y_q = w_Ns^{jq} * sum_m x_m w_R^{mq}             x_m = buf[base+m*M], y_q -> buf[base+q*M]
//  adjoint      :  x_m = sum_q conj(w_R^{mq}) conj(w_Ns^{jq}) y_q   (exact conjugate transpose of the forward stage)
// Radix 2/3/4/5 cores use the closed forms (adds, +-i swaps, two or four real constants): the kernels are instruction-bound, and
// a table-driven core costs ~300 instructions per radix-4 butterfly against ~50 here.  SGN = -1 forward, +1 adjoint: the
// adjoint core is the forward core with i -> -i, i.e. the exact conjugate transpose with the same constants.
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return float2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return float2{a.x - b.x, a.y - b.y}; }
template <int SGN> __device__ __forceinline__ float2 mul_i(float2 a) { return SGN > 0 ? float2{-a.y, a.x} : float2{a.y, -a.x}; }   // (SGN*i) * a

template <int R, int SGN>
__device__ __forceinline__ void dft_core(const float2 (&v)[R], float2 (&o)[R]) {
    if constexpr (R == 2) {
        o[0] = cadd(v[0], v[1]);
        o[1] = csub(v[0], v[1]);
    } else if constexpr (R == 4) {
        const float2 a = cadd(v[0], v[2]), b = csub(v[0], v[2]), c = cadd(v[1], v[3]), dd = mul_i<SGN>(csub(v[1], v[3]));
        o[0] = cadd(a, c); o[2] = csub(a, c); o[1] = cadd(b, dd); o[3] = csub(b, dd);
    } else if constexpr (R == 3) {
        constexpr float C = 0.86602540378443864676f;                       // sin(2 pi / 3)
        const float2 sum = cadd(v[1], v[2]), t = mul_i<SGN>(csub(v[1], v[2]));
        const float2 h = float2{v[0].x - 0.5f * sum.x, v[0].y - 0.5f * sum.y};
        o[0] = cadd(v[0], sum);
        o[1] = float2{h.x + C * t.x, h.y + C * t.y};
        o[2] = float2{h.x - C * t.x, h.y - C * t.y};
    } else {                                                               // R == 5
        constexpr float C1 = 0.30901699437494742410f, C2 = -0.80901699437494742410f;   // cos(2 pi / 5), cos(4 pi / 5)
        constexpr float S1 = 0.95105651629515357212f, S2 = 0.58778525229247312917f;    // sin(2 pi / 5), sin(4 pi / 5)
        const float2 s1 = cadd(v[1], v[4]), s2 = cadd(v[2], v[3]), d1 = csub(v[1], v[4]), d2 = csub(v[2], v[3]);
        const float2 a1 = float2{v[0].x + C1 * s1.x + C2 * s2.x, v[0].y + C1 * s1.y + C2 * s2.y};
        const float2 a2 = float2{v[0].x + C2 * s1.x + C1 * s2.x, v[0].y + C2 * s1.y + C1 * s2.y};
        const float2 b1 = mul_i<SGN>(float2{S1 * d1.x + S2 * d2.x, S1 * d1.y + S2 * d2.y});
        const float2 b2 = mul_i<SGN>(float2{S2 * d1.x - S1 * d2.x, S2 * d1.y - S1 * d2.y});
        o[0] = float2{v[0].x + s1.x + s2.x, v[0].y + s1.y + s2.y};
        o[1] = cadd(a1, b1); o[4] = csub(a1, b1); o[2] = cadd(a2, b2); o[3] = csub(a2, b2);
    }
}

template <int R, bool ADJ>
__device__ __forceinline__ void butterfly(float2* buf, int base, int M, int j, int tstride /* N/Ns */, const FftPlan& pl, const float2* tw) {
    float2 v[R], o[R];
    (void)pl;
#pragma unroll
    for (int m = 0; m < R; ++m) v[m] = buf[base + __mul24(m, M)];
    const int t1 = __mul24(tstride, j);                   // j < Ns/R: t1 * q < N for q < R, no wrap
    if (ADJ) {
#pragma unroll
        for (int q = 1; q < R; ++q) v[q] = cmulc(v[q], tw[t1 * q]);
        dft_core<R, +1>(v, o);
    } else {
        dft_core<R, -1>(v, o);
#pragma unroll
        for (int q = 1; q < R; ++q) o[q] = cmul(o[q], tw[t1 * q]);
    }
#pragma unroll
    for (int q = 0; q < R; ++q) buf[base + __mul24(q, M)] = o[q];
}

// generic radix (primes 7..MAXR: BNERV_FFT_MAX_RADIX, or SSIM_FFT_MAX_RADIX in the single-scale SSIM path's own instantiations): O(R^2) with the table, operands staged in registers one output at a time
template <bool ADJ, int MAXR>
__device__ void butterfly_generic(float2* buf, int base, int M, int j, int tstride, int R, const FftPlan& pl, const float2* tw) {
    float2 v[MAXR], o[MAXR];
    const int rstep = pl.N / R;
    for (int m = 0; m < R; ++m) {
        v[m] = buf[base + m * M];
        if (ADJ && m) v[m] = cmulc(v[m], tw[tstride * j * m]);
    }
    for (int q = 0; q < R; ++q) {
        float2 s = v[0];
        for (int m = 1; m < R; ++m) {
            const float2 w = tw[rstep * ((m * q) % R)];
            const float2 t = ADJ ? cmulc(v[m], w) : cmul(v[m], w);
            s.x += t.x; s.y += t.y;
        }
        if (!ADJ && q) s = cmul(s, tw[tstride * j * q]);
        o[q] = s;
    }
    for (int q = 0; q < R; ++q) buf[base + q * M] = o[q];
}

// all butterflies of one stage, radix R known at compile time.  A thread's butterflies (2-3 per stage at 720 / 1280 points) are
// independent: the loop is unrolled by UNR so that their LDS reads are in flight together instead of one round trip per butterfly.
template <int R, bool ADJ>
__device__ __forceinline__ void fft_stage_r(float2* buf, int nlines, int lstride, int Ns, const FftPlan& pl, const float2* tw) {
    const int N = pl.N, M = Ns / R, per_line = N / R, tstride = N / Ns;
    // index split by reciprocal multiplication (operands < 2^20, quotients < 2^11: the +0.5 margin dwarfs the rounding error) and
    // 24-bit multiplies: a runtime integer division costs ~40 instructions and a 32-bit multiply issues at quarter rate, and this
    // loop is instruction-latency bound (a few butterflies per thread per stage)
    const float inv_pl = 1.0f / (float)per_line, inv_M = 1.0f / (float)M;
    const int total = nlines * per_line;
    constexpr int UNR = ADJ ? 2 : 3;                       // (measured: the forward row pass 26 us at 3 / 35 at 2, the adjoint row pass 21 at 3 / 18 at 2; columns indifferent)
    for (int bf0 = threadIdx.x; bf0 < total; bf0 += UNR * blockDim.x) {
        float2 v[UNR][R], o[UNR][R];
        int base[UNR], t1[UNR];
        bool on[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int bf = bf0 + u * blockDim.x;
            on[u] = bf < total;
            const int bfc = on[u] ? bf : 0;
            const int line = (int)(((float)bfc + 0.5f) * inv_pl), rem = bfc - __mul24(line, per_line);
            const int blk = (int)(((float)rem + 0.5f) * inv_M), j = rem - __mul24(blk, M);
            base[u] = __mul24(line, lstride) + __mul24(blk, Ns) + j;
            t1[u] = __mul24(tstride, j);                   // j < Ns/R: t1 * q < N for q < R, no wrap
#pragma unroll
            for (int m = 0; m < R; ++m) v[u][m] = buf[base[u] + __mul24(m, M)];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (ADJ) {
#pragma unroll
                for (int q = 1; q < R; ++q) v[u][q] = cmulc(v[u][q], tw[t1[u] * q]);
                dft_core<R, +1>(v[u], o[u]);
            } else {
                dft_core<R, -1>(v[u], o[u]);
#pragma unroll
                for (int q = 1; q < R; ++q) o[u][q] = cmul(o[u][q], tw[t1[u] * q]);
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (on[u]) {
#pragma unroll
                for (int q = 0; q < R; ++q) buf[base[u] + __mul24(q, M)] = o[u][q];
            }
        }
    }
    __syncthreads();
}

template <bool ADJ, int MAXR>
__device__ void fft_stage(float2* buf, int nlines, int lstride, int Ns, int R, const FftPlan& pl, const float2* tw) {
    switch (R) {
        case 2: fft_stage_r<2, ADJ>(buf, nlines, lstride, Ns, pl, tw); return;
        case 3: fft_stage_r<3, ADJ>(buf, nlines, lstride, Ns, pl, tw); return;
        case 4: fft_stage_r<4, ADJ>(buf, nlines, lstride, Ns, pl, tw); return;
        case 5: fft_stage_r<5, ADJ>(buf, nlines, lstride, Ns, pl, tw); return;
        default: break;
    }
    const int N = pl.N, M = Ns / R, per_line = N / R, tstride = N / Ns;
    const float inv_pl = 1.0f / (float)per_line, inv_M = 1.0f / (float)M;
    for (int bf = threadIdx.x; bf < nlines * per_line; bf += blockDim.x) {
        const int line = (int)(((float)bf + 0.5f) * inv_pl), rem = bf - __mul24(line, per_line);
        const int blk = (int)(((float)rem + 0.5f) * inv_M), j = rem - __mul24(blk, M);
        const int base = __mul24(line, lstride) + __mul24(blk, Ns) + j;
        butterfly_generic<ADJ, MAXR>(buf, base, M, j, tstride, R, pl, tw);
    }
    __syncthreads();
}

// `tw`: the plan's twiddle table (and, for the row kernels, the frequency -> buffer position table) copied to LDS.  The copy is split
// into an issue half (global loads into registers, up to TAB_U per thread) and a commit half (LDS stores), so that a kernel can put its
// own input loads between the two: ONE memory round trip for tables and data instead of one per loop iteration (these blocks are a
// single latency chain each -- there is about one transform line per SIMD on the chip -- so every round trip shows in the launch).
constexpr int TAB_U = 8;
struct TabRegs { float2 t[TAB_U]; int p[TAB_U]; };
template <bool POS>
__device__ __forceinline__ void tables_issue(TabRegs& r, const FftPlan& pl) {
#pragma unroll
    for (int u = 0; u < TAB_U; ++u) {
        const int i = threadIdx.x + u * blockDim.x;
        r.t[u] = i < pl.N ? pl.tw[i] : float2{0.f, 0.f};
        if (POS) r.p[u] = i < pl.N ? pl.pos[i] : 0;
    }
}
template <bool POS>
__device__ __forceinline__ void tables_commit(const TabRegs& r, float2* tw, int* lpos, const FftPlan& pl) {
#pragma unroll
    for (int u = 0; u < TAB_U; ++u) {
        const int i = threadIdx.x + u * blockDim.x;
        if (i < pl.N) { tw[i] = r.t[u]; if (POS) lpos[i] = r.p[u]; }
    }
    for (int i = threadIdx.x + TAB_U * blockDim.x; i < pl.N; i += blockDim.x) { tw[i] = pl.tw[i]; if (POS) lpos[i] = pl.pos[i]; }   // (N > 2048)
}
template <int MAXR = BNERV_FFT_MAX_RADIX>
__device__ void fft_forward(float2* buf, int nlines, int lstride, const FftPlan& pl, const float2* tw) {
    int Ns = pl.N;
    for (int s = 0; s < pl.nrad; ++s) { fft_stage<false, MAXR>(buf, nlines, lstride, Ns, pl.rad[s], pl, tw); Ns /= pl.rad[s]; }
}
template <int MAXR = BNERV_FFT_MAX_RADIX>
__device__ void fft_adjoint(float2* buf, int nlines, int lstride, const FftPlan& pl, const float2* tw) {
    int Ns = 1;
    for (int s = pl.nrad - 1; s >= 0; --s) { Ns *= pl.rad[s]; fft_stage<true, MAXR>(buf, nlines, lstride, Ns, pl.rad[s], pl, tw); }
}

// The row transforms work on PAIRS of real rows: z = a + i b is ONE complex transform, and the two real rows' spectra are its
// Hermitian and anti-Hermitian parts, A[f] = (Z[f] + conj Z[W - f]) / 2, B[f] = (Z[f] - conj Z[W - f]) / (2 i).  The adjoint pass is the
// same idea backwards: a row's gradient is Re(F^H G) of its mirrored spectrum G, which only sees G's Hermitian part (the entries
// f = 0 and f = W / 2 enter with their real parts), so F^H (G_a + i G_b) = grad_a + i grad_b.  Half the butterflies of the
// row-by-row form (these kernels are instruction-bound) for the same HBM traffic.
#ifndef BNERV_FFT_LINES
#define BNERV_FFT_LINES 1
#endif
constexpr int LINES_PER_BLOCK = BNERV_FFT_LINES;            // complex lines (row pairs) per block
constexpr int ROWS_PER_BLOCK = 2 * LINES_PER_BLOCK;
static_assert(LINES_PER_BLOCK == 1 || LINES_PER_BLOCK == 2, "the staging loops of the row kernels split their index into at most two lines");
constexpr int ROW_U = LINES_PER_BLOCK == 1 ? 5 : 4;         // input elements per thread and batch (1280 points on 256 threads: one batch)
constexpr int COLS_PER_BLOCK = 4;

struct FftArgs {
    const float* pred; const float* target;
    float2* T;            // [BC][H][Wh] complex workspace: the input is real, so only the Wh = W/2 + 1 non-redundant columns of the
                          // row transform are kept (natural frequency order); the others are their conjugate mirrors
    int Wh;
    float* partial;       // [BC][ncolblk]
    float* grad;          // [BC][H][W]
    int BC, H, W;
    float gscale;         // c_fft / (B*C*H*W*2)
    int accumulate;       // rows_adj: grad += (1) or grad = (0)
    FftPlan prow, pcol;
};

template <int MAXR = BNERV_FFT_MAX_RADIX>
__device__ __forceinline__ void fft_rows_fwd_body(const FftArgs& a, const int bx) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float2* buf = reinterpret_cast<float2*>(sm);
    const int W = a.W;
    const size_t row0 = (size_t)bx * ROWS_PER_BLOCK;                    // global row index over BC*H
    const size_t nrows = (size_t)a.BC * a.H;
    const int nl = (int)min((size_t)ROWS_PER_BLOCK, nrows - row0);
    const int nlines = (nl + 1) >> 1;                                    // complex lines: rows (2 l, 2 l + 1) -> real / imaginary part
    float2* tw = buf + LINES_PER_BLOCK * W;
    int* lpos = reinterpret_cast<int*>(tw + W);
    TabRegs tr;
    tables_issue<true>(tr, a.prow);
    bool tabs_done = false;
    for (int i0 = threadIdx.x; i0 < nlines * W; i0 += blockDim.x * ROW_U) {   // 4 ROW_U loads in flight per thread (+ the tables), then the LDS stores
        float pa[ROW_U], ta[ROW_U], pb[ROW_U], tb[ROW_U];
#pragma unroll
        for (int u = 0; u < ROW_U; ++u) {
            const int i = i0 + u * blockDim.x;
            const int line = (LINES_PER_BLOCK > 1 && i >= W) ? 1 : 0, x = i - line * W;
            const bool oka = i < nlines * W, okb = oka && 2 * line + 1 < nl;
            const size_t o = (row0 + 2 * line) * W + x;
            pa[u] = oka ? a.pred[o] : 0.f;     ta[u] = oka ? a.target[o] : 0.f;
            pb[u] = okb ? a.pred[o + W] : 0.f; tb[u] = okb ? a.target[o + W] : 0.f;
        }
        if (!tabs_done) { tables_commit<true>(tr, tw, lpos, a.prow); tabs_done = true; }
#pragma unroll
        for (int u = 0; u < ROW_U; ++u) {
            const int i = i0 + u * blockDim.x;
            if (i < nlines * W) buf[i] = float2{pa[u] - ta[u], pb[u] - tb[u]};
        }
    }
    if (!tabs_done) tables_commit<true>(tr, tw, lpos, a.prow);            // (a thread without input elements still owns table entries)
    __syncthreads();
    fft_forward<MAXR>(buf, nlines, W, a.prow, tw);
    const int Wh = a.Wh;
    for (int i = threadIdx.x; i < nl * Wh; i += blockDim.x) {
        const int row = i / Wh, f = i - row * Wh;
        const float2* ln = buf + (row >> 1) * W;
        const float2 z = ln[lpos[f]], m = ln[lpos[f == 0 ? 0 : W - f]];
        // even row: (Z[f] + conj Z[W - f]) / 2;  odd row: (Z[f] - conj Z[W - f]) / (2 i)
        a.T[(row0 + row) * Wh + f] = (row & 1) ? float2{0.5f * (z.y + m.y), 0.5f * (m.x - z.x)} : float2{0.5f * (z.x + m.x), 0.5f * (z.y - m.y)};
    }
}

template <int MAXR = BNERV_FFT_MAX_RADIX>
__device__ __forceinline__ void fft_cols_body(const FftArgs& a, const int bx, const int bc, const int ncolblk) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float2* buf = reinterpret_cast<float2*>(sm);                          // [COLS_PER_BLOCK][H]
    __shared__ float red[4];
    const int H = a.H, W = a.Wh;                                           // W: kept columns (half spectrum)
    const int v0 = bx * COLS_PER_BLOCK;
    const int nc = min(COLS_PER_BLOCK, W - v0);
    float2* T = a.T + (size_t)bc * H * W;
    float2* tw = buf + COLS_PER_BLOCK * H;
    TabRegs tr;
    tables_issue<false>(tr, a.pcol);
    bool tabs_done = false;
    for (int i0 = threadIdx.x; i0 < H * nc; i0 += blockDim.x * 8) {       // column gather: 8 loads in flight per thread (+ the twiddles)
        float2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * blockDim.x;
            const int y = i / nc, c = i - y * nc;
            v[u] = i < H * nc ? T[(size_t)y * W + v0 + c] : float2{0.f, 0.f};
        }
        if (!tabs_done) { tables_commit<false>(tr, tw, nullptr, a.pcol); tabs_done = true; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * blockDim.x;
            const int y = i / nc, c = i - y * nc;
            if (i < H * nc) buf[c * H + y] = v[u];
        }
    }
    if (!tabs_done) tables_commit<false>(tr, tw, nullptr, a.pcol);
    __syncthreads();
    fft_forward<MAXR>(buf, nc, H, a.pcol, tw);
    float acc = 0.f;
    for (int i = threadIdx.x; i < H * nc; i += blockDim.x) {
        const float2 f = buf[i];           // lines are contiguous: nc*H elements
        const int col = v0 + i / H;        // a kept column stands for itself and for its mirror W_full - col, unless it is its own mirror
        const float wgt = (col == 0 || 2 * col == a.W) ? 1.f : 2.f;
        acc += wgt * (fabsf(f.x) + fabsf(f.y));
        buf[i] = float2{(f.x > 0.f) ? 1.f : ((f.x < 0.f) ? -1.f : 0.f), (f.y > 0.f) ? 1.f : ((f.y < 0.f) ? -1.f : 0.f)};
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.partial[(size_t)bc * ncolblk + bx] = red[0] + red[1] + red[2] + red[3];
    if (a.grad == nullptr) return;
    fft_adjoint<MAXR>(buf, nc, H, a.pcol, tw);
    for (int i = threadIdx.x; i < H * nc; i += blockDim.x) {
        const int y = i / nc, c = i - y * nc;
        T[(size_t)y * W + v0 + c] = buf[c * H + y];
    }
}

template <int MAXR = BNERV_FFT_MAX_RADIX>
__device__ __forceinline__ void fft_rows_adj_body(const FftArgs& a, const int bx) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float2* buf = reinterpret_cast<float2*>(sm);
    const int W = a.W;
    const size_t row0 = (size_t)bx * ROWS_PER_BLOCK;
    const size_t nrows = (size_t)a.BC * a.H;
    const int nl = (int)min((size_t)ROWS_PER_BLOCK, nrows - row0);
    const int nlines = (nl + 1) >> 1;
    float2* tw = buf + LINES_PER_BLOCK * W;
    int* lpos = reinterpret_cast<int*>(tw + W);
    const int Wh = a.Wh;
    TabRegs tr;
    tables_issue<true>(tr, a.prow);
    constexpr int AU = 4;
    // P = G_a + i G_b of the row pair, G = kept columns + their conjugate mirrors (self-mirrored columns with their real parts), into DIF order
    for (int i0 = threadIdx.x, first = 1; first || i0 < nlines * Wh; i0 += blockDim.x * AU, first = 0) {   // (every thread runs the first batch: it holds the barrier)
        float2 va[AU], vb[AU];
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const int i = i0 + u * blockDim.x;
            const int line = (LINES_PER_BLOCK > 1 && i >= Wh) ? 1 : 0, f = i - line * Wh;
            const bool oka = i < nlines * Wh, okb = oka && 2 * line + 1 < nl;
            const size_t o = (row0 + 2 * line) * Wh + f;
            va[u] = oka ? a.T[o] : float2{0.f, 0.f};
            vb[u] = okb ? a.T[o + Wh] : float2{0.f, 0.f};
        }
        if (first) { tables_commit<true>(tr, tw, lpos, a.prow); __syncthreads(); }     // (the position table is read below)
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const int i = i0 + u * blockDim.x;
            if (i < nlines * Wh) {
                const int line = (LINES_PER_BLOCK > 1 && i >= Wh) ? 1 : 0, f = i - line * Wh;
                float2 ga = va[u], gb = vb[u];
                const bool self = f == 0 || 2 * f == W;
                if (self) { ga.y = 0.f; gb.y = 0.f; }
                buf[line * W + lpos[f]] = float2{ga.x - gb.y, ga.y + gb.x};                       // G_a[f] + i G_b[f]
                if (!self) buf[line * W + lpos[W - f]] = float2{ga.x + gb.y, gb.x - ga.y};         // conj G_a[f] + i conj G_b[f]
            }
        }
    }
    // the gradient this launch adds to: loaded under the transform
    float ga[2 * ROW_U], gb[2 * ROW_U];
    const bool one_batch = nlines * W <= 2 * ROW_U * (int)blockDim.x;
    if (one_batch) {
#pragma unroll
        for (int u = 0; u < 2 * ROW_U; ++u) {
            const int i = threadIdx.x + u * blockDim.x;
            const int line = (LINES_PER_BLOCK > 1 && i >= W) ? 1 : 0, x = i - line * W;
            const bool oka = i < nlines * W, okb = oka && 2 * line + 1 < nl;
            const size_t o = (row0 + 2 * line) * W + x;
            ga[u] = (a.accumulate && oka) ? a.grad[o] : 0.f;
            gb[u] = (a.accumulate && okb) ? a.grad[o + W] : 0.f;
        }
    }
    __syncthreads();
    fft_adjoint<MAXR>(buf, nlines, W, a.prow, tw);
    for (int i0 = threadIdx.x; i0 < nlines * W; i0 += blockDim.x * 2 * ROW_U) {
        if (!one_batch) {
#pragma unroll
            for (int u = 0; u < 2 * ROW_U; ++u) {
                const int i = i0 + u * blockDim.x;
                const int line = (LINES_PER_BLOCK > 1 && i >= W) ? 1 : 0, x = i - line * W;
                const bool oka = i < nlines * W, okb = oka && 2 * line + 1 < nl;
                const size_t o = (row0 + 2 * line) * W + x;
                ga[u] = (a.accumulate && oka) ? a.grad[o] : 0.f;
                gb[u] = (a.accumulate && okb) ? a.grad[o + W] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 2 * ROW_U; ++u) {
            const int i = i0 + u * blockDim.x;
            if (i < nlines * W) {
                const int line = (LINES_PER_BLOCK > 1 && i >= W) ? 1 : 0, x = i - line * W;
                const size_t o = (row0 + 2 * line) * W + x;
                const float2 r = buf[i];
                a.grad[o] = ga[u] + a.gscale * r.x;
                if (2 * line + 1 < nl) a.grad[o + W] = gb[u] + a.gscale * r.y;
            }
        }
    }
}
