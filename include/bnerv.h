/*
 * bnerv.h -- C-ABI of libbnerv_hip.so: the MI355X (gfx950) kernels of the Boosting-NeRV conditional-decoder
 * train path.  This is the drop-in boundary.
 *
 * The reference (Xinjie-Q/Boosting-NeRV) is pure Python/PyTorch and has NO FFI: every arithmetic op on the path is an
 * ATen call made from the Python files cited below.  Each entry point here replaces the ATen call sequence of one
 * reference call site; the Python host package (boosting_nerv_amd/) binds them with ctypes and mirrors the reference's
 * module API (INTEGRATION.md shows the binding a reference maintainer would add).
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and ints; no torch types.  All tensors are DEVICE pointers to contiguous fp32 NCHW
 *     (OIHW for weights) unless stated otherwise; the caller owns every buffer (no ownership transfer, no allocation
 *     here); workspaces are passed in explicitly and their sizes are given by the matching *_ws_bytes() helper.
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and the call never synchronises.
 *   - Return 0 on success, negative BNERV_E_* on failure; bnerv_last_error() returns a thread-local message.
 *   - Thread-safe per stream; no global mutable state except read-only twiddle tables created through bnerv_fft_*.
 */
#ifndef BNERV_H
#define BNERV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BNERV_ABI_VERSION 9

#define BNERV_OK 0
#define BNERV_E_ARG (-1)      /* bad argument / unsupported shape */
#define BNERV_E_LAUNCH (-2)   /* hip launch error */
#define BNERV_E_WS (-3)       /* workspace too small */

int bnerv_abi_version(void);
const char* bnerv_last_error(void);
/* name of the gfx arch the code object was built for ("gfx950") */
const char* bnerv_build_arch(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Positional encoding.  Replaces PositionEncoding.forward (model_blocks.py:120-126):
 *   v = pos * bases ; out = cat[sin v, cos v]  -> [N, 2L]
 * f32 form: pos fp32, ONE IEEE fp32 multiply, accurate sinf/cosf (model_nerv.py:47-48, model_enerv.py:286-292).
 * f64 form: pos fp64, product and sin/cos in fp64, result cast to fp32 (HNeRV_Boost, model_hnerv.py:241).
 * `bases` is the fp32 table built by the host with the reference's own torch expression (model_blocks.py:113-117).
 * No backward: pos carries no gradient.
 * ------------------------------------------------------------------------------------------------------------------ */
int bnerv_pe_fwd_f32(void* stream, const float* pos, const float* bases, float* out, int N, int L);
int bnerv_pe_fwd_f64(void* stream, const double* pos, const float* bases, float* out, int N, int L);
/* f32 form on fp64 positions: pos is rounded to fp32 first (the `input[:, None].float()` of model_nerv.py:47 / model_enerv.py:286), then as _f32 */
int bnerv_pe_fwd_f32_from_f64(void* stream, const double* pos, const float* bases, float* out, int N, int L);

/* ------------------------------------------------------------------------------------------------------------------
 * Grouped dense layers on [B, I] vectors (1x1 convs on [B,C,1,1]).  Replaces the CustomConv2d(kernel_size=1) calls of
 * NeRV_MLP (model_blocks.py:66-71: stem / stem_t / t_branch) and of SFTLayer's four 1x1 convs (model_blocks.py:92-105).
 * One launch evaluates up to BNERV_MAX_DENSE_GROUPS independent layers  y = act(W x + b).
 *   act: 0 none, 1 relu, 2 sin.   aux (sin only, may be NULL): cos(Wx+b), saved for the backward.
 * ------------------------------------------------------------------------------------------------------------------ */
#define BNERV_MAX_DENSE_GROUPS 40
#define BNERV_ACT_NONE 0
#define BNERV_ACT_RELU 1
#define BNERV_ACT_SIN 2

typedef struct {
    const float* x;   /* [B, I] */
    const float* w;   /* [O, I] */
    const float* b;   /* [O] or NULL */
    float* y;         /* [B, O] */
    float* aux;       /* [B, O] or NULL */
    int I, O, act, _pad;
} bnerv_dense_fwd_desc;

typedef struct {
    const float* x;    /* [B, I]  layer input */
    const float* w;    /* [O, I] */
    const float* y;    /* [B, O]  layer output (relu mask) */
    const float* aux;  /* [B, O]  cos(pre) for sin */
    const float* dy;   /* [B, O]  incoming gradient */
    float* dpre;       /* [B, O]  scratch: gradient wrt pre-activation (written) */
    float* dw;         /* [O, I]  written */
    float* db;         /* [O]     written (may be NULL) */
    float* dx_part;    /* [nchunk, B, I] partial input gradients (NULL: not needed); nchunk = ceil(O / BNERV_DENSE_DX_CHUNK) */
    int I, O, act, _pad;
} bnerv_dense_bwd_desc;

#define BNERV_DENSE_DX_CHUNK 64

int bnerv_dense_grouped_fwd(void* stream, const bnerv_dense_fwd_desc* groups, int n_groups, int B);
int bnerv_dense_grouped_bwd(void* stream, const bnerv_dense_bwd_desc* groups, int n_groups, int B);

/* The time-embedding branch of NeRV_Boost.forward except the stem's second layer, as ONE launch (ABI 8; csrc/dense.hip):
 *   pe = PositionEncoding(pos)                               model_nerv.py:47, model_blocks.py:120-126   (fp64 position rounded to fp32 first)
 *   stem layer 0 : sy0 = sin(sw0 pe + sb0) [SH]                                model_nerv.py:48-50, NeRV_MLP model_blocks.py:66-71
 *   stem_t       : ty0 = sin(tw0 pe + tb0) [TH];  ty1 = sin(tw1 ty0 + tb1) [TO] = z_t
 *   every TAT modulation MLP i:  hs_i = relu(w1_i z_t + b1_i) [TO];  out_i = w2_i hs_i + b2_i [C_i]          SFTLayer, model_blocks.py:92-105
 * (the stem's second layer follows as an ordinary bnerv_dense_grouped_fwd launch).  Every tensor the five-launch form leaves behind --
 * outputs and the cosines saux0 / taux* of the sin layers -- is written, so the backward can be bnerv_time_branch_bwd (below) or the bnerv_dense_grouped_bwd sequence it was derived from.
 * Requires w1_i [TO, TO] and w2_i [C_i, TO] row-major, sw0 / tw0 [*, 2L].  Returns 1 when the shapes are not this kernel's (B > 4, 2L > 256,
 * TH > 64, TO > 32, C_i > 128, more than BNERV_MAX_DENSE_GROUPS MLPs, unaligned weights): the caller issues the grouped launches. */
typedef struct { const float* w1; const float* b1; const float* w2; const float* b2; float* hs; float* out; int C; int _pad; } bnerv_time_branch_mlp;
typedef struct {
    const double* pos;     /* [B] */
    const float* bases;    /* [L] */
    float* pe;             /* [B, 2L] */
    const float* sw0; const float* sb0;                                          /* stem layer 0: [SH, 2L], [SH] */
    float* sy0; float* saux0;                                                    /* [B, SH] x 2 */
    const float* tw0; const float* tb0; const float* tw1; const float* tb1;      /* stem_t: [TH, 2L], [TH], [TO, TH], [TO] */
    float* ty0; float* taux0; float* ty1; float* taux1;                          /* [B, TH] x 2, [B, TO] x 2 */
    int B, L, SH, TH, TO, n_mlp;
} bnerv_time_branch_desc;
int bnerv_time_branch_fwd(void* stream, const bnerv_time_branch_desc* d, const bnerv_time_branch_mlp* mlps /* [n_mlp] */);

/* The backward of that branch (the stem's second layer included) as TWO launches instead of the five dependent grouped ones (csrc/dense.hip):
 *   launch A: the stem's layer 1 (the grouped kernel's own row and chunk blocks: d_sw1, d_sb1, the chunk partials of d_sy0)  |  one block per
 *             modulation MLP: BOTH its layers (dw2, db2, dw1, db1) and its slab of the d z_t partials;
 *   launch B: the stem's layer 0 from the summed chunk partials (d_sw0, d_sb0)  |  one block: d z_t = sum of the slabs (+ d_ty1), then stem_t's
 *             layer 1 and layer 0 (d_tw1, d_tb1, d_tw0, d_tb0).
 * Every gradient has the bits of the five-launch form: the same fmaf chains, and the two cross-block sums in the order of the deferred slab
 * reductions.  d_out of an MLP may be NULL (no gradient arrived: zeros), d_ty1 may be NULL (nothing is added).  Scratch is the caller's: sx_part
 * [ceil(SO / BNERV_DENSE_DX_CHUNK), B, SH], zt_part [n_mlp, B, TO], s_dpre [B, SO].  Nothing is allocated and nothing synchronises (graph capture).
 * Returns 1 -- before any device call -- when the shapes are not these kernels' (B > 4, 2L > 256, SH > 4096, TH > 64, TO > 32, C_i > 128,
 * n_mlp + 1 > BNERV_MAX_DENSE_GROUPS): the caller issues the five grouped launches.  Both tables travel by value in the kernel-argument
 * segment (<= 4096 bytes): sizeof(bnerv_time_branch_bwd_mlp) is BNERV_TIME_BRANCH_BWD_MLP_BYTES, sizeof(bnerv_time_branch_bwd_desc) is
 * BNERV_TIME_BRANCH_BWD_DESC_BYTES. */
#define BNERV_TIME_BRANCH_BWD_MLP_BYTES 72
#define BNERV_TIME_BRANCH_BWD_DESC_BYTES 216
typedef struct {
    const float* w1; const float* w2;      /* [TO, TO], [C, TO] */
    const float* hs;                       /* [B, TO]  relu output of layer 0 (saved by the forward) */
    const float* d_out;                    /* [B, C]   incoming gradient, or NULL */
    float* dw1; float* db1; float* dw2; float* db2;      /* written */
    int C; int _pad;
} bnerv_time_branch_bwd_mlp;
typedef struct {
    const float* pe;                                                             /* [B, 2L] */
    const float* sw1; const float* sy0; const float* saux0; const float* saux1;  /* stem: [SO, SH], [B, SH] x 2, [B, SO] */
    const float* d_sy1;                                                          /* [B, SO] */
    const float* tw1; const float* ty0; const float* taux0; const float* ty1; const float* taux1;     /* stem_t: [TO, TH], [B, TH] x 2, [B, TO] x 2 */
    const float* d_ty1;                                                          /* [B, TO] or NULL */
    float* d_sw0; float* d_sb0; float* d_sw1; float* d_sb1;                      /* written: [SH, 2L], [SH], [SO, SH], [SO] */
    float* d_tw0; float* d_tb0; float* d_tw1; float* d_tb1;                      /* written: [TH, 2L], [TH], [TO, TH], [TO] */
    float* sx_part; float* zt_part; float* s_dpre;                               /* scratch (see above) */
    int B, L, SH, SO, TH, TO, n_mlp, _pad;
} bnerv_time_branch_bwd_desc;
int bnerv_time_branch_bwd(void* stream, const bnerv_time_branch_bwd_desc* d, const bnerv_time_branch_bwd_mlp* mlps /* [n_mlp] */);

/* Stand-alone TAT affine  y = x*(scale[b,c]+1) + shift[b,c]  (SFTLayer.forward, model_blocks.py:101-105) and its backward:
 *   dx = g*(scale+1);  part[chunk][0][b,c] = sum_chunk g*x;  part[chunk][1][b,c] = sum_chunk g
 * finish with bnerv_reduce_slabs(part, BNERV_SFT_CHUNKS, 2*B*C, out) -> out[0][b,c] = dscale, out[1][b,c] = dshift.
 * (Inside the decoder blocks the affine is fused into the conv prologues; these two exist for the module-level API.) */
#define BNERV_SFT_CHUNKS 32
int bnerv_sft_affine_fwd(void* stream, const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW);
int bnerv_sft_affine_bwd(void* stream, const float* x, const float* scale, const float* g, float* dx, float* part, int B, int C, int HW);

/* LayerNorm over the channel axis of an NCHW tensor (reference: model_blocks.py:250-270 `LayerNorm`, data_format
 * "channels_first"; the "channels_last" form of the ConvNeXt block is the same arithmetic on the permuted tensor):
 *   y[b,c,p] = w[c] * (x[b,c,p] - mean_c) / sqrt(var_c + eps) + b[c],  var = mean_c (x - mean_c)^2.   1 <= C <= 64.
 * bwd: dx as autograd's; dwb = [2][C] = (dw, db), summed over b and p in a fixed order (ws: bnerv_lncf_bwd_ws_bytes). */
int bnerv_lncf_fwd(void* stream, const float* x, const float* w, const float* b, float* y, int B, int C, int HW, float eps);
size_t bnerv_lncf_bwd_ws_bytes(int B, int C, int HW);
int bnerv_lncf_bwd(void* stream, const float* x, const float* w, const float* dy, float* dx, float* dwb, void* ws, size_t ws_bytes,
                   int B, int C, int HW, float eps);

/* out[i] = sum_{s<n_slabs} slabs[s*count + i]   (deterministic finish of every split reduction in this library) */
int bnerv_reduce_slabs(void* stream, const float* slabs, int n_slabs, int count, float* out);

/* Deferred form of the same reduction.  On MI355X a tiny dependent kernel between two big ones costs ~10 us of pipeline,
 * so the ~45 slab reductions of a train step are queued instead of launched: the next bnerv_conv_igemm / bnerv_conv_wgrad
 * launch GIVEN THE SAME CONTEXT whose kernel can host them executes the queued reductions at the end of its least-loaded
 * blocks (same fixed summation order whoever executes them).  `slabs` and `out` must stay valid, and `out` must not be read,
 * until a hosting launch or bnerv_flush_deferred() has been issued on the stream; bnerv_flush_deferred launches whatever is
 * still queued (a no-op when the queue is empty).
 *
 * The queue lives in a CALLER-OWNED context: the library keeps no mutable global state.  One context serves one stream
 * (every launch that names it must go to that stream, from one thread at a time); contexts are independent of each other, so
 * two streams / two models in one process never see each other's jobs.  A NULL context is legal everywhere: nothing is
 * hosted, and a deferral request is executed immediately instead. */
typedef struct bnerv_ctx bnerv_ctx;
int bnerv_ctx_create(bnerv_ctx** out);
void bnerv_ctx_destroy(bnerv_ctx* ctx);
/* The context also owns a device scratch buffer (pre-split weight fragments of the wide split conv kernels).  It grows on demand,
 * except while its stream is being captured into a graph (allocation is illegal there: such a call falls back to the f32 kernels).
 * A caller that is about to capture on a fresh stream reserves what the eager steps needed:  bnerv_ctx_reserve(new_ctx,
 * bnerv_ctx_scratch_bytes(old_ctx)). */
size_t bnerv_ctx_scratch_bytes(const bnerv_ctx* ctx);
int bnerv_ctx_reserve(bnerv_ctx* ctx, size_t bytes);
/* Weight-fragment plan of a repeated step (ABI 4).  Every wide split conv call (forward conv, up-conv, data gradient) is preceded
 * by a small launch that splits its weight tensor into 16-bit matrix fragments; inside one train step the weights do not change
 * between the first forward conv and the last data gradient (the optimizer runs after backward), so a step that is replayed as a
 * graph can prepare ALL of them in one launch at its start:
 *     bnerv_ctx_wplan_record(ctx);  <one forward + backward with this context, eager>;  n = bnerv_ctx_wplan_freeze(ctx);
 *     per step (normally inside the capture):  bnerv_ctx_wplan_run(ctx, stream);  <forward, backward>;  bnerv_ctx_wplan_end(ctx);
 * record: forget any previous plan and note, for every wide split conv call of this context, (weight pointer, layout, fragment
 * geometry).  freeze: allocate one arena for the distinct entries (device synchronize; not inside a capture); returns their number
 * (>= 0) or a negative error.  run: ONE launch that writes every entry's fragments from the CURRENT weights; from then until
 * wplan_end, a conv call of this context whose weight pointer / geometry matches an entry reads the arena and launches no
 * preparation of its own; calls that match nothing, and all calls outside run..end, behave as before (own preparation, scratch
 * buffer).  The caller guarantees that the planned weight tensors are not written between run and end and that their addresses
 * stay what they were at record time; the fragments are the same bits either way, so results do not depend on the plan. */
int bnerv_ctx_wplan_record(bnerv_ctx* ctx);
int bnerv_ctx_wplan_freeze(bnerv_ctx* ctx);
int bnerv_ctx_wplan_run(bnerv_ctx* ctx, void* stream);
/* bnerv_ctx_wplan_run and bnerv_fetch_frame (below) as ONE launch (ABI 8): both open a captured step on a resident clip and neither depends on the
 * other.  Returns 1 when the context has no frozen plan with work -- the caller then calls bnerv_fetch_frame alone. */
int bnerv_ctx_wplan_run_fetch(bnerv_ctx* ctx, void* stream, const float* clip, const double* norms, const float* sel_dev, int n_frames, size_t frame_elems,
                              float* dst_img, double* dst_norm);
int bnerv_ctx_wplan_end(bnerv_ctx* ctx);
int bnerv_ctx_wplan_entries(const bnerv_ctx* ctx);     /* entries of the frozen plan (0: none) */
int bnerv_reduce_slabs_deferred(bnerv_ctx* ctx, void* stream, const float* slabs, int n_slabs, int count, float* out);
int bnerv_flush_deferred(bnerv_ctx* ctx, void* stream);
int bnerv_deferred_pending(const bnerv_ctx* ctx);

/* ------------------------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution (fp32 MFMA 16x16x4), stride 1, square kernel k in {1,3}, zero padding (k-1)/2, with fused
 * input prologue and output epilogue.  One kernel family serves the forward conv and the data gradient.
 * Replaces CustomConv2d.forward = F.conv2d (lib/quant_ops.py:39-41) as used by UpConv (model_blocks.py:196-220),
 * ResBlock_SFT (model_blocks.py:74-89), Conv_Up_Block (model_enerv.py:73-102), DownConv 'conv' (model_blocks.py:184-185)
 * and head_layer (model_nerv.py:41,56), together with the elementwise ops around it:
 *   SFTLayer affine x*(scale+1)+shift (model_blocks.py:101-105), GELU (model_blocks.py:81), PixelShuffle + Sin
 *   (model_blocks.py:213-218, :129-134), residual add (model_blocks.py:89), OutImg tanh (model_blocks.py:57-63),
 * and, for the data gradient, autograd's backward of the same.
 * ------------------------------------------------------------------------------------------------------------------ */
/* input prologues */
#define BNERV_IN_PLAIN 0         /* a = x */
#define BNERV_IN_AFFINE 1        /* a = x*(1+scale[b,c]) + shift[b,c]          (padding applies AFTER the affine) */
#define BNERV_IN_GELU_AFFINE 2   /* a = gelu(x)*(1+scale[b,c]) + shift[b,c] */
#define BNERV_IN_UNSHUFFLE 3     /* a[c*s*s+i*s+j][y][x] = x[c][y*s+i][x*s+j]  (pixel-unshuffle gather, s = in_s) */
#define BNERV_IN_TANHGRAD 4      /* a = x * 0.5*(1-(2*aux0-1)^2)               (x = dL/dimg, aux0 = img = OutImg output) */
/* output epilogues (v = conv result, o = output element) */
#define BNERV_EP_BIAS 0          /* out = v + bias                              (optionally pixel-shuffled by out_s) */
#define BNERV_EP_BIAS_SIN 1      /* u = v + bias; out = sin u; out2 = cos u     (pixel-shuffled by out_s) */
#define BNERV_EP_BIAS_RES 2      /* out = v + bias + aux0 */
#define BNERV_EP_BIAS_TANH 3     /* out = tanh(v + bias)*0.5 + 0.5 */
#define BNERV_EP_PLAIN 4         /* out = v */
#define BNERV_EP_DGELU 5         /* out = v*(1+scale[b,c])*gelu'(aux0);   partial: ds += v*gelu(aux0), dt += v */
#define BNERV_EP_DSIN 6          /* t = aux1 + v*(1+scale[b,c]); out = t*aux2 (aux2 NULL: 1); partial: ds += v*aux0, dt += v */
#define BNERV_EP_BIAS_GELU 7     /* u = v + bias; out = gelu(u); out2 = gelu'(u) (out2 may be NULL: decode)  (the TAT block saves both instead of u: the three
                                    consumers -- next conv, its weight gradient, the dGELU epilogue -- then need no erf/exp) */
#define BNERV_EP_DGELU_SAVED 8   /* out = v*(1+scale[b,c])*aux0 (aux0 = saved gelu');  partial: ds += v*aux1 (aux1 = saved gelu), dt += v */

typedef struct {
    const float* x;       /* input, conv-space [B, Cin, H, W]  (IN_UNSHUFFLE: stored as [B, Cin/s^2, H*s, W*s]) */
    const float* w;       /* weight tensor [wCo, wCi, k, k] (OIHW, as in state_dict) */
    const float* bias;    /* [Cout] or NULL */
    float* out;           /* conv-space [B, Cout, H, W], stored pixel-shuffled as [B, Cout/s^2, H*s, W*s] when out_s>1 */
    float* out2;          /* EP_BIAS_SIN: cos(u), same layout as out (may be NULL) */
    const float* aux0;    /* see epilogue / prologue tables */
    const float* aux1;
    const float* aux2;
    const float* scale;   /* [B, Cin] for IN_AFFINE / IN_GELU_AFFINE;  [B, Cout] for EP_DGELU / EP_DSIN */
    const float* shift;   /* [B, Cin] for IN_AFFINE / IN_GELU_AFFINE */
    float* partial;       /* EP_DGELU / EP_DSIN: [R][B][2][Cout] per-tile partial sums (written), R = bnerv_conv_partial_rows(d);
                             finish with bnerv_reduce_slabs(partial, R, B*2*Cout, out) -> out[b][0][c] = ds, out[b][1][c] = dt.
                             EP_PLAIN: optional split-K workspace (see bnerv_conv_splitk_ws_bytes) */
    int B, Cin, Cout, H, W;
    int k;                /* 1 or 3 */
    int in_mode, ep_mode;
    int in_s, out_s;      /* shuffle factors (1 = none) */
    int transposed;       /* 0: forward  (Cout=wCo, Cin=wCi, W(co,ci,t) = w[co][ci][t]);
                             1: data gradient (Cout=wCi, Cin=wCo, W(co,ci,t) = w[ci][co][k*k-1-t]) */
    int wCo, wCi;
    bnerv_ctx* ctx;       /* deferred-reduction context of the stream (may be NULL) */
} bnerv_conv_desc;

/* number of 8x32 spatial tiles per sample of an H x W conv-space image */
int bnerv_conv_tiles(int H, int W);
/* EP_DGELU / EP_DSIN: number of per-sample rows R this descriptor's kernel writes into `partial` ([R][B][2][Cout]); the
 * kernel is chosen from the shape and pointer alignment, so fill in every field before asking.  For the epilogues that write rows
 * the answer does not depend on `partial`, which may still be NULL.  (For EP_PLAIN, which writes none, the answer names the tiles of
 * the family that the launch would run with `partial` as given: a workspace changes that family.) */
int bnerv_conv_partial_rows(const bnerv_conv_desc* d);
/* Kernel selection as a host query (additive to ABI 9; no device is touched, like bnerv_conv_partial_rows).  bnerv_conv_igemm decides
 * once which kernel family takes a descriptor (csrc/route.h); these report that decision, so that it can be tested without a GPU.
 * bnerv_conv_family: the BNERV_CONV_FAM_* id that bnerv_conv_igemm(d) runs, read from d exactly as the launch reads it (`partial`
 * included: an EP_PLAIN workspace enables split-K and the stem kernel, and the 3x3 head's data gradient wants none), or -1 for a
 * descriptor without positive dimensions or with k other than 1 or 3.  *rows (may be NULL) = bnerv_conv_partial_rows(d): the tiles of
 * that family's grid -- 4x16 for SMALL / SMALL96, bnerv_conv_tiles otherwise.  For the sums epilogues the answer does not depend on
 * `partial`.  A WIDE_BF16 route may still fall to Q4 / GENERIC at launch when the context has no scratch for the weight fragments
 * (same 8x32 tiles; the launch checks that). */
#define BNERV_CONV_FAM_HEAD1_FWD 0      /* 1x1 head 12 -> 3 + tanh, streaming */
#define BNERV_CONV_FAM_HEAD1_DGRAD 1    /* its data gradient (tanh-grad prologue), streaming */
#define BNERV_CONV_FAM_HEAD3 2          /* 3x3 head with 3 outputs: forward + tanh, or its data gradient (csrc/head3.hip) */
#define BNERV_CONV_FAM_STEM_DGRAD 3     /* image of <= 256 pixels, long K: K-slice slabs in `partial` (csrc/stem.hip) */
#define BNERV_CONV_FAM_SMALL 4          /* low-resolution stages, 4x16 tiles (csrc/convs.hip) */
#define BNERV_CONV_FAM_SMALL96 5        /* the same with 33..96 staged channels */
#define BNERV_CONV_FAM_WIDE_BF16 6      /* wide layers on split bf16 (csrc/convbf.hip) */
#define BNERV_CONV_FAM_Q4 7             /* <= 12-channel 3x3 layers on the 4x4x1 MFMA (csrc/conv4.hip) */
#define BNERV_CONV_FAM_GENERIC 8        /* the 16x16x4 f32 kernels of csrc/conv.hip (lean, fast, generic) */
int bnerv_conv_family(const bnerv_conv_desc* d, int* rows);
/* EP_PLAIN only: bytes of split-K workspace this layer wants (0 = none).  Layers with a long K loop and almost no
 * spatial parallelism (the low-resolution data gradients, e.g. Cin = 750 at 9x16) split their input-channel range over
 * work items; pass a buffer of this size in `partial` and bnerv_conv_igemm finishes with a deterministic slab reduction.
 * With partial == NULL the layer runs unsplit. */
size_t bnerv_conv_splitk_ws_bytes(const bnerv_conv_desc* d);
int bnerv_conv_igemm(void* stream, const bnerv_conv_desc* d);

/* Weight + bias gradient (autograd's backward of F.conv2d wrt weight/bias at the same call sites):
 *   dw[co][ci][t] = sum_{b,p} g[b][co][p] * a[b][ci][p + t - pad],  db[co] = sum_{b,p} g[b][co][p]
 * a = prologue(x) (IN_PLAIN / IN_AFFINE / IN_GELU_AFFINE), g gathered with pixel-unshuffle g_s or through tanh'
 * (g_mode BNERV_IN_TANHGRAD with gaux = img).  Split over spatial tiles into slabs, finished deterministically. */
typedef struct {
    const float* x;       /* [B, Cin, H, W] */
    const float* g;       /* [B, Cout, H, W] conv-space, stored shuffled [B, Cout/s^2, H*s, W*s] when g_s>1 */
    const float* gaux;    /* img for BNERV_IN_TANHGRAD */
    const float* scale;   /* [B, Cin] */
    const float* shift;   /* [B, Cin] */
    float* dw;            /* [Cout, Cin, k, k] written */
    float* db;            /* [Cout] written (may be NULL) */
    void* ws;             /* workspace of bnerv_conv_wgrad_ws_bytes() bytes */
    size_t ws_bytes;
    int B, Cin, Cout, H, W, k;
    int in_mode;          /* prologue on x */
    int g_mode;           /* BNERV_IN_PLAIN / BNERV_IN_UNSHUFFLE / BNERV_IN_TANHGRAD */
    int g_s;
    int defer_finish;     /* 1: queue the slab reduction into dw/db (see bnerv_reduce_slabs_deferred) instead of launching it */
    bnerv_ctx* ctx;       /* deferred-reduction context of the stream (NULL: nothing hosted, defer_finish ignored) */
} bnerv_wgrad_desc;

size_t bnerv_conv_wgrad_ws_bytes(int B, int Cin, int Cout, int H, int W, int k);
int bnerv_conv_wgrad(void* stream, const bnerv_wgrad_desc* d);
/* The BNERV_WGRAD_FAM_* id that bnerv_conv_wgrad(d) runs (host query, additive to ABI 9; -1 for a descriptor without positive dimensions
 * or with k other than 1 or 3) and, in *n_slabs (may be NULL), the slabs that family writes into `ws` (0 for STEM: dw / db directly). */
#define BNERV_WGRAD_FAM_STEM 0          /* image of <= 256 pixels, >= 64 output channels (csrc/stem.hip) */
#define BNERV_WGRAD_FAM_GEMM1X1 1       /* k = 1 with >= 16 channels on both sides: a GEMM over the pixels (csrc/wgrad1.hip) */
#define BNERV_WGRAD_FAM_LEAN 2          /* <= 16 output channels, <= 12 (k = 3) / 15 (k = 1) input channels */
#define BNERV_WGRAD_FAM_WIDE_BF16 3     /* > 16 output channels on split bf16 */
#define BNERV_WGRAD_FAM_WIDE_F32 4      /* the other stride-1 3x3 layers with aligned rows */
#define BNERV_WGRAD_FAM_GENERIC 5
int bnerv_conv_wgrad_family(const bnerv_wgrad_desc* d, int* n_slabs);

/* ------------------------------------------------------------------------------------------------------------------
 * 5x5 'same' convolution family of the HNeRV baseline decoder (csrc/conv5.hip; additive to ABI 9).  Replaces the F.conv2d of
 * UpConv 'pshuffel' with ks = 5 (model_blocks.py:196-220) as built by HNeRV (model_hnerv.py:49-56, `--ks 0_1_5`), its PixelShuffle and
 * the GELU of NeRVBlock (model_blocks.py:34-46), and autograd's backward of the three.  f32 contract on the bf16 matrix pipe (three
 * bf16 pieces per operand, six products, f32 accumulate).  The descriptors are those of bnerv_conv_igemm / bnerv_conv_wgrad with
 *   k = 5;  any Cin, Cout, B, H, W >= 1;
 *   bnerv_conv5_igemm:  in_mode IN_PLAIN | IN_UNSHUFFLE (in_s 1 | 2); aux0 != NULL multiplies the gathered input element-wise by
 *                       aux0 (same storage layout as x: the saved gelu' of the block, so du = g * gelu'(u) is never written out);
 *                       ep_mode EP_BIAS | EP_BIAS_GELU (out2 = gelu'(u), may be NULL) | EP_PLAIN; out_s 1 | 2; transposed as documented above.
 *                       ws: bnerv_conv5_ws_bytes(Cin, Cout) bytes of 16-byte aligned device memory (the split weight fragments of THIS
 *                       call; written by a preparation launch, then read by the main launch).
 *   bnerv_conv5_wgrad:  in_mode IN_PLAIN; g_mode IN_PLAIN | IN_UNSHUFFLE (g_s 1 | 2); gaux != NULL multiplies the gathered gradient by gaux
 *                       (same layout as g); ws of bnerv_conv5_wgrad_ws_bytes() bytes; the slab sums are finished in a fixed order by a
 *                       launch of their own (defer_finish / ctx are ignored).
 * ------------------------------------------------------------------------------------------------------------------ */
size_t bnerv_conv5_ws_bytes(int Cin, int Cout);
int bnerv_conv5_igemm(void* stream, const bnerv_conv_desc* d, void* ws, size_t ws_bytes);
size_t bnerv_conv5_wgrad_ws_bytes(int B, int Cin, int Cout, int H, int W);
int bnerv_conv5_wgrad(void* stream, const bnerv_wgrad_desc* d);
/* Streaming GELU around the 1x1 / 3x3 up-convs of the same decoder: y = gelu(u), gp = gelu'(u) (gp may be NULL; y may alias u), and the
 * element-wise product out = a * b (du = g * gelu'). */
int bnerv_gelu_fwd(void* stream, const float* u, float* y, float* gp, size_t n);
int bnerv_mul(void* stream, const float* a, const float* b, float* out, size_t n);

#define BNERV_LOSS_STATS 5
/* ------------------------------------------------------------------------------------------------------------------
 * CEM compression path: the per-step quantise + rate term of model.cal_params(entropy_model)
 * (model_hnerv.py:292-303) fused over tensors.  Per tensor (per-tensor `scale`, Gaussian rate model):
 *   code = w / scale;  dequant = round(code) * scale                                   Scale_T.forward, lib/transform_ops.py:239-251
 *   mu = mean(code), sigma = std(code);  x = code + noise (training) | round(code)      DiffEntropyModel, lib/entropy_model.py:21-43
 *   bits = sum max(-log2(Phi((x+.5-mu)/sigma) - Phi((x-.5-mu)/sigma) + 1e-5), 0)
 * stats[item] = {bits, mu, sigma, n}.  Backward: d_bits[item] = dL/d bits, d_dequant = dL/d dequant (NULL: none);
 * writes dw (NULL: skipped) and dscale[item], including the paths through mu, sigma and the LowerBound gate (:100-114).
 * `first` = index of the chunk's first tensor in stats / d_bits / dscale (tables travel by value, <= 48 tensors per launch). */
#define BNERV_CEM_MAX_TENSORS 48
typedef struct { const float* w; const float* scale; const float* noise; float* dequant; int n; int _pad; } bnerv_cem_item;
typedef struct { bnerv_cem_item it[BNERV_CEM_MAX_TENSORS]; int n_items; int training; int first; int _pad; } bnerv_cem_chunk;
typedef struct { const float* w; const float* scale; const float* noise; const float* d_dequant; float* dw; int n; int _pad; } bnerv_cem_item_bwd;
typedef struct { bnerv_cem_item_bwd it[BNERV_CEM_MAX_TENSORS]; int n_items; int training; int first; int _pad; } bnerv_cem_chunk_bwd;
/* Every tensor is cut into chunks of 8192 elements (one block each); the chunk partial sums (f64, fixed order) live in a caller-provided
 * workspace of bnerv_cem_ws_bytes(n_items, numel of the largest tensor of the chunk) bytes per call (ABI 3). */
size_t bnerv_cem_ws_bytes(int n_items, int max_n);
int bnerv_cem_scale_fwd(void* stream, const bnerv_cem_chunk* chunk, float* stats, void* ws, size_t ws_bytes);
int bnerv_cem_scale_bwd(void* stream, const bnerv_cem_chunk_bwd* chunk, const float* stats, const float* d_bits, float* dscale,
                        void* ws, size_t ws_bytes);

/* ------------------------------------------------------------------------------------------------------------------
 * Bitstream decoder (additive to ABI 9; csrc/codec.hip, boosting_nerv_amd/codec.py).
 *   bnerv_dequant_table:  for every item  out[i] = float(q[i]) * scale[0]  (+ beta[0] when beta != NULL), i < n: the de-quantisation of
 *       Scale_T / ScaleBeta_T (lib/transform_ops.py) from int32 symbols, every product and sum ONE IEEE fp32 operation (no fused
 *       multiply-add), i.e. the bits of torch's `quant * scale` and `quant * scale + beta`.  <= BNERV_CEM_MAX_TENSORS items per launch (the
 *       table travels by value), every item cut into chunks of BNERV_DEQUANT_CHUNK elements, one block each.  16-byte loads / stores where q
 *       and out are 16-byte aligned and n % 4 == 0, element by element otherwise (4-byte alignment is all that is required).
 *   bnerv_frame_to_u8:  x [B, 3, H, W] fp32 planar -> out [B, H, W, 3] uint8 interleaved, u = (uint8)(clamp(x, 0, 1) * 255.0f + 0.5f) with the
 *       multiply and the add rounded separately (train_nerv_all._save_images).  Four pixels per thread (three 16-byte loads, three dword
 *       stores) where H * W % 4 == 0, x is 16-byte and out 4-byte aligned; pixel by pixel otherwise.  NaN inputs are not defined. */
#define BNERV_DEQUANT_CHUNK 8192
typedef struct { const int* q; float* out; const float* scale; const float* beta; int n; int _pad; } bnerv_dequant_item;
typedef struct { bnerv_dequant_item it[BNERV_CEM_MAX_TENSORS]; int n_items; int _pad; } bnerv_dequant_chunk;
int bnerv_dequant_table(void* stream, const bnerv_dequant_chunk* chunk);
int bnerv_frame_to_u8(void* stream, const float* x, unsigned char* out, int B, int H, int W);

/* ------------------------------------------------------------------------------------------------------------------
 * Raw planar YUV 4:2:0 video in and out (additive to ABI 9; csrc/yuv.hip, boosting_nerv_amd/yuvio.py; definitions: DESIGN section 25).
 * A raw frame is plane Y [H, W], then U [H/2, W/2], then V [H/2, W/2], bytes_per_sample 1 (yuv420p) or 2 (yuv420p10le, little endian);
 * frame b starts frame_stride_bytes * b bytes behind the pointer.  The kernels know no standard: bnerv_yuv_coeffs carries what the host
 * computed in float64 --
 *   load:   n_p = (sample_p - off[p]) * scale[p] for p = Y, U, V;  rgb[c] = clamp(m[3c] n_Y + m[3c+1] n_U + m[3c+2] n_V, 0, 1)
 *   store:  v_p = m[3p] R + m[3p+1] G + m[3p+2] B from RGB clamped to [0, 1];  code_p = clamp(floor(off[p] + scale[p] * v_p + 0.5), 0, maxcode)
 *           (chroma v_p filtered [1 2 1] / 4 along the row at even x with the left edge clamped, then averaged over the row pair)
 *   bnerv_yuv420_to_rgb:  src -> out [B, 3, ch, cw] fp32, the crop window at (top, left) of the src_h x src_w frame (any parity); chroma
 *       up-sampled for MPEG-2 "left" siting on the sample values, in source coordinates.
 *   bnerv_rgb_to_yuv420:  x [B, 3, H, W] fp32 -> out in file layout.
 * Both validate before any launch (null pointers, odd dimensions, bytes_per_sample, a crop that leaves the frame, a stride smaller than a
 * frame); fp32 operands need 4-byte, 16-bit samples 2-byte alignment, every wider access is chosen per address. */
typedef struct { float m[9]; float off[3]; float scale[3]; float maxcode; } bnerv_yuv_coeffs;
int bnerv_yuv420_to_rgb(void* stream, const void* src, int bytes_per_sample, int B, size_t frame_stride_bytes, int src_h, int src_w, int top,
                        int left, float* out, int ch, int cw, const bnerv_yuv_coeffs* coeffs);
int bnerv_rgb_to_yuv420(void* stream, const float* x, int B, int H, int W, void* out, int bytes_per_sample, size_t frame_stride_bytes,
                        const bnerv_yuv_coeffs* coeffs);

/* Scoring a decoded clip against its raw source (additive to ABI 9; csrc/yuv.hip; definitions: DESIGN section 32).
 *   bnerv_yuv420_sse:  a = B packed H x W frames in file layout (what bnerv_rgb_to_yuv420 writes), b = B raw src_h x src_w frames of the same
 *       bytes_per_sample; the window of b starts at (top, left), both even, its chroma at (top/2, left/2).  out[B][3] (8-byte aligned) receives the
 *       exact sums of squared differences of the integer codes per frame and plane Y, U, V.  The call zeroes out itself (a memset in front of the
 *       launch, on `stream`: capturable) and accumulates with 64-bit integer atomics: the result does not depend on the order of the additions.
 *   bnerv_yuv_luma_f32:  the H x W luma window at (top, left), any parity, of B raw src_h x src_w frames -> out [B, 1, H, W] fp32 =
 *       float(code) / maxcode, the correctly rounded fp32 division (maxcode: 255 or 1023 as a float).
 * Both validate like the two entry points above (plus: a window that leaves the frame, an odd window offset for the SSE); every access wider than a
 * sample is chosen per address. */
int bnerv_yuv420_sse(void* stream, const void* a, size_t a_stride_bytes, const void* b, size_t b_stride_bytes, int bytes_per_sample, int B, int H, int W,
                     int src_h, int src_w, int top, int left, unsigned long long* out);
int bnerv_yuv_luma_f32(void* stream, const void* src, int bytes_per_sample, int B, size_t frame_stride_bytes, int src_h, int src_w, int top, int left,
                       float* out, int H, int W, float maxcode);

/* Training against the raw source's planes (additive to ABI 9; csrc/yuv.hip; definition: DESIGN section 33; yuvio.plane_loss_reference is the
 * float64 restatement).  pred [B, 3, H, W] fp32, H and W even, NOT clamped; src = n_frames raw src_h x src_w frames in file layout; the window
 * at (top, left), both even.  coeffs is the STORE struct (m = to_yuv, scale = denom).  With a_p the store arithmetic before rounding,
 *   e_p = (a_p - code_p) / maxcode,  mse_p[b] = mean over plane p of e_p^2,  L[b] = sum_p w_p mse_p[b] (w = weights / sum(weights)),  L = mean_b L[b]
 *   frame_sel:  null -- sample b is compared against frame b (B <= n_frames); else B device floats, sample b against frame (int)frame_sel[b]
 *       clamped to [0, n_frames - 1] (the convention of bnerv_fetch_frame's sel_dev: a captured step on a resident clip hands over that word)
 *   grad (may be null):  accumulate == 0: grad = lambda * dL/dpred, loss[0] = lambda * L;  accumulate != 0: both are ADDED to what is there
 *   stats [B, 4] = {L[b], mse_y, mse_u, mse_v}, always written, never scaled by lambda
 * One streaming launch (per-wave partial sums to ws) plus a one-block finalize that adds them in a fixed order: the same operands give the same
 * bits.  Validates before any launch: null pointers, odd H / W / top / left, a window that leaves the frame, a stride smaller than a frame,
 * bytes_per_sample, negative weights or a zero weight sum, B > n_frames without frame_sel; BNERV_E_WS for a workspace below _ws_bytes.  fp32
 * operands need 4-byte, 16-bit samples 2-byte alignment; every wider access is chosen per address. */
size_t bnerv_yuv420_loss_ws_bytes(int B, int H, int W);
int bnerv_yuv420_loss(void* stream, const float* pred, int B, int H, int W, const void* src, int bytes_per_sample, size_t frame_stride_bytes,
                      int n_frames, int src_h, int src_w, int top, int left, const float* frame_sel, const bnerv_yuv_coeffs* coeffs,
                      const float* weights, float lambda, float* grad, int accumulate, float* loss, float* stats, void* ws, size_t ws_bytes);

/* The MS-SSIM-Y term of training against the raw source (additive to ABI 9; csrc/yuv.hip; definition: DESIGN section 37; yuvio.luma_pre_reference
 * is the float64 restatement).  Two streaming launches around bnerv_loss_fwd_bwd at C = 1 with (c_l1, c_l2, c_ms, c_fft) = (0, 0, 1, 0):
 *   bnerv_yuv_luma_pair:  pred [B, 3, H, W] fp32, NOT clamped, and the H x W luma window at (top, left), any parity, of raw frames (src, n_frames,
 *       frame_sel: as bnerv_yuv420_loss; coeffs: the STORE struct) -> yp_out [B, 1, H, W] = (off[0] + scale[0] (m[0] R + m[1] G + m[2] B)) / maxcode, the
 *       luma code before rounding over the peak, and ys_out [B, 1, H, W] = float(code) / maxcode, the bits of bnerv_yuv_luma_f32.
 *   bnerv_luma_grad_rgb:  gy [B, 1, H, W] = dL/dyp -> grad [B, 3, H, W]: accumulate == 0: grad[b, c] = (lambda k[c]) gy, loss[0] = lambda * loss_term[0];
 *       accumulate != 0: grad[b, c] = fma(lambda k[c], gy, grad[b, c]), loss[0] = fma(lambda, loss_term[0], loss[0]).  k[c] = scale[0] m[c] / maxcode
 *       in float64 (the host's); loss_term and loss are device words.  gy and grad both null: the loss word alone.
 * Both validate before any launch (null pointers, bytes_per_sample, a window that leaves the frame, a stride smaller than a frame, B > n_frames
 * without frame_sel); fp32 operands need 4-byte alignment, every wider access is chosen per address.  No LDS, barriers or atomics. */
int bnerv_yuv_luma_pair(void* stream, const float* pred, int B, int H, int W, const void* src, int bytes_per_sample, size_t frame_stride_bytes,
                        int n_frames, int src_h, int src_w, int top, int left, const float* frame_sel, const bnerv_yuv_coeffs* coeffs,
                        float* yp_out, float* ys_out);
int bnerv_luma_grad_rgb(void* stream, const float* gy, int B, int H, int W, const double* k, float lambda, float* grad, int accumulate,
                        const float* loss_term, float* loss);

/* ------------------------------------------------------------------------------------------------------------------
 * GEMM-shaped dense work on v_mfma_f32_16x16x4_f32 (csrc/gemm.hip).
 *
 * Dense layers applied to many rows (B >= 16: the token MLPs of E-NeRV's transformer stem, NeRV_MLP at larger batches;
 * reference model_blocks.py:66-71, model_enerv.py:22-60) -- same arguments as one group of bnerv_dense_grouped_*:
 *   fwd: y [B,O] = act(x [B,I] w[O,I]^T + b), aux [B,O] = cos(pre) for BNERV_ACT_SIN (may be NULL)
 *   bwd: dw [O,I], db [O] (may be NULL), dx [B,I] (may be NULL) from dy [B,O]; y (relu) / aux (sin) as the activation needs. */
int bnerv_dense_gemm_fwd(void* stream, const float* x, const float* w, const float* b, float* y, float* aux, int B, int I, int O, int act);
size_t bnerv_dense_gemm_bwd_ws_bytes(int B, int I, int O);      /* 0 for small B; row-split partial weight gradients otherwise */
int bnerv_dense_gemm_bwd(void* stream, const float* x, const float* w, const float* y, const float* aux, const float* dy,
                         float* dx, float* dw, float* db, void* ws, size_t ws_bytes, int B, int I, int O, int act);

/* Pointwise MLP of the ConvNeXt encoder block (reference model_blocks.py:245-258, channels_last form:
 *   x = pwconv2(gelu(pwconv1(x))); x = gamma * x; return input + x ) on NCHW tensors, C in {16, 32, 48, 64}:
 *   fwd: out [B,C,HW] = inp + gamma * (w2 [C,4C] gelu(w1 [4C,C] x + b1) + b2);  hsave [B,4C,HW] (may be NULL) keeps w1 x + b1
 *   bwd: from h1 (= hsave) and dout: dx [B,C,HW] = d loss / d x, and the two pixel-contraction operands of the weight gradients,
 *        gbuf = gelu(h1), dhbuf = d loss / d h1 ([B,4C,HW] each).  The weight / bias / gamma gradients follow from two
 *        bnerv_conv_wgrad (k = 1) calls: (x, dhbuf) -> dw1, db1 and (gbuf, dout) -> S, t with dw2 = gamma S, db2 = gamma t,
 *        dgamma = rowsum(w2 * S) + b2 * t.  (d loss / d inp is dout itself.) */
/* Alignment: w1 and w2 must be 16-byte aligned (BNERV_E_ARG otherwise: they are staged with 16-byte loads); every other operand: any fp32 pointer. */
int bnerv_cnx_mlp_fwd(void* stream, const float* x, const float* inp, const float* w1, const float* b1, const float* w2, const float* b2,
                      const float* gamma, float* out, float* hsave, int B, int C, int HW);
int bnerv_cnx_mlp_bwd(void* stream, const float* h1, const float* dout, const float* w1, const float* w2, const float* gamma,
                      float* dx, float* gbuf, float* dhbuf, int B, int C, int HW);
/* Host-only (no launch, no device): the launch the two calls above make for [B, C, HW] -- nt: 16-pixel tiles per wave item (1 or 2),
 * grid_blocks: blocks of four waves, items: wave items; wave w of block k takes items 4 k + w, + 4 grid_blocks, ...  (outputs may be
 * NULL).  BNERV_E_ARG for a C the kernels are not built for. */
int bnerv_cnx_mlp_plan(int B, int C, int HW, int* nt, int* grid_blocks, int* items);
/* the [C x 4C] bookkeeping of that backward in one launch: dw2 = gamma S, db2 = gamma t, dgamma = rowsum(w2 * S) + b2 * t */
int bnerv_cnx_param_grads(void* stream, const float* S, const float* t, const float* w2, const float* b2, const float* gamma,
                          float* dw2, float* db2, float* dgamma, int C);

/* ------------------------------------------------------------------------------------------------------------------
 * Range-ANS entropy coder of the compression report (HOST buffers; csrc/ans.cpp).  Replaces constriction's AnsCoder +
 * QuantizedGaussian / Categorical models behind `real_bitrate` (lib/entropy_model.py:46-62, :65-81; consumed at
 * train_nerv_compression.py:484-512, 560-577): rANS, 64-bit state, 32-bit words, 24-bit probabilities, symbols pushed in
 * reverse so that decoding yields them in message order.
 *   *_encode_*  returns the number of 32-bit words of the compressed message (also when out == NULL or cap_words is too small:
 *               nothing is written then), or -1 on a bad argument (bnerv_last_error()).
 *   *_decode_*  the inverse; BNERV_OK or an error code.
 *   gaussian:    integer symbols in [min_sym, max_sym] under the leaky quantised Gaussian(mean, std) on that support
 *   categorical: symbols 0 .. K-1 under probs[K] (any non-negative weights; normalised internally) */
long bnerv_ans_encode_gaussian(const int32_t* symbols, size_t n, int32_t min_sym, int32_t max_sym, double mean, double std, uint32_t* out, size_t cap_words);
int bnerv_ans_decode_gaussian(const uint32_t* words, size_t n_words, size_t n, int32_t min_sym, int32_t max_sym, double mean, double std, int32_t* symbols_out);
long bnerv_ans_encode_categorical(const int32_t* symbols, size_t n, const double* probs, int K, uint32_t* out, size_t cap_words);
int bnerv_ans_decode_categorical(const uint32_t* words, size_t n_words, size_t n, const double* probs, int K, int32_t* symbols_out);

/* ------------------------------------------------------------------------------------------------------------------
 * The same coder in independent runs (additive to ABI 9; csrc/ans.cpp on the host, csrc/rans.hip on the device;
 * boosting_nerv_amd/rstream.py).
 *
 * The n symbols of a record are cut into runs of `run` symbols (the last may be shorter).  Every run is a message of its own, coded from
 * an empty state under the record's one table: its bulk words in refill order, then its final state as EXACTLY two words (low, high; the
 * high word may be zero), so a decoder knows where the state lies without trying.  The messages of the runs lie back to back;
 * run_words[k] is the word count of run k (>= 2; <= 65535, which bounds `run`: 24 bits per symbol at most).
 *   bnerv_ans_gaussian_cdf          the max_sym - min_sym + 2 cumulative 24-bit slot counts of the quantised Gaussian (symbol i owns
 *                                   [cdf[i], cdf[i + 1])): the one table of the encoders, the host decoders and the device kernel.  Returns
 *                                   the entry count (also when out_cdf == NULL or cap is too small: nothing is written then), -1 on a bad model.
 *   bnerv_ans_encode_gaussian_runs  -> the total word count (also when out_words == NULL or cap_words is too small: no word is written
 *                                   then); out_run_words (may be NULL) takes ceil(n / run) counts either way; -1 on a bad argument.
 *   bnerv_ans_decode_gaussian_runs  the inverse, run by run, each from its own span of `words`: a run is valid when it consumes exactly its
 *                                   bulk words and ends with state 0; otherwise an error that names the run.  Never reads outside a run's span.
 *   bnerv_rans_dequant  (device)    ONE launch.  A block is one wave and serves up to 64 consecutive runs of ONE record: it stages that
 *                                   record's table (with a first-level table on the top 8 bits of a slot) and its runs' words in LDS, lane k decodes run blocks[b].run + k sequentially, and the
 *                                   wave writes  out[i] = float(lo + index) * scale (+ beta, when the item has one)  -- product and sum one
 *                                   fp32 operation each -- with consecutive lanes on consecutive elements.  `words`: the device copy of all
 *                                   runs back to back followed by two zero words (n_words counts them); `run_start`: n_runs + 1 device
 *                                   entries, the first word of every run and the end of the last; `blocks`, `items`, `tables` (all tables
 *                                   back to back, items[k].table = offset of its first entry): device arrays.  A run that does not consume
 *                                   exactly its words or does not end with state 0 sets bit 0 of *err (device int); a descriptor that
 *                                   points outside `words` or `tables` sets bit 1 and nothing of its block is decoded. */
#define BNERV_RANS_MAX_ALPHABET 4096
#define BNERV_RANS_MIN_RUN 64
#define BNERV_RANS_MAX_RUN 4096
typedef struct { unsigned item; unsigned run; unsigned first; unsigned _pad; } bnerv_rans_block;   /* run: global index of the block's first run; first: that run's index within its item */
typedef struct { float* out; float scale; float beta; int lo; unsigned n; unsigned table; unsigned alphabet; int has_beta; int _pad; } bnerv_rans_item;
long bnerv_ans_gaussian_cdf(int32_t min_sym, int32_t max_sym, double mean, double std, uint32_t* out_cdf, size_t cap);
long bnerv_ans_encode_gaussian_runs(const int32_t* symbols, size_t n, int32_t min_sym, int32_t max_sym, double mean, double std, int run,
                                    uint32_t* out_words, size_t cap_words, unsigned short* out_run_words);
int bnerv_ans_decode_gaussian_runs(const uint32_t* words, size_t n_words, const unsigned short* run_words, size_t n_runs, size_t n,
                                   int32_t min_sym, int32_t max_sym, double mean, double std, int run, int32_t* symbols_out);
int bnerv_rans_dequant(void* stream, const uint32_t* words, size_t n_words, const uint32_t* run_start, size_t n_runs,
                       const bnerv_rans_block* blocks, size_t n_blocks, const bnerv_rans_item* items, int n_items,
                       const uint32_t* tables, size_t n_table_words, int run, int* err);

/* ------------------------------------------------------------------------------------------------------------------
 * Runs under a table the file carries, and the device encoder (additive to ABI 9; csrc/ans.cpp on the host, csrc/ransenc.hip on the
 * device; boosting_nerv_amd/estream.py).
 *
 *   bnerv_ans_counts_cdf          the A + 1 cumulative 24-bit slot counts of a histogram of A symbols, integer arithmetic only:
 *                                 f[k] = 1 + floor((2^24 - A) * counts[k] / n), the slots lost to truncation one each to the symbols in
 *                                 order of decreasing count (index order on ties).  A pure function of the counts; strictly increasing,
 *                                 ends at 2^24.  Returns A + 1 (also when out_cdf == NULL or cap is too small), -1 on a bad histogram.
 *   bnerv_ans_encode_table_runs / bnerv_ans_decode_table_runs
 *                                 bnerv_ans_encode_gaussian_runs / _decode_gaussian_runs with an explicit cumulative table (A + 1 entries,
 *                                 strictly increasing from 0 to 2^24; symbol min_sym + i owns [cdf[i], cdf[i + 1])) in place of (mean, std).
 *   bnerv_sym_hist  (device)      ONE launch over `items`: counts[items[k].out + s - lo] = how often symbol s occurs in items[k].sym.
 *                                 `blocks`: n_blocks device pairs (item, first element); a block counts BNERV_HIST_SLICE elements from there
 *                                 in a private LDS histogram and adds it to `counts` (n_counts device dwords, zeroed by the caller).  A
 *                                 symbol outside [lo, lo + alphabet) sets bit 0 of *err and is not counted; a descriptor that points
 *                                 outside the arrays sets bit 1.
 *   bnerv_rans_encode  (device)   ONE launch.  Blocks as bnerv_rans_dequant's: one wave, up to 64 consecutive runs of ONE item, that item's
 *                                 table in LDS; lane k encodes run blocks[b].run + k from its last symbol to its first with the host
 *                                 coder's arithmetic.  Run g owns slot g of `slots`: slot_words = run * 24 / 32 + 3 dwords.  The run's
 *                                 message -- bulk words in refill order, state low, state high -- ends at the END of its slot, and
 *                                 run_words[g] is its length.  A symbol outside the table, or a word that would leave the slot, sets bit 0
 *                                 of *err, and the lane writes nothing more (run_words[g] = 0); a bad descriptor sets bit 1.
 *   bnerv_rans_compact (device)   copies[j] = (slot, destination word, word count): the last `count` words of slot `slot` go to
 *                                 out[dst .. dst + count).  A copy that points outside `slots` or `out` sets bit 1 of *err and is skipped. */
#define BNERV_HIST_SLICE 16384
typedef struct { const int* sym; unsigned n; int lo; unsigned alphabet; unsigned out; } bnerv_hist_item;      /* out: first entry in `counts` */
typedef struct { const int* sym; unsigned n; int lo; unsigned alphabet; unsigned table; } bnerv_renc_item;     /* table: first entry in `tables` */
typedef struct { unsigned slot; unsigned dst; unsigned count; unsigned _pad; } bnerv_rans_copy;
long bnerv_ans_counts_cdf(const uint32_t* counts, int A, uint32_t* out_cdf, size_t cap);
long bnerv_ans_encode_table_runs(const int32_t* symbols, size_t n, int32_t min_sym, const uint32_t* cdf, int A, int run,
                                 uint32_t* out_words, size_t cap_words, unsigned short* out_run_words);
int bnerv_ans_decode_table_runs(const uint32_t* words, size_t n_words, const unsigned short* run_words, size_t n_runs, size_t n,
                                int32_t min_sym, const uint32_t* cdf, int A, int run, int32_t* symbols_out);
int bnerv_sym_hist(void* stream, const bnerv_hist_item* items, int n_items, const uint32_t* blocks, size_t n_blocks, uint32_t* counts, size_t n_counts, int* err);
int bnerv_rans_encode(void* stream, const bnerv_rans_block* blocks, size_t n_blocks, const bnerv_renc_item* items, int n_items,
                      const uint32_t* tables, size_t n_table_words, int run, uint32_t* slots, size_t n_slots, unsigned short* run_words, int* err);
int bnerv_rans_compact(void* stream, const uint32_t* slots, size_t n_slots, int slot_words, const bnerv_rans_copy* copies, size_t n_copies,
                       uint32_t* out, size_t n_out, int* err);

/* ------------------------------------------------------------------------------------------------------------------
 * Wide runs: records whose symbols span more than 4096 values (additive to ABI 9; csrc/ans.cpp on the host, csrc/ransw.hip on the
 * device; boosting_nerv_amd/wstream.py).
 *
 * A record on [min_sym, max_sym] has a `shift` k in 0..16 and B = ceil((max_sym - min_sym + 1) / 2^k) buckets.  A symbol v is coded as
 * v - min_sym = (bucket << k) | low: the bucket under a cumulative table of B entries, `low` as k raw bits in the same state under the
 * implicit uniform table (left = low << (24 - k), prob = 1 << (24 - k)).  The encoder pushes low, then the bucket; the decoder pops the
 * bucket, refills, pops low ( q = state & (2^24 - 1); low = q >> (24 - k); state = ((state >> 24) << (24 - k)) | (q & (2^(24-k) - 1)) ),
 * refills.  A run takes at most run * (24 + k) / 32 + 3 words.  With k = 0 the words are those of bnerv_ans_encode_table_runs.
 *   bnerv_ans_gaussian_bucket_cdf   bnerv_ans_gaussian_cdf over the buckets: B + 1 entries, bucket j from min_sym + j * 2^shift - 0.5 (the last
 *                                   one ends at max_sym + 0.5).  With shift 0 it is bnerv_ans_gaussian_cdf entry for entry.
 *   bnerv_ans_encode_wide_runs / bnerv_ans_decode_wide_runs
 *                                   bnerv_ans_encode_table_runs / _decode_table_runs with the range, the table over its B buckets and the
 *                                   shift.  Decode also fails a run in which a value of the last bucket lies above max_sym.
 *   bnerv_sym_hist_wide  (device)   bnerv_sym_hist over buckets: counts[items[k].at + ((s - lo) >> shift)].  A symbol outside [lo, lo + span_m1]
 *                                   sets bit 0 of *err and is not counted.
 *   bnerv_rans_encode_wide (device) bnerv_rans_encode with the extra push per symbol.  Every run owns `slot_words` dwords of `slots` (one
 *                                   stride for the launch: at least run * (24 + shift) / 32 + 3 of every item) and may fill the last
 *                                   run * (24 + shift) / 32 + 3 of them; a symbol outside the range, or a word past that, sets bit 0 of *err and
 *                                   ends the lane's stores (run_words[g] = 0).  bnerv_rans_compact gathers the slots as it does the narrow ones.
 *   bnerv_rans_dequant_wide (device) bnerv_rans_dequant with the raw-bits step per symbol:  out[i] = float(lo + offset) * scale (+ beta).  An offset
 *                                   above span_m1 sets bit 0 of *err and is clamped to span_m1. */
#define BNERV_RANSW_MAX_SHIFT 16
typedef struct { const int* sym; unsigned n; int lo; unsigned alphabet; unsigned at; unsigned shift; unsigned span_m1; } bnerv_wsym_item;   /* alphabet: B; at: first entry in `counts` / `tables`; span_m1: max_sym - min_sym */
typedef struct { float* out; float scale; float beta; int lo; unsigned n; unsigned table; unsigned alphabet; int has_beta; unsigned shift; unsigned span_m1; unsigned _pad; } bnerv_ransw_item;
long bnerv_ans_gaussian_bucket_cdf(int32_t min_sym, int32_t max_sym, int shift, double mean, double std, uint32_t* out_cdf, size_t cap);
long bnerv_ans_encode_wide_runs(const int32_t* symbols, size_t n, int32_t min_sym, int32_t max_sym, const uint32_t* cdf, int B, int shift, int run,
                                uint32_t* out_words, size_t cap_words, unsigned short* out_run_words);
int bnerv_ans_decode_wide_runs(const uint32_t* words, size_t n_words, const unsigned short* run_words, size_t n_runs, size_t n,
                               int32_t min_sym, int32_t max_sym, const uint32_t* cdf, int B, int shift, int run, int32_t* symbols_out);
int bnerv_sym_hist_wide(void* stream, const bnerv_wsym_item* items, int n_items, const uint32_t* blocks, size_t n_blocks, uint32_t* counts, size_t n_counts, int* err);
int bnerv_rans_encode_wide(void* stream, const bnerv_rans_block* blocks, size_t n_blocks, const bnerv_wsym_item* items, int n_items,
                           const uint32_t* tables, size_t n_table_words, int run, uint32_t* slots, size_t n_slots, int slot_words, unsigned short* run_words, int* err);
int bnerv_rans_dequant_wide(void* stream, const uint32_t* words, size_t n_words, const uint32_t* run_start, size_t n_runs,
                            const bnerv_rans_block* blocks, size_t n_blocks, const bnerv_ransw_item* items, int n_items,
                            const uint32_t* tables, size_t n_table_words, int run, int* err);

/* ------------------------------------------------------------------------------------------------------------------
 * Temporal CEM file: inter-coded frame embeddings (additive to ABI 9; csrc/ranst.hip and csrc/ransw.hip;
 * boosting_nerv_amd/tstream.py).  All three are device entry points of ONE launch each.
 *
 *   bnerv_embed_delta    q: n_frames rows of P int32 symbols, q_pitch elements apart.  d[t][p] = q[t][p] - q[t-1][p] for t >= 1 (row 0 of d is
 *                        not written), rows d_pitch apart, and stats[t] over row t of d (stats[0] stays zero).  The entry point zeroes
 *                        `stats` on the stream; min and max are kept as order-preserving keys for which zero is neutral:
 *                            max d = (int)(max_key ^ 0x80000000),   min d = (int)(~min_key_inv ^ 0x80000000);
 *                        s1 = sum d (exact: |s1| < 2^63), s2 = sum d^2 mod 2^64 (exact while P * max d^2 < 2^64).  Integer atomics only: the
 *                        result does not depend on the order of arrival.  Any 4-byte alignment of q and d, any pitch >= P.
 *   bnerv_rans_decode_wide   bnerv_rans_dequant_wide with an int32 store:  ((int*)items[k].out)[i] = lo + offset;  scale, beta and has_beta
 *                        of the item are not read.  The same kernel body, the same error bits.
 *   bnerv_embed_chain_dequant   sym: n_frames rows of P int32, sym_pitch apart.  q_0 = sym_0;  q_t = pred[t] ? q_{t-1} + sym_t : sym_t  (pred[0] is
 *                        not read as a prediction: callers refuse a file that sets it);  out[t][p] = float(q_t) * scale[t] + beta[t], product
 *                        and sum one fp32 operation each, rows out_pitch apart.  pred / scale / beta: n_frames device entries.  The chain is
 *                        summed in 64 bits: a q_t outside int32 sets bit 0 of *err (device int) and is clamped.  A thread walks t with
 *                        BNERV_CHAIN_UNROLL loads in flight; a block serves BNERV_CHAIN_SEG frames, starting from the nearest frame at or
 *                        before them that is not predicted. */
#define BNERV_CHAIN_UNROLL 8
#define BNERV_CHAIN_SEG 64
typedef struct { unsigned max_key; unsigned min_key_inv; long long s1; unsigned long long s2; } bnerv_delta_stats;
int bnerv_embed_delta(void* stream, const int32_t* q, size_t q_pitch, int n_frames, size_t P, int32_t* d, size_t d_pitch, bnerv_delta_stats* stats);
int bnerv_rans_decode_wide(void* stream, const uint32_t* words, size_t n_words, const uint32_t* run_start, size_t n_runs,
                           const bnerv_rans_block* blocks, size_t n_blocks, const bnerv_ransw_item* items, int n_items,
                           const uint32_t* tables, size_t n_table_words, int run, int* err);
int bnerv_embed_chain_dequant(void* stream, const int32_t* sym, size_t sym_pitch, const unsigned char* pred, const float* scale, const float* beta,
                              int n_frames, size_t P, float* out, size_t out_pitch, int* err);

/* ------------------------------------------------------------------------------------------------------------------
 * Huffman coder of the post-hoc quantised model (additive to ABI 9; csrc/huff.cpp on the host, csrc/huff.hip on the device;
 * boosting_nerv_amd/qstream.py).
 *
 * The code is given by BNERV_HUFF_LEAVES code lengths, one byte each: symbols 0..255, then the EOF leaf (never written); length 0 = unused,
 * at most 32, Kraft equality over the used leaves.  Codes are canonical: leaves ordered by (length, leaf index), the first code of the
 * shortest length is 0, code(next leaf) = (code + 1) << (its length - the previous length).  A code's bits go into the bit string most
 * significant first; bit p of the string is bit 31 - (p % 32) of 32-bit word p / 32.
 * The symbols of item k (counts[k] of them, items back to back in `symbols`) are cut into runs of R = BNERV_HUFF_RUN symbols (the last run
 * of an item may be shorter; a run never spans two items); the bit string is continuous over runs and items, padded with zero bits to
 * the final word only.  run_bits[r] is the bit length of run r (<= 32 R, so it fits 16 bits).
 *   bnerv_huff_encode   (host)  -> the number of 32-bit words of the bit string, also when words_out == NULL or cap_words is too small
 *                       (nothing is written then); -1 on a bad argument (a symbol without a code, bad lengths, cap_runs too small).
 *   bnerv_huff_decode   (host)  the inverse, run by run from the recorded lengths.  An error -- never a read past `words` -- when a run
 *                       does not end on its recorded bit, a bit pattern has no code or decodes to EOF, or the lengths do not add up to n_words.
 *   bnerv_huff_dequant  (device) ONE launch: one lane decodes one run sequentially into LDS (first-level lookup table of 2^BNERV_HUFF_LUT_BITS
 *                       entries, canonical search of <= 32 steps for longer codes), a wave then writes
 *                           out[i] = float(min[s]) + float(scale[s]) * float(q[i]),   s = (i / (red * inner)) * inner + i % inner
 *                       for its 64 runs with coalesced stores; the product and the sum are each ONE IEEE fp32 operation.  `words`: n_words
 *                       device words of which the last two are zero padding (every payload read is clamped to them); `runs`: n_runs + 1
 *                       device descriptors, the last one a sentinel holding the total bit count; `items`: n_items device entries.  A lane
 *                       whose run does not end on the next descriptor's start bit (or that meets EOF) sets bit 0 of *err (device int). */
#define BNERV_HUFF_RUN 256
#define BNERV_HUFF_LEAVES 257
#define BNERV_HUFF_LUT_BITS 12
#define BNERV_HUFF_F32 0
#define BNERV_HUFF_F16 1
typedef struct { unsigned long long start_bit; unsigned item; unsigned first; } bnerv_huff_run;      /* first: index of the run's first element in its item */
typedef struct { float* out; const void* min; const void* scale; int dtype; unsigned n; unsigned red; unsigned inner; } bnerv_huff_item;
long bnerv_huff_encode(const unsigned char* symbols, const unsigned* counts, int n_items, const unsigned char* lengths, int R,
                       uint32_t* words_out, size_t cap_words, unsigned short* run_bits_out, size_t cap_runs);
int bnerv_huff_decode(const uint32_t* words, size_t n_words, const unsigned short* run_bits, size_t n_runs, const unsigned* counts, int n_items,
                      const unsigned char* lengths, int R, unsigned char* symbols_out);
int bnerv_huff_dequant(void* stream, const uint32_t* words, size_t n_words, const bnerv_huff_run* runs, size_t n_runs,
                       const bnerv_huff_item* items, int n_items, const unsigned char* lengths_host, int R, int* err);

/* ------------------------------------------------------------------------------------------------------------------
 * Temporal post-hoc file: inter-coded frame embeddings under Huffman codes of their own (additive to ABI 9; csrc/hufft.hip and
 * csrc/huff.hip; boosting_nerv_amd/pstream.py).  All three are device entry points of ONE launch each; every sum is an
 * integer, so no result depends on the order in which blocks arrive.
 *
 *   bnerv_embed_delta_u8   q: n_frames rows of P uint8 codes, q_pitch bytes apart, at any byte alignment.  d[t][p] = (q[t][p] - q[t-1][p]) mod 256
 *                        for t >= 1 (row 0 of d is not written), rows d_pitch apart, and hist[t][0][s] = the number of p with q[t][p] == s,
 *                        hist[t][1][s] = the number with d[t][p] == s (hist[0][1] stays zero).  The entry point zeroes `hist`
 *                        (n_frames * 2 * 256 uint32) on the stream.  A thread owns 16 consecutive bytes of a row and takes each of its three
 *                        accesses as wide as that address allows; a block counts in LDS and adds its non-zero bins with one integer atomic each.
 *   bnerv_huff_decode_u8   bnerv_huff_dequant with a byte store:  items[k].out[i] = q[i], the symbols a run holds; the same kernel body, the
 *                        same descriptors of runs, the same error bit.  Rows may start at any byte.
 *   bnerv_embed_chain_dequant_u8   sym: n_frames rows of P uint8, sym_pitch apart.  q_0 = sym_0;  q_t = pred[t] ? (q_{t-1} + sym_t) mod 256 : sym_t
 *                        (pred[0] is not read as a prediction: callers refuse a file that sets it);
 *                            out[t][p] = float(min[s]) + float(scale[s]) * float(q_t[p]),   s = (i / (red * inner)) * inner + i % inner,  i = t * P + p,
 *                        product and sum one fp32 operation each, rows out_pitch floats apart; min / scale: device arrays of
 *                        n_frames * P / red entries of `dtype` (BNERV_HUFF_F32 | BNERV_HUFF_F16).  A block serves BNERV_CHAIN_SEG frames,
 *                        starting from the nearest frame at or before them that is not predicted.  Nothing can leave its range: there is
 *                        no error word. */
typedef struct { unsigned char* out; unsigned n; } bnerv_huff_item_u8;
int bnerv_embed_delta_u8(void* stream, const unsigned char* q, size_t q_pitch, int n_frames, size_t P, unsigned char* d, size_t d_pitch, uint32_t* hist);
int bnerv_huff_decode_u8(void* stream, const uint32_t* words, size_t n_words, const bnerv_huff_run* runs, size_t n_runs,
                         const bnerv_huff_item_u8* items, int n_items, const unsigned char* lengths_host, int R, int* err);
int bnerv_embed_chain_dequant_u8(void* stream, const unsigned char* sym, size_t sym_pitch, const unsigned char* pred, const void* min, const void* scale,
                                 int dtype, unsigned red, unsigned inner, int n_frames, size_t P, float* out, size_t out_pitch);

/* ------------------------------------------------------------------------------------------------------------------
 * Huffman coder of the SPARSE post-hoc quantised model (additive to ABI 9; csrc/huffz.cpp on the host, csrc/huffz.hip on the device;
 * boosting_nerv_amd/zstream.py).  Bit order, canonical codes, descriptors and item table are those of the coder above.
 *
 * The alphabet has BNERV_HUFFZ_LEAVES leaves: 0..255 the 8-bit code of a kept element, BNERV_HUFFZ_ZERO + k (k = 0..8) 2^k consecutive
 * zero elements, then the EOF leaf (never written).  An element is a zero when its `keep` byte is 0; its symbol byte is ignored by the
 * encoder and written as 0 by the decoder.  The ELEMENTS of item k are cut into runs of R <= BNERV_HUFF_RUN (the last run of an item may be
 * shorter); a stretch of zeros is clipped at the ends of its run.  A stretch of z zeros is written as z leaves BNERV_HUFFZ_ZERO under
 * parse BNERV_HUFFZ_SINGLE and as the leaves BNERV_HUFFZ_ZERO + k of the set bits of z, highest first, under BNERV_HUFFZ_RUNS; a decoder
 * needs no case for the parse.  A run holds at most R leaves, so run_bits[r] fits 16 bits.
 *   bnerv_huffz_encode  (host)  as bnerv_huff_encode: the word count also when words_out == NULL or cap_words is too small; -1 on a bad argument.
 *   bnerv_huffz_decode  (host)  -> symbols_out and keep_out (one byte each per element).  An error -- never a read past `words` -- when a
 *                       run does not end on its recorded bit, a bit pattern has no code or decodes to EOF, a zero-run leaf would carry the
 *                       run past its element count, or the lengths do not add up to n_words.
 *   bnerv_huffz_dequant (device) ONE launch, arguments as bnerv_huff_dequant (R = BNERV_HUFF_RUN):
 *                           out[i] = keep[i] ? float(min[s]) + float(scale[s]) * float(q[i]) : +0.0f
 *                       A lane decodes until it has produced the element count of its run (from the descriptors); every leaf produces
 *                       at least one element.  A leaf that would overrun the run, an EOF, or a run that does not end on the next
 *                       descriptor's start bit sets bit 0 of *err. */
#define BNERV_HUFFZ_LEAVES 266
#define BNERV_HUFFZ_ZERO 256
#define BNERV_HUFFZ_ZERO_LEAVES 9
#define BNERV_HUFFZ_SINGLE 0
#define BNERV_HUFFZ_RUNS 1
long bnerv_huffz_encode(const unsigned char* symbols, const unsigned char* keep, const unsigned* counts, int n_items, const unsigned char* lengths,
                        int parse, int R, uint32_t* words_out, size_t cap_words, unsigned short* run_bits_out, size_t cap_runs);
int bnerv_huffz_decode(const uint32_t* words, size_t n_words, const unsigned short* run_bits, size_t n_runs, const unsigned* counts, int n_items,
                       const unsigned char* lengths, int R, unsigned char* symbols_out, unsigned char* keep_out);
int bnerv_huffz_dequant(void* stream, const uint32_t* words, size_t n_words, const bnerv_huff_run* runs, size_t n_runs,
                        const bnerv_huff_item* items, int n_items, const unsigned char* lengths_host, int R, int* err);

/* ------------------------------------------------------------------------------------------------------------------
 * Depthwise KxK convolution (K odd <= 7, stride 1, padding K/2) of the ConvNeXt encoder block of HNeRV_Boost
 * (model_blocks.py:223-247: nn.Conv2d(dim, dim, 7, padding=3, groups=dim)); first kernels of SURVEY 8(f) row N3.
 *   bnerv_dwconv_fwd(flip=0): y = conv(x, w) + bias;   flip=1: the data gradient (taps flipped, bias ignored: pass g as x)
 *   bnerv_dwconv_wgrad: dwb[C][K*K+1] = weight gradient rows with the bias gradient in the last column (slabs in ws;
 *   defer_ctx != NULL queues the slab reduction there, see bnerv_reduce_slabs_deferred).  x, y, g: [B, C, H, W];  w: [C, 1, K, K]. */
/* Alignment: 16-byte stores to y when y is 16-byte aligned and W % 4 == 0, scalar stores (same bits) otherwise; x, w, bias: any fp32 pointer. */
int bnerv_dwconv_fwd(void* stream, const float* x, const float* w, const float* bias, float* y, int B, int C, int H, int W, int K, int flip);
size_t bnerv_dwconv_wgrad_ws_bytes(int B, int C, int H, int W, int K);
int bnerv_dwconv_wgrad(void* stream, const float* x, const float* g, float* dwb, void* ws, size_t ws_bytes, int B, int C, int H, int W, int K, bnerv_ctx* defer_ctx);
/* Host-only (no launch, no device): how bnerv_dwconv_wgrad splits the rows of 16 x 64 tiles of a plane -- `groups` blocks per tile column,
 * each summing rows_per_group tile rows in registers (the last group may hold fewer).  Outputs may be NULL. */
int bnerv_dwconv_wgrad_plan(int B, int C, int H, int W, int* groups, int* rows_per_group);

/* ------------------------------------------------------------------------------------------------------------------
 * Loss and metrics.  Replaces loss_fn (hnerv_utils.py:335-397; every variant) including its autograd backward, and
 * psnr_fn_single (hnerv_utils.py:400-403).
 *   loss_b = c_l1 * mean|d| + c_l2 * mean d^2 + c_ms * (1 - ms_ssim_b) + c_ss * (1 - ssim_b)
 *            + c_fft * mean|FFT2(pred)-FFT2(target)|_{re,im}
 * with d = pred - target; the reported loss is mean_b loss_b (batch_average=True) and `grad` = d(loss)/d(pred).
 *   bnerv_loss_fwd_bwd (c_ss = 0):
 *     L1: c_l1=1   L2: c_l2=1   L1_freq: c_l1=60,c_fft=1   Fusion7: c_l1=.3,c_l2=.7   Fusion8: c_l1=.5,c_l2=.5
 *     Fusion10/11/12: c_l1=.7/.9/.8,c_ms=.3/.1/.2   Fusion10_freq: c_l1=42,c_ms=18,c_fft=1
 *   bnerv_loss_ssim_fwd_bwd (c_ms = 0, c_ss = its c_ssim argument):
 *     SSIM: c_ss=1   Fusion1/3/5: c_l2=.3/.5/.7,c_ss=.7/.5/.3   Fusion2/4/6/9: c_l1=.3/.5/.7/.9,c_ss=.7/.5/.3/.1
 *     L1_ssim_freq: c_l1=42,c_ss=18,c_fft=1
 * MS-SSIM and SSIM follow pytorch_msssim 0.2.1 (win 11, sigma 1.5; 5 levels / one level, ssim_b = mean over channels and valid window
 * positions of lum * cs, no relu) -- third-party, PARITY UNPINNED.  MS-SSIM needs min(H, W) > 160, SSIM min(H, W) >= 11.
 * The 2-D DFT is a mixed-radix LDS FFT; H and W may have any prime factors <= BNERV_FFT_MAX_RADIX.
 * (bnerv_loss_ssim_fwd_bwd, whose frames may be as small as 11 x 11: <= 37, its own kernel instantiations).  A side may be 1 or 2.
 * A row (20 W bytes: line, twiddle and position tables) and four columns (40 H bytes) must fit the 160 KB of LDS of a block NEXT TO the static LDS
 * of every kernel of the entry point that may run that transform; the entry reads those sizes from the loaded code object.  As built: W <= 8117
 * (1488 static bytes in the merged head launch) and H <= 4094 (48 in the merged column launch) for bnerv_loss_fwd_bwd, whatever its coefficients;
 * W <= 6553 (this path keeps its rows below 128 KB) and H <= 4095 for bnerv_loss_ssim_fwd_bwd.  A larger frame with c_fft != 0 is BNERV_E_ARG, before
 * anything is launched; bnerv_fft_prepare / bnerv_loss_ssim_prepare check the prime factors only.
 * stats_out: [B, BNERV_LOSS_STATS] = {loss_b, sum|d|, sum d^2, ms_ssim_b (bnerv_loss_ssim_fwd_bwd: ssim_b), psnr_b (hnerv_utils.py:400-403)};
 * loss_out: [1].
 * ------------------------------------------------------------------------------------------------------------------ */
#define BNERV_FFT_MAX_RADIX 31
#define BNERV_MSSSIM_LEVELS 5

typedef struct {
    const float* pred;    /* [B, C, H, W] */
    const float* target;  /* [B, C, H, W] */
    float* grad;          /* [B, C, H, W] written (may be NULL: value only) */
    float* loss_out;      /* [1] */
    float* stats_out;     /* [B, BNERV_LOSS_STATS] */
    void* ws;
    size_t ws_bytes;
    int B, C, H, W;
    float c_l1, c_l2, c_ms, c_fft;
} bnerv_loss_desc;

size_t bnerv_loss_ws_bytes(int B, int C, int H, int W, int use_ms, int use_fft);
/* Build the read-only FFT twiddle tables for H x W frames ahead of time.  Tables are otherwise built on first use,
 * which allocates and copies synchronously -- not allowed while `stream` is being captured into a hipGraph. */
int bnerv_fft_prepare(int H, int W);
/* Alignment: pred, target and grad may sit at any 4-byte boundary (the MS-SSIM pyramid takes 8-byte loads only when pred and target are
 * 8-byte aligned, same bits either way); ws must be 8-byte aligned (float2 spectra; BNERV_E_ARG otherwise); the same holds for bnerv_loss_ssim_fwd_bwd. */
int bnerv_loss_fwd_bwd(void* stream, const bnerv_loss_desc* d);
/* per-sample MS-SSIM only (evaluate(): msssim_fn_single, hnerv_utils.py:410-412); out [B] */
int bnerv_msssim(void* stream, const float* x, const float* y, float* out, void* ws, size_t ws_bytes, int B, int C, int H, int W);
/* The single-scale SSIM losses (an additive entry of ABI 9): the descriptor of bnerv_loss_fwd_bwd with c_ms == 0, plus c_ssim != 0.  Level 0
 * only, no pyramid: two launches per value + gradient call, five with a spectral term.  grad == NULL: value and stats only.
 * ws: bnerv_loss_ssim_ws_bytes(B, C, H, W, c_fft != 0).  bnerv_loss_ssim_prepare(H, W) is this path's bnerv_fft_prepare (prime factors
 * <= 37): call it before a capture when c_fft != 0.  bnerv_fft_prepare itself keeps the BNERV_FFT_MAX_RADIX limit. */
size_t bnerv_loss_ssim_ws_bytes(int B, int C, int H, int W, int use_fft);
int bnerv_loss_ssim_prepare(int H, int W);
int bnerv_loss_ssim_fwd_bwd(void* stream, const bnerv_loss_desc* d, float c_ssim);
/* per-sample SSIM only (ssim(x, y, data_range=1, size_average=False)); out [B], the bits of stats_out column 3 above;
 * ws: bnerv_loss_ssim_ws_bytes(B, C, H, W, 0) */
int bnerv_ssim(void* stream, const float* x, const float* y, float* out, void* ws, size_t ws_bytes, int B, int C, int H, int W);
/* (ABI 9) The output head's tanh-gradient as a tensor: gt = g * 0.5 (1 - (2 img - 1)^2), the derivative of OutImg's tanh(v) * 0.5 + 0.5
 * (reference model_blocks.py:57-63) applied to the incoming gradient -- what the IN_TANHGRAD prologue computes on the fly -- with the
 * per-block channel sums of gt in part [B * bnerv_tanh_grad_blocks(HW)][C] (sum over the first index = the head's bias gradient:
 * bnerv_reduce_slabs(part, B * blocks, C, db)).  Used by the 3x3 head of HNeRV_Boost (model_hnerv.py:214), whose weight gradient runs
 * with input and gradient swapped (38 input channels on the MFMA M side). */
/* Alignment: the 16-byte form needs g, img, gt 16-byte aligned and HW % 4 == 0; otherwise the scalar form runs (same gt; no refusal). */
int bnerv_tanh_grad_blocks(int HW);
int bnerv_tanh_grad(void* stream, const float* g, const float* img, float* gt, float* part, int B, int C, int HW);

/* Inpainting (additive to ABI 9; csrc/eltwise.hip): the reference masks both sides of the loss with an [H, W] mask that depends on the frame
 * size only (hnerv_utils.py:59-84 TransformInput; train_nerv_all.py:343 loss_fn(out * mask, gt * mask)).  Streaming passes over [B, C, HW]
 * fp32 with the mask [HW] broadcast over B and C; every product is ONE fp32 multiply, so a loss entry point called on (pred_m, gt_m) sees
 * the bits torch's `x * mask` would hand it.
 *   bnerv_inpaint_head:  gt_m = img * mask;  inp (may be NULL) = clamp(img * mask, 0, 1), the frame an image-consuming model reads
 *   bnerv_inpaint_pred:  pred_m = pred * mask, and per-block sums of (pred - gt)^2 against the UNMASKED gt as doubles in ws
 *                        (bnerv_inpaint_ws_bytes(B, C, HW) bytes)
 *   bnerv_inpaint_psnr:  psnr[b * stride] = -10 log10(mean_{CHW}(pred - gt)^2 + 1e-9) from that ws, partials added in one fixed order --
 *                        the PSNR the reference logs (train_nerv_all.py:350).  A launch of its own so that it can follow the loss call and
 *                        land in column 4 of its stats (stride = BNERV_LOSS_STATS), which the loss computes on masked data
 *   bnerv_inpaint_grad:  g *= mask in place (the backward of pred * mask)
 * Alignment: any 4-byte boundary and any HW; the 16-byte form runs when HW % 4 == 0 and every tensor is 16-byte aligned, the scalar form
 * otherwise (same bits; no refusal).  ws must be 8-byte aligned. */
int bnerv_inpaint_head(void* stream, const float* img, const float* mask, float* inp, float* gt_m, int B, int C, int HW);
size_t bnerv_inpaint_ws_bytes(int B, int C, int HW);
int bnerv_inpaint_pred(void* stream, const float* pred, const float* gt, const float* mask, float* pred_m, void* ws, size_t ws_bytes, int B, int C, int HW);
int bnerv_inpaint_psnr(void* stream, const void* ws, size_t ws_bytes, float* psnr, int stride, int B, int C, int HW);
int bnerv_inpaint_grad(void* stream, float* g, const float* mask, int B, int C, int HW);

/* psnr[b] = -10 log10(mean_{CHW}(out-gt)^2 + 1e-9)  (hnerv_utils.py:400-403); ws: bnerv_psnr_ws_bytes() */
size_t bnerv_psnr_ws_bytes(int B, int C, int H, int W);
int bnerv_psnr(void* stream, const float* out, const float* gt, float* psnr, void* ws, size_t ws_bytes, int B, int C, int H, int W);

/* Paired launch (ABI 5): the data gradient of a 3x3 convolution with at most 12 channels on both sides (plain input; epilogues
 * EP_DGELU_SAVED / EP_DSIN / EP_PLAIN) and a weight gradient of the same image size that does not depend on it, in ONE grid.  Inside
 * the backward of ResBlock_SFT / NeRVBlock (model_blocks.py:83-89, :34-39) autograd computes, for each of the three convolutions, the
 * weight gradient and the input gradient from the SAME incoming gradient: (dW1 | d conv1), (dW0 | d conv0), (dW_block | d block conv);
 * issued as two launches each half leaves most of the chip idle through its prologue and tail (one tile per block at 180x320).
 * Both descriptors are exactly those bnerv_conv_wgrad / bnerv_conv_igemm would take (same workspaces; the weight gradient must be
 * deferred -- defer_finish with a context -- and both must name the same context).  Returns BNERV_OK when the pair was launched, 1 when
 * this pair is not one the launch takes (issue the two calls separately, weight gradient first), negative BNERV_E_* on error. */
int bnerv_conv_wgrad_pair(void* stream, const bnerv_conv_desc* conv, const bnerv_wgrad_desc* wgrad);
/* The form bnerv_conv_wgrad_pair(conv, wgrad) launches (host query, additive to ABI 9), BNERV_PAIR_NONE where it returns 1 or an error;
 * *conv_rows (may be NULL): the rows the conv half of that form writes into conv->partial ([R][B][2][Cout], sums epilogues), 0 for NONE.
 * The launch refuses (returns 1) a form whose rows differ from bnerv_conv_partial_rows(conv), which sized the caller's buffer; the query
 * reports NONE there.  A form that declines late for want of scratch (BF16_WIDE) lets the launch go on to a later form. */
#define BNERV_PAIR_NONE (-1)
#define BNERV_PAIR_STEM 0               /* form 0: the stem stage's weight and data gradient (csrc/stem.hip) */
#define BNERV_PAIR_Q4_LEAN 1            /* form 1: the <= 12-channel conv next to the lean weight gradient (interleaved, shared-tile or fold) */
#define BNERV_PAIR_SMALL_WIDE 2         /* form 2: the low-resolution conv (4x16 tiles) next to a wide weight gradient */
#define BNERV_PAIR_BF16_WIDE 3          /* form 3: the wide split conv next to the wide split weight gradient */
#define BNERV_PAIR_HEAD 4               /* form H: the 1x1 output head's backward as one streaming pass */
int bnerv_conv_wgrad_pair_form(const bnerv_conv_desc* conv, const bnerv_wgrad_desc* wgrad, int* conv_rows);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused multi-tensor Adan step.  Replaces Adan.step -> _multi_tensor_adan (optimizer.py:125-235, :296-362), i.e. the
 * slot the reference reserves for the external `fused_adan` extension (optimizer.py:365-395).
 * Per tensor: p, g, exp_avg, exp_avg_sq, exp_avg_diff, neg_pre_grad (all n floats).  `first_step` != 0 makes
 * neg_pre_grad := -g before the update (optimizer.py:190-192).  Scalars are those computed at optimizer.py:171-173,
 * :208-226.  lr is read from DEVICE memory (lr_dev[0]) so a captured hipGraph replays with a changing schedule.
 * ------------------------------------------------------------------------------------------------------------------ */
#define BNERV_ADAN_MAX_TENSORS 48
typedef struct {
    float* p[BNERV_ADAN_MAX_TENSORS];
    const float* g[BNERV_ADAN_MAX_TENSORS];
    float* exp_avg[BNERV_ADAN_MAX_TENSORS];
    float* exp_avg_sq[BNERV_ADAN_MAX_TENSORS];
    float* exp_avg_diff[BNERV_ADAN_MAX_TENSORS];
    float* neg_pre_grad[BNERV_ADAN_MAX_TENSORS];
    int n[BNERV_ADAN_MAX_TENSORS];
    int n_tensors;
} bnerv_adan_chunk;

typedef struct {
    float beta1, beta2, beta3;
    float eps, weight_decay;
    float clip_global_grad_norm;
    int no_prox;
    /* bias corrections depend on the step count; like lr they are read from device memory:
       sched_dev = {lr, bias_correction1, bias_correction2, sqrt(bias_correction3), first_step(0/1)} */
    const float* sched_dev;
} bnerv_adan_hyper;

int bnerv_adan_multi_tensor(void* stream, const bnerv_adan_chunk* chunk, const bnerv_adan_hyper* h);

/* Table form of the same step (ABI 5): the descriptors of ALL tensors live in DEVICE memory, so one launch serves any number of
 * tensors (the chunk form passes 48 descriptors by value: C1's 186 tensors were four dependent launches per step).  The caller
 * fills the table on the host -- entry i owns blocks [bstart, bstart + bnerv_adan_table_blocks(n)) of the grid, bstart = running
 * sum -- and uploads it once; it stays valid while the tensors keep their addresses.  Same arithmetic, same order. */
typedef struct {
    float* p;
    const float* g;
    float* exp_avg;
    float* exp_avg_sq;
    float* exp_avg_diff;
    float* neg_pre_grad;
    int n;
    int bstart;
} bnerv_adan_entry;
int bnerv_adan_table_blocks(int n);
int bnerv_adan_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, const bnerv_adan_hyper* h);

/* Fused Adam, table form (additive to ABI 9): torch.optim.Adam with its defaults (no weight decay, no amsgrad), one launch over the same
 * device table as bnerv_adan_table (exp_avg_diff / neg_pre_grad are not read).  Of `h`: beta1, beta2, eps and
 * sched_dev = {lr, bias_correction1, sqrt(bias_correction2), 1 - beta1, 1 - beta2} in device memory (the complements rounded from float64):
 *   m += (1 - b1)(g - m);  v = b2 v + (1 - b2) g^2;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps) */
int bnerv_adam_table_blocks(int n);
int bnerv_adam_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, const bnerv_adan_hyper* h);

/* Global-norm gradient clip on the device (additive to ABI 9): torch.nn.utils.clip_grad_norm_(params, max_norm) with its defaults
 * (train_nerv_all.py:346-347 of the reference) over the gradients of the same device table, with no host round trip, so a captured step can hold it:
 *   total = sqrt(sum g^2);  coef = min(1, max_norm / (total + 1e-6));  g *= coef  (also when coef == 1)
 * Of an entry only g, n and bstart are read; the grid is the optimizer launch's (bnerv_adan_table_blocks).  bnerv_grad_sqsum_table leaves one
 * double per block in partials[0 .. total_blocks); bnerv_grad_scale_table has every block add partials[0 .. n_partials) in one fixed order
 * (n_partials >= total_blocks: several tables -- parameter groups -- may have written consecutive ranges of one workspace and are then clipped
 * by their common norm), forms coef in fp32, scales its slice in place, and block 0 writes out[0] = total, out[1] = coef.  No atomics: the same
 * build and launch sequence gives the same bits.  max_norm travels by value (fixed for a run).
 * Alignment: a gradient may start at any 4-byte boundary and n need not be a multiple of 4 (16-byte accesses over the aligned body only);
 * partials must be 8-byte aligned. */
int bnerv_grad_sqsum_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, double* partials);
int bnerv_grad_scale_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, const double* partials,
                           int n_partials, float max_norm, float* out);

/* Frame fetch of a step whose clip is resident in device memory (train_nerv_all.py:329 moves one frame host -> device per step; with
 * the clip in HBM the step only needs to know WHICH frame): copies frame k = (int)sel_dev[0] of clip [N][frame_elems] to dst_img
 * and norm[k] (fp64, hnerv_utils.py:47) to dst_norm.  sel_dev is device memory, so a captured step replays with a moving index. */
/* Alignment: clip and dst_img must be 16-byte aligned and, for n_frames > 1, frame_elems % 4 == 0 (every frame on the 16-byte grid):
 * BNERV_E_ARG otherwise -- a clip with an odd frame size is refused, not copied element-wise. */
int bnerv_fetch_frame(void* stream, const float* clip, const double* norms, const float* sel_dev, int n_frames, size_t frame_elems,
                      float* dst_img, double* dst_norm);

/* flat-bucket helpers for the data-parallel gradient exchange (replaces DDP's bucket copy, train_nerv_all.py:254):
 * gather `n_tensors` gradients into one contiguous bucket scaled by `scale`, and scatter it back. */
typedef struct {
    float* t[BNERV_ADAN_MAX_TENSORS * 2];
    int n[BNERV_ADAN_MAX_TENSORS * 2];
    int off[BNERV_ADAN_MAX_TENSORS * 2];
    int n_tensors;
} bnerv_bucket_chunk;
int bnerv_bucket_gather(void* stream, const bnerv_bucket_chunk* c, float* bucket, float scale);
int bnerv_bucket_scatter(void* stream, const bnerv_bucket_chunk* c, const float* bucket, float scale);

/* ------------------------------------------------------------------------------------------------------------------
 * Global magnitude pruning (additive to ABI 9; csrc/prune.hip, boosting_nerv_amd/prune.py).
 * A table of fp32 tensors (`items`, device memory) is walked by blocks of 256 threads; `blocks` holds n_blocks device pairs
 * (item, first element) and a block owns BNERV_PRUNE_SLICE elements of its item from there -- the layout of bnerv_sym_hist.  A tensor may
 * start at any 4-byte boundary, a mask at any byte (16-byte accesses over the aligned body of x only); an item has fewer than 2^31 elements,
 * a table fewer than 2^32.
 *
 *   bnerv_kth_abs      tau = the k-th smallest |x| over ALL items (1-based, 1 <= k <= total, exact): a most-significant-digit radix select on
 *                      key = bits(x) & 0x7fffffff, BNERV_KTH_PASSES digits of 8 bits.  A fixed launch sequence -- one memset, then per digit
 *                      one histogram launch over `blocks` and one single-block launch that finds the bin holding the remaining rank and
 *                      narrows the prefix -- with the select state in the context's scratch: no host round trip, no launch that depends on
 *                      the data, integer arithmetic only (the same table and k give the same bits on every device and in every run).
 *                      out (device, 4 dwords, 8-byte aligned): out[0] = bits of tau, out[1] = flags (bit 0: a NaN was seen -- it ranks
 *                      above +inf; bit 1: k exceeds the element count; bit 2: a descriptor points outside the uploaded arrays),
 *                      out[2..3] = 64-bit count of elements with |x| <= tau.  The mask pointers of the items are not read.
 *                      Needs a context (BNERV_E_ARG without one, or when its scratch would have to grow inside a stream capture).
 *   bnerv_prune_masks  mask[i] = |x[i]| > tau (1 / 0, key compare: a NaN is kept), x[i] *= mask[i]; tau_dev = out of bnerv_kth_abs.
 *   bnerv_mask_mul     x[i] *= mask[i] over the table.
 *   bnerv_grad_mask_table  g *= mask over the GRADIENTS of the optimizer's device table (of an entry g, n and bstart are read; the grid is
 *                      the optimizer launch's): masks_dev[t] is the mask of entry t, NULL for a tensor that is not pruned.  The per-step
 *                      launch of a masked train step, in front of the clip and the update. */
#define BNERV_PRUNE_SLICE 16384
#define BNERV_KTH_PASSES 4
typedef struct { float* x; unsigned char* mask; unsigned n; unsigned _pad; } bnerv_prune_item;
int bnerv_kth_abs(bnerv_ctx* ctx, void* stream, const bnerv_prune_item* items, int n_items, const uint32_t* blocks, size_t n_blocks,
                  unsigned long long k, uint32_t* out);
int bnerv_prune_masks(void* stream, const bnerv_prune_item* items, int n_items, const uint32_t* blocks, size_t n_blocks, const uint32_t* tau_dev);
int bnerv_mask_mul(void* stream, const bnerv_prune_item* items, int n_items, const uint32_t* blocks, size_t n_blocks);
int bnerv_grad_mask_table(void* stream, const bnerv_adan_entry* table_dev, int n_tensors, int total_blocks, const unsigned char* const* masks_dev);

/* ------------------------------------------------------------------------------------------------------------------
 * Interpolation file (additive to ABI 9; csrc/interp.hip): the frame embeddings a file does not store, derived from
 * those it stores.  out [N, P] from src [S, P] under plan_dev (device memory, N entries, hnerv_utils.interp_plan): row t of out is
 *   ia == ib   src[ia]                                               (a stored frame, or a derived one with a stored frame on one side only)
 *   w == 0.5f  0.5f * (src[ia] + src[ib])                            (the reference's expression, model_hnerv.py:82, :237)
 *   otherwise  (1.0f - w) * src[ia] + w * src[ib], both products and the sum rounded to fp32 on their own (no fused contraction)
 * -- the same bits as hnerv_utils.embed_expand_reference.  The caller validates the plan (0 <= ia, ib < S, 0 <= w < 1) before it uploads
 * it; a row whose entry names a row outside src is left unwritten.  One streaming launch, grid (ceil(P / 1024), N): N <= 65535.
 * Alignment: any 4-byte boundary and any P; the 16-byte form runs when P % 4 == 0 and src and out are 16-byte aligned (every row then is),
 * the scalar form otherwise (same bits; no refusal).  src and out must not overlap.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct { int ia, ib; float w; } bnerv_interp_entry;
int bnerv_embed_expand(void* stream, const float* src, const bnerv_interp_entry* plan_dev, float* out, int S, int N, int P);

/* ------------------------------------------------------------------------------------------------------------------
 * Frame resize (additive to ABI 9; csrc/resize.hip): the separable antialiased bicubic of boosting_nerv_amd/resize.py,
 * one axis per launch.  Every output sample is  acc = fp32(acc + fp32(w_j * x_j))  over its taps in ascending j from 0.0f, the product
 * and the sum rounded on their own (no fused contraction) -- the bits of resize.resize_reference.
 *
 * table_dev (device memory, 4-byte aligned, (2 + 2 T) n_out words; resize.axis_table makes it, resize.pack_table lays it out):
 *   int32 first[n_out] | int32 count[n_out] | fp32 weights[n_out][T] | fp32 weights transposed [T][n_out]
 * Output sample i reads input first[i] .. first[i] + count[i] - 1 of its axis; 1 <= T <= BNERV_RESIZE_MAX_TAPS.  The caller validates the
 * table before it uploads it; a kernel clamps what it reads of it (first, count) to the axis, so a bad table cannot become a wild read.
 *
 *   bnerv_resize_rows  x [rows, n_in] -> out [rows, n_out] along the last axis.  A block stages the input span of BNERV_RESIZE_STRIP
 *                      output columns for a group of rows in LDS (coalesced reads whatever the scale; 16-byte loads when n_in % 4 == 0 and
 *                      x is 16-byte aligned), taps are LDS reads.  `span` is the LDS pitch of a row in floats: a multiple of 4, at least
 *                      max over strips of (first[last] + count[last] - (first[first of strip] & ~3)) (resize.strip_span); the rows per
 *                      block are sized from it here (16, or 4 when 16 rows of `span` floats exceed 48 KiB; 4 rows of the largest span a
 *                      table of <= 64 taps can have always fit).
 *   bnerv_resize_cols  x [planes, n_in, width] -> out [planes, n_out, width] along the middle axis: consecutive lanes take consecutive
 *                      columns, every tap row is a coalesced read; 16-byte loads and stores when width % 4 == 0 and x and out are 16-byte
 *                      aligned, the scalar form otherwise (same bits).  clamp != 0: the result is clamped to [0, 1].
 * x and out: any 4-byte boundary, no overlap.  No atomics, no workspace; rows <= 2^27, planes <= 65535, n_out <= 262140 (cols).
 * ------------------------------------------------------------------------------------------------------------------ */
#define BNERV_RESIZE_MAX_TAPS 64
#define BNERV_RESIZE_STRIP 64
int bnerv_resize_rows(void* stream, const float* x, float* out, const void* table_dev, long long rows, int n_in, int n_out, int T, int span);
int bnerv_resize_cols(void* stream, const float* x, float* out, const void* table_dev, int planes, int n_in, int n_out, int width, int T, int clamp);

/* ------------------------------------------------------------------------------------------------------------------
 * Vertical resize fused with the raw 4:2:0 store (additive to ABI 9; csrc/upyuv.hip): the second launch of a decoder
 * that up-samples to the master's size and writes raw video.
 *
 *   bnerv_resize_cols_yuv420  x [B * 3, n_in, W] fp32 (what bnerv_resize_rows wrote for B RGB frames) and the table of n_in -> H (layout
 *                             above) -> out: B raw frames in file layout (planes Y [H, W], U, V [H/2, W/2]), frame b at byte
 *                             b * frame_stride_bytes -- the bytes of bnerv_rgb_to_yuv420 on the frame bnerv_resize_cols (clamp = 1) gives:
 *                             every value is that kernel's tap sum, clamped to [0, 1], then the store's matrix, [1 2 1] / 4 chroma filter,
 *                             mean of the row pair and floor(offset + scale * v + 0.5).  The full-size fp32 frame is never written.
 * Any table within BNERV_RESIZE_MAX_TAPS: up, down or identity; first and count are clamped to the axis.  H and W even; B <= 65535.
 * x and the table: any 4-byte boundary (16-byte loads where a strip's address allows, element by element otherwise); out: any address at
 * 1 byte per sample, an even address and frame stride at 2.  No LDS, no atomics, no workspace; nothing is allocated or synchronised.
 * ------------------------------------------------------------------------------------------------------------------ */
int bnerv_resize_cols_yuv420(void* stream, const float* x, const void* table_dev, int B, int n_in, int H, int W, int T, void* out,
                             int bytes_per_sample, size_t frame_stride_bytes, const bnerv_yuv_coeffs* coeffs);

/* ------------------------------------------------------------------------------------------------------------------
 * The plane loss at the master's size for a prediction below it (additive to ABI 9; csrc/upyuvloss.hip, DESIGN section 42;
 * yuvio.plane_loss_up_reference is the float64 restatement):  L_up(P) = L(U P)  with L, mse_p, weights, lambda and stats those of
 * bnerv_yuv420_loss and U the two-pass table filter above WITHOUT its clamp (Q[c] = Wc P[c] Wr^T), and the exact adjoint
 * dL_up/dP = Wc^T (dL/dQ) Wr.  pred [B, 3, h, w] fp32, not clamped, any h and w; the H x W window (both even) at (top, left), both even,
 * of the raw src_h x src_w frames.
 *
 *   _fwd  bnerv_resize_rows (pred -> S [B*3, h, W] in ws; table_w_dev of w -> W, T_w, span_w as that call takes them), then one launch that
 *         forms bnerv_resize_cols_yuv420's tap sums (table_h_dev of h -> H, T_h), does not clamp them, takes the errors against the source
 *         (src, bytes_per_sample, frame_stride_bytes, n_frames, frame_sel, coeffs = the STORE struct, weights: as bnerv_yuv420_loss) and
 *         writes per-wave partial sums and, with need_grad != 0, the error planes 2 w_p d_p e_p / (B m n_p) into ws; then the one-block
 *         finalize: stats [B, 4] = {L[b], mse_y, mse_u, mse_v} (never scaled), loss[0] = lambda * L, or += with accumulate != 0.
 *   _bwd  (after a _fwd with need_grad != 0 on the same ws) two launches: the adjoint of the column pass over adj_h_dev, the ADJOINT table of
 *         h -> H (resize.adjoint_table: for every input row the contiguous range of output rows that read it and their weights, in the
 *         table layout above with n_in entries; Ta_h its width), chroma carried at half width; then the adjoint of the row pass with the
 *         colour mix over adj_w_dev / Ta_w, span_a the LDS pitch in floats (resize.strip_span of the adjoint table; a multiple of 4, three
 *         rows of it within 48 KiB).  grad [B, 3, h, w] = lambda * dL_up/dP, or += with accumulate != 0.
 * ws: _ws_bytes(B, h, w, H, W) bytes = S (12 B h W) + error planes (6 B H W) + the column adjoint's output (8 B h W) + partials, every part
 * rounded up to 16 bytes; no [B, 3, H, W] buffer exists.  Validates before any launch and without a device: null pointers, odd H / W / top /
 * left or source size, a window that leaves the frame, a stride smaller than a frame, bytes_per_sample, tap counts outside 1 ..
 * BNERV_RESIZE_MAX_TAPS, weights, B > n_frames without frame_sel, B > 21845; BNERV_E_WS for a short workspace.  fp32 operands and tables need
 * 4-byte alignment; every wider access is chosen per address.  Table entries are clamped to the axis and the LDS pitch where they are read.
 * No float atomics: the same operands give the same bits.  Nothing is allocated or synchronised.
 * ------------------------------------------------------------------------------------------------------------------ */
size_t bnerv_yuv420_up_loss_ws_bytes(int B, int h, int w, int H, int W);
int bnerv_yuv420_up_loss_fwd(void* stream, const float* pred, int B, int h, int w, int H, int W, const void* table_w_dev, int T_w, int span_w,
                             const void* table_h_dev, int T_h, const void* src, int bytes_per_sample, size_t frame_stride_bytes, int n_frames,
                             int src_h, int src_w, int top, int left, const float* frame_sel, const bnerv_yuv_coeffs* coeffs, const float* weights,
                             float lambda, int need_grad, int accumulate, float* loss, float* stats, void* ws, size_t ws_bytes);
int bnerv_yuv420_up_loss_bwd(void* stream, int B, int h, int w, int H, int W, const void* adj_h_dev, int Ta_h, const void* adj_w_dev, int Ta_w,
                             int span_a, const bnerv_yuv_coeffs* coeffs, float lambda, float* grad, int accumulate, void* ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* BNERV_H */
