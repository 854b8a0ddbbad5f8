/* imagdressing_hip.h -- C ABI of libimagdressing_hip.so (MI355X / gfx950 only).
 *
 * The drop-in boundary of the IMAGDressing-v1 denoising hot path.  The reference is pure Python
 * on this path (its device code is whatever torch dispatches to), so the "FFI" a maintainer binds
 * is ctypes: see INTEGRATION.md for the stub.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - All pointers are DEVICE pointers into HBM unless stated otherwise; 16-bit tensors (bf16 or fp16, chosen
 *     per call by `dtype`) are passed as uint16_t*.  Inputs are borrowed and must stay alive until the stream work completes.
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); kernels are only
 *     enqueued, never synchronised; no allocation happens inside any call (hipGraph-capturable).
 *   - Return value: 0 on success, non-zero on error; imd_last_error() returns the message
 *     (thread-local).  There is NO CPU fallback: argument/shape/arch errors are reported, never
 *     papered over.
 *   - Activations are NHWC / token-major ([B, H*W, C]) bf16; weights are [N][K] bf16 with
 *     k = (ky*3 + kx) * Cin + ci for 3x3 convolutions.
 *   - ABI v8: the first field of every parameter block is `struct_bytes` = sizeof(the struct) as the CALLER compiled it.  An
 *     entry point that receives any other value returns an error instead of reading fields the caller never wrote (the v7 blocks
 *     grew at the tail; a binding that mirrored an older header handed the library a truncated struct).  Zero-initialise the
 *     block, set struct_bytes, then fill what you need: every optional pointer is NULL-off.
 */
#ifndef IMAGDRESSING_HIP_H
#define IMAGDRESSING_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMD_ABI_VERSION 9

enum { IMD_ACT_NONE = 0, IMD_ACT_SILU = 1, IMD_ACT_GEGLU = 2, IMD_ACT_GELU = 3, IMD_ACT_QUICK_GELU = 4 /* x * sigmoid(1.702 x): CLIP text MLP */ };
enum { IMD_OUT_ROWMAJOR = 0, IMD_OUT_HEADS = 1 };
/* 16-bit element type of activations and weights (both run v_mfma_f32_32x32x16_* at the same rate) */
enum { IMD_DTYPE_BF16 = 0, IMD_DTYPE_F16 = 1 };

/* destination of one split (Q, K or V) of a head-split projection */
typedef struct imd_heads_dest {
    uint16_t* ptr; /* NULL: drop this split */
    int kind;      /* 0: [B, H, L, DP] (rows = tokens)   1: [B, H, DP, L] (rows = head dim, keys contiguous) */
    int DP;        /* kind 0: padded head dim (row length)   kind 1: rows per head */
    int L;         /* kind 0: tokens per batch entry         kind 1: padded token count (row length) */
    float scale;   /* multiplied in fp32 before rounding (softmax scale * log2 e folded into Q) */
} imd_heads_dest;

/* Per-call tuning (ABI v8; tag widened in v9): `flags` of imd_conv_gemm_params / imd_attn_params is an INPUT.  0 (what a zero-initialised
 * block carries) = use the process-wide knobs of imd_set_tuning().  A caller whose flags carry the 8-bit tag IMD_TUNING_PER_CALL in bits
 * 24..31 -- (flags & IMD_TUNING_TAG_MASK) == IMD_TUNING_PER_CALL -- chooses for THIS call only:
 *   imd_conv_gemm:  bits 0..4 = bits 0..4 of tuning knob 2 (tap-inner K order, weight loads past L1, XCD-aware tile order, grouped order)
 *   imd_attention:  bits 0..7 = head-dim-40 kernel variant (tuning knob 0; 0 = the process-wide value; validated against the same range
 *                   as imd_set_tuning(0, .) of this build), bit 8 = 1: plain work order (tuning knob 1 = 0)
 * so two pipelines in one process can run different settings without touching global state (imagdressing_amd.ops.tuning_scope).  Any
 * other non-zero value in bits 24..31 is refused (v9): a block whose flags were left uninitialised does not silently select a tuning.
 * The fp8 attention, row-resident projection and fused feed-forward entry points have no per-call choice and ignore the field. */
#define IMD_TUNING_PER_CALL 0x5A000000
#define IMD_TUNING_TAG_MASK 0xFF000000u

typedef struct imd_conv_gemm_params {
    uint32_t struct_bytes; /* sizeof(imd_conv_gemm_params) in the caller's view (ABI v8); checked on entry */
    const uint16_t* x; /* NHWC activations (pixel stride x_pix_stride) or [M, K] rows */
    const uint16_t* w; /* [N][K] */
    void* out;         /* bf16 (fp32 when out_f32) [M, out_ld] */
    int M, N, K;
    int Cin, taps, Hin, Win, Hout, Wout, stride, ups;
    int x_pix_stride;
    int out_ld, res_ld;
    const float* bias;   /* [N] or NULL */
    const float* rowvec; /* per-batch vector [B][rowvec_stride] added to every pixel of batch b, or NULL */
    int rowvec_stride;   /* floats between the vectors of consecutive batch entries; 0 = ONE vector for the whole batch (a shared timestep) */
    const uint16_t* res; /* residual [M, res_ld] or NULL */
    float out_scale;     /* applied after bias/rowvec, before the residual add */
    int act;             /* IMD_ACT_* */
    int out_f32;
    int mode;            /* IMD_OUT_* */
    int hC, hH, hD;      /* head split: channels per split, heads, head dim */
    imd_heads_dest hd[3];
    int dtype;           /* IMD_DTYPE_* */
    int split_k;         /* K slices (<= 1: none); > 1 needs splitk_ws and a row-major epilogue */
    float* splitk_ws;    /* split_k * M * N floats of scratch */
    uint32_t x_bytes, w_bytes; /* filled in by the library (buffer-descriptor extents) */
    int flags;           /* filled in by the library (tuning bits); on entry: 0, or IMD_TUNING_PER_CALL | per-call tuning bits (see above) */
    /* fused GroupNorm(+SiLU) prologue (cfg 5 only): x is normalised as x*gn_a[b][c] + gn_b[b][c] (then SiLU when
     * gn_silu) while it is staged; coefficients come from imd_groupnorm_coeffs().  NULL: plain convolution. */
    const float* gn_a;
    const float* gn_b;
    int gn_silu;
    int pad_br_only;     /* 3x3 taps: 0 = symmetric zero padding 1 (UNet); 1 = padding on the bottom / right edge only, i.e.
                          * F.pad(x, (0, 1, 0, 1)) + conv(padding = 0): the stride-2 Downsample2D of the VAE encoder */
    int* splitk_counters; /* split_k > 1 only.  NULL: the K slices are summed by a second launch (fixed order).  Otherwise >=
                          * IMD_SPLITK_COUNTERS ints that are ZERO on entry and are left zero: every output tile's last-arriving
                          * workgroup sums the slices itself, in the same fixed order (bit-identical results, one launch less) */
    /* GroupNorm statistics of the OUTPUT (row-major 16-bit output, N % gn_stats_groups == 0, >= 8 channels per group): the fp32 (sum, sum of
     * squares) per group of the FINAL (rounded) values, written to gn_stats_out[((b * nparts + part) * G + g) * 2].  Size the buffer with
     * nparts = imd_conv_gemm_stats_parts(p, cfg) -- NOT imd_conv_patch_stats_parts() -- because the layout depends on who writes it:
     *   - tile configs 5 / 22 / 23 / 29 with split_k == 1: the halo-patch kernel's own epilogue, part = (pixel tile of the image) * n_tiles +
     *     channel tile; groups outside a tile get zeros;
     *   - ANY K-sliced launch that finishes with the second launch (split_k > 1, splitk_counters == NULL): the finish launch, part = a block
     *     of consecutive pixels of image b (all channels), nparts = ceil(HW / rows per part).
     * imd_conv_gemm_stats_parts() answers 0 when this (p, cfg) cannot produce them; a launch that asks anyway is refused.  The next
     * imd_groupnorm on that tensor passes the buffer as `partial` with `nparts` and skips its statistics pass (ResnetBlock2D: conv1 -> norm2,
     * conv2 -> the next block's norm). */
    float* gn_stats_out;
    int gn_stats_groups;
    /* GroupNorm (+ SiLU) of the OUTPUT inside the finish launch of a K-sliced problem (ABI v9; imd_conv_gemm_gn_out_supported()): when
     * gn_out_gamma is given, `out` receives  act(GroupNorm_G(epilogue(sum of the K slices)))  instead of the epilogue's result -- the tensor
     * ResnetBlock2D.norm2 + nonlinearity would produce from conv1's output, which nothing else reads (diffusers-0.24 ResnetBlock2D.forward:
     * conv1 -> + temb -> norm2 -> SiLU -> conv2).  One workgroup owns all pixels of one (image, group), so the statistics are complete in
     * the launch: the un-normalised tensor never exists in memory and the separate imd_groupnorm launch disappears.  Statistics are those of
     * the value ROUNDED to the element type (what imd_groupnorm would read back), fp32, fixed summation order.  Needs split_k > 1 without
     * splitk_counters, a row-major 16-bit output without activation / GEGLU, N % groups == 0 with 4 | N / groups, and
     * Hout * Wout * (N / groups) <= 12288 (the 16x16 and 8x8 levels); gn_stats_out must be NULL (there is nothing left to normalise). */
    /* GroupNorm (+ SiLU) of the INPUT rows inside the row-resident projections (ABI v9; imd_row_linear_gn_in_supported(p, cfg); tile configs
     * 12 / 13 / 14): Transformer2DModel.norm -> proj_in as ONE launch -- the normalised tensor never exists in memory.  gn_in_partial holds the
     * (sum, sum of squares) partials of x exactly as imd_groupnorm takes them (`partial` + `nparts`: [B][gn_in_nparts][gn_in_groups][2], written by
     * the producer of x through gn_stats_out or by a statistics pass); every workgroup folds its image's partials in imd_groupnorm's order and
     * applies  y = x * (gamma rstd) + (beta - mean gamma rstd)  (+ SiLU) to its rows in registers, rounded to the element type -- bit-identical
     * to imd_groupnorm followed by the same projection.  Needs K = Cin = 320 / 640 / 1280, K % gn_in_groups == 0, gn_in_groups <= 64 and
     * Hout * Wout a multiple of the kernel's row block (128 / 128 / 64). */
    const float* gn_in_partial; /* NULL: off */
    const float* gn_in_gamma;   /* [K] */
    const float* gn_in_beta;    /* [K] */
    int gn_in_nparts, gn_in_groups, gn_in_silu;
    float gn_in_eps;
    const float* gn_out_gamma; /* [N] or NULL */
    const float* gn_out_beta;  /* [N] */
    float gn_out_eps;
    int gn_out_silu;
    int gn_out_groups;
    /* PERIODIC residual (ABI v9, the K = 320 row-resident projection -- tile config 12 -- only; any other kernel refuses a non-zero value):
     * `res` holds res_rows rows and output row m adds res[m % res_rows].  The first hybrid block of a CFG batch, whose block input is the same
     * for the cond and the uncond rows (one copy kept): attn1's out-projection and Transformer2DModel.proj_out add it to both halves without a
     * materialised torch.cat([x, x]).  Needs res_rows % 128 == 0 and M % res_rows == 0; 0 = one residual row per output row. */
    int res_rows;
} imd_conv_gemm_params;
#define IMD_SPLITK_COUNTERS 16384

/* Head dims of imd_attention: 40, 64, 80, 160 (attention.hip / attention_d40.hip: every field below) and 512 (attention_d512.hip, the VAE mid
 * block's single-head attention as one flash launch: DPK = DPV = 512, any B / H / N / L1, kv1_bdiv >= 1, out_ld >= H * 512, bf16 and fp16).
 * At head dim 512 the optional forms are REFUSED by name, without a launch: a second key set (k2 / v2t / scale2), causal, proj_w, out_dup,
 * phase2_out / phase2_rows and k_pad_one must all be NULL / 0. */
typedef struct imd_attn_params {
    uint32_t struct_bytes; /* sizeof(imd_attn_params) in the caller's view (ABI v8); checked on entry */
    const uint16_t* q;   /* [B, H, N, DPK], pre-scaled by D^-1/2 * log2(e) */
    const uint16_t* k1;  /* [B1, H, L1, DPK] */
    const uint16_t* v1t; /* [B1, H, DPV, L1P] */
    const uint16_t* k2;  /* optional second key/value set (garment tokens / IP tokens) or NULL */
    const uint16_t* v2t;
    const float* scale2; /* [B] weight of the second softmax branch per batch entry (0 => skipped) */
    uint16_t* out;       /* [B, N, out_ld] with head h at columns h*D .. */
    int B, H, N, D;
    int L1, L1P, kv1_bdiv; /* kv batch entry of batch b is b / kv1_bdiv */
    int L2, L2P, kv2_bdiv;
    int out_ld;
    int dtype;
    int flags;           /* filled in by the library (tuning bits); on entry: 0, or IMD_TUNING_PER_CALL | per-call tuning bits (see above) */
    int causal;          /* 1: query i attends keys 0..i of the first key set only (CLIP text encoder); needs k2 == NULL, D != 40 */
    int k_pad_one;       /* 1: the caller guarantees that pad column D of EVERY K row (k1 and k2) holds 1.0 (D < DPK only, i.e.
                          * D = 40: the slot through which the deferred row maximum enters the QK^T MFMA).  The kernels that
                          * stage K through registers write that 1 themselves (0 or 1 in memory are both fine); with the
                          * guarantee the d = 40 kernel may stage K / V^T by LDS-DMA, which cannot patch data in flight. */
    /* Fused out-projection (ABI v7; head dim 40 with H * D == 320 and N >= 512 only -- the UNet's 64x64-level blocks): when proj_w is
     * given the launch also computes  proj_out = proj_res + proj_b + out . proj_w^T  (Attention.to_out[0] + the block residual,
     * attention_processor.py:614-622), i.e. the hybrid block's third launch disappears.  `out` is still written (it is the hand-off
     * buffer between the heads of a row block: stored write-through, read back by the head that finishes last). */
    const uint16_t* proj_w;   /* NULL, or [H*D, H*D] row-major (out channel, in channel) */
    const float* proj_b;      /* [H*D] or NULL */
    const uint16_t* proj_res; /* [B, N, proj_res_ld] or NULL */
    uint16_t* proj_out;       /* [B, N, proj_out_ld] */
    int proj_res_ld, proj_out_ld;
    int* proj_counters;       /* >= B * ceil(N / 256) ints, ZERO on entry, left zero (one per batch entry and 256-row block) */
    /* Duplicated first-phase output (ABI v9; imd_attention_dup_supported(): head dim 40, N >= 512, k_pad_one, no causal mask, no fused
     * out-projection): when out_dup is given, softmax(Q K1^T) V1 of batch entry b -- rounded to the element type exactly as a row
     * WITHOUT a second key set stores it -- is also written to out_dup[b, :, :] (same out_ld).  For the first hybrid block of a CFG
     * batch, where the cond and uncond rows of an image still have identical Q / K / V: one launch over the B cond rows produces the
     * cond rows (`out`) and the uncond rows (`out_dup`), bit-identical to a 2B-row launch (RefSAttnProcessor2_0 with and without
     * sa_hidden_states on the same hidden states, attention_processor.py:589-612). */
    uint16_t* out_dup;
    /* Phase-split launch of the hybrid attention (ABI v9; imd_attention_phase_split_supported(): head dims 64 / 80 / 160, k2 given, no causal mask):
     * the two softmaxes of a row with a second key set are independent until their results are added, and at the 32x32 / 16x16 / 8x8 levels a
     * launch has too few workgroups to hide one row's 2 x L / 64 sequential key tiles.  With phase2_rows = R > 0 the rows [0, R) are the ones
     * whose scale2 is non-zero (the cond half of a CFG batch) and the grid grows to B + R batch entries: entry b < B runs the FIRST softmax of
     * row b only and stores it as a row without a second key set would; entry B + r runs the SECOND softmax of row r and stores
     * scale2[r] * softmax(Q K2^T) V2 as fp32 to phase2_out[r, :, :] ([R, N, H * D]); a second, elementwise launch then writes
     * out[r] = round(out[r] + phase2_out[r]) -- the same arithmetic as the one-workgroup form (first result rounded to the element type,
     * second added in fp32, rounded once): bit-identical, with every workgroup half as long and 1.5x as many of them. */
    float* phase2_out;   /* NULL: off */
    int phase2_rows;
} imd_attn_params;

/* Fused feed-forward of a transformer block on the 64x64 level (ff_fused.hip), C = 320, inner = 1280:
 *   out = x + b2 + W2 . geglu(W1 . LN(x) + b1)         (norm3 -> ff.net[0] GEGLU -> ff.net[2] -> + residual, ONE launch)
 * w1 / b1 / w2 are PACKED by the host (imagdressing_amd/ops.py::pack_ff_fused; layout documented there and in ff_fused.hip):
 *   w1 [80 blocks][32 rows][320]: block b holds inner channels 16 b .. 16 b + 15; row i is the value row (bit 3 of i clear)
 *      or the gate row (bit 3 set) of inner channel 16 b + (i & 7) + 8 (i >> 4); LayerNorm gamma folded in (W1 diag(gamma));
 *   b1 [80][32] fp32 in the same order, LayerNorm beta folded in (b1 + W1 beta);
 *   w2 [40 chunks][320 rows][32]: chunk c holds inner channels 32 c .. 32 c + 31 as two 16-groups whose members are stored in
 *      the order 0-3, 8-11, 4-7, 12-15 (the register order of the GEGLU outputs of a lane). */
typedef struct imd_ff_params {
    uint32_t struct_bytes; /* sizeof(imd_ff_params) in the caller's view (ABI v8); checked on entry */
    const uint16_t* x;   /* [M, x_ld] block input (un-normalised when ln) -- also the residual */
    const uint16_t* w1;
    const float* b1;
    const uint16_t* w2;
    const float* b2;     /* [C] */
    uint16_t* out;       /* [M, out_ld] */
    int M, C, inner;
    int x_ld, out_ld;
    int ln;              /* 1: LayerNorm without affine (eps = ln_eps) on every row of x first */
    float ln_eps;
    int dtype;
} imd_ff_params;

/* Text cross-attention of a transformer block on the 64x64 level as one launch (row_xattn.hip), C = 320, 8 heads of 40, L <= 96 keys:
 *   out = x + bo + Wo . concat_h( softmax(q_h Kt_h^T) Vt_h ),   q = (LN(x) . Wq'^T + bq') * q_scale
 *   (norm2 -> attn2.to_q -> attention over the text keys -> attn2.to_out[0] + bias + block residual; softmax in base 2: q_scale carries log2 e)
 * Operands are PACKED by the host (imagdressing_amd/ops.py::pack_text_xattn / pack_text_kv; layouts documented there and in row_xattn.hip):
 *   w  [11 chunks][64 rows][320]: chunks 0..5 = Wq' (LayerNorm gamma folded in) with every head padded to 48 rows (row 32 c + r of half
 *      r / 32 = head 4 (r / 32) + (32 c + r % 32) / 48, dim (32 c + r % 32) % 48; dims >= 40 are zero rows), chunks 6..10 = Wo with its input
 *      channels in the order of the kernel's O registers; the 16-byte pieces of chunk row r sit at position piece ^ ((r >> 1) & 7);
 *   bq [6][64] fp32 in the row order of chunks 0..5 (LayerNorm beta folded in), bo [320] fp32;
 *   kv [text_rows][4 chunks][40960 bytes]: chunk c = the K / V^T images of heads c and c + 4 (19200 bytes each) of one conditioning row. */
typedef struct imd_xattn_params {
    uint32_t struct_bytes; /* sizeof(imd_xattn_params) in the caller's view; checked on entry */
    const uint16_t* x;   /* [M, x_ld] the block's UN-normalised state -- also the residual */
    const uint16_t* w;
    const float* bq;
    const float* bo;
    const uint16_t* kv;
    uint16_t* out;       /* [M, out_ld] */
    int M, C, heads, L;  /* L: text keys per conditioning row (the images mask keys >= L) */
    int rows_per_image;  /* tokens per batch entry, a multiple of 128; image b = row / rows_per_image reads conditioning row b / kv_bdiv */
    int kv_bdiv, text_rows;
    int x_ld, out_ld;
    float q_scale;       /* head_dim^-1/2 * log2(e) */
    float ln_eps;
    int dtype;
} imd_xattn_params;

typedef struct imd_groupnorm_params {
    uint32_t struct_bytes; /* sizeof(imd_groupnorm_params) in the caller's view (ABI v8); checked on entry */
    const uint16_t* x; uint16_t* y; const float* gamma; const float* beta;
    float* partial;      /* workspace of imd_groupnorm_workspace_floats() floats */
    int B, HW, C, G, x_ld, y_ld;
    float eps;
    int silu;
    int dtype;
    int nparts;          /* 0: imd_groupnorm computes the statistics itself (two launches).  > 0: `partial` already holds
                          * [B][nparts][G][2] fp32 (sum, sum of squares) partials of x written by the PRODUCER of x -- the
                          * convolution epilogue, imd_conv_gemm_params.gn_stats_out -- and only the normalise pass is launched */
} imd_groupnorm_params;

typedef struct imd_layernorm_params {
    uint32_t struct_bytes; /* sizeof(imd_layernorm_params) in the caller's view (ABI v8); checked on entry */
    const uint16_t* x; uint16_t* y; const float* gamma; const float* beta;
    int rows, C, x_ld, y_ld;
    float eps;
    int dtype;
} imd_layernorm_params;

typedef struct imd_ddim_params {
    uint32_t struct_bytes; /* sizeof(imd_ddim_params) in the caller's view (ABI v8); checked on entry */
    float* z;             /* [B, HW, 4] fp32 latent state, updated in place */
    const float* eps;     /* [2B, HW, 4] fp32: rows [0,B) cond pass, [B,2B) uncond pass */
    uint16_t* x_next;     /* [2B, HW, 8] bf16 next UNet input (channels 4..7 = 0) or NULL */
    int B, HW;
    float guidance, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev;
    const float* mask;    /* [B, HW] inpaint mask or NULL */
    const float* z_img;   /* [B, HW, 4] */
    const float* noise;   /* [B, HW, 4] */
    float sqrt_a_next, sqrt_1m_a_next;
    int dtype;            /* element type of x_next */
    const float* coefs;   /* NULL, or DEVICE pointer to 6 fp32 {sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev, sqrt_a_next,
                           * sqrt_1m_a_next} read by the kernel INSTEAD of the host scalars above: lets one captured HIP graph of a
                           * denoising step serve every timestep (the host refreshes 24 bytes per step, stream-ordered) */
    const float* var_noise; /* NULL, or [B, HW, 4] fp32 standard-normal noise of the stochastic DDIM step (eta > 0, DDIMScheduler.step's
                           * `variance_noise`): z_prev += sigma * var_noise BEFORE the inpaint blend; the caller then passes
                           * sqrt_1m_a_prev = sqrt(1 - a_prev - sigma^2) (the direction coefficient of diffusers' step) */
    float sigma;          /* eta * sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)); read only with var_noise */
} imd_ddim_params;

/* One step of an affine sampler (imd_sampler_step) over the [B, HW, 4] latent, per element in fp32:
 *   e  = eps_u + g (eps_c - eps_u)                         g = guidance, or guidance_rows[row]
 *   m  = m_x z + m_e e                                     the quantity the sampler keeps a history of (x0 prediction, or e itself)
 *   z' = z_x z + z_m m + sum_{k < K} z_h[k] hist[k] + z_n noise
 *   z' = (1 - mask) (b_img z_img + b_noise blend_noise) + mask z'            (with mask)
 *   z <- z';  hist[store] <- m (store >= 0);  x_next[both CFG halves] <- 16-bit(in_scale z'), channels 4..7 = 0
 * DPM-Solver++ (1 / 2M), Euler, Euler-ancestral and PNDM/PLMS differ in the host-computed coefficients only
 * (imagdressing_amd/scheduler.py). */
#define IMD_SAMPLER_MAX_HISTORY 4
#define IMD_SAMPLER_COEFS 13     /* floats of the device coefficient block: m_x, m_e, z_x, z_m, z_h[4], z_n, b_img, b_noise, in_scale, store */
typedef struct imd_sampler_params {
    uint32_t struct_bytes; /* sizeof(imd_sampler_params) in the caller's view; checked on entry */
    float* z;             /* [B, HW, 4] fp32 latent state, updated in place */
    const float* eps;     /* [2B, HW, 4] fp32: rows [0,B) cond pass, [B,2B) uncond pass */
    uint16_t* x_next;     /* [2B, HW, 8] 16-bit next UNet input (channels 4..7 = 0) or NULL */
    float* hist;          /* [K][B HW 4] fp32, ONE contiguous buffer owned by the caller (NULL iff K == 0).  A slot may be read and
                           * overwritten by the same launch: every thread reads its element of each slot before it stores */
    int B, HW, K;         /* K: history slots, 0..IMD_SAMPLER_MAX_HISTORY */
    int dtype;            /* element type of x_next */
    float guidance;
    const float* guidance_rows; /* NULL, or DEVICE [B] fp32: the guidance scale of each latent row, read instead of `guidance` */
    float m_x, m_e, z_x, z_m;
    float z_h[4];         /* by PHYSICAL slot; a slot whose coefficient is 0 is not read */
    float z_n, b_img, b_noise, in_scale;
    int store;            /* physical slot that receives m, -1: none */
    const float* noise;   /* NULL, or [B, HW, 4] fp32 standard-normal noise of a stochastic step (scaled by z_n, added before the blend) */
    const float* mask;    /* NULL, or [B, HW] inpaint mask; then z_img and blend_noise [B, HW, 4] are required */
    const float* z_img;
    const float* blend_noise;
    const float* coefs;   /* NULL, or DEVICE pointer to IMD_SAMPLER_COEFS fp32 read by the kernel INSTEAD of m_x .. store above (store as
                           * a float holding the integer; a value outside -1..K-1 stores nothing): a captured HIP graph of a step then
                           * holds no pointer or scalar that changes between replays -- the host refreshes 52 bytes per step */
} imd_sampler_params;

/* One step of the UniPC multistep sampler (imd_unipc_step) over the [B, HW, 4] latent, per element in fp32:
 *   e  = eps_u + g (eps_c - eps_u)                         g = guidance, or guidance_rows[row]
 *   m  = m_x z + m_e e                                     the x0 prediction made at this position
 *   s' = s_x z + s_m m + sum_{k < K} s_h[k] hist[k]        the corrected sample (UniC), the library's last_sample; no corrector: s_x = 1, rest 0
 *   z' = z_s s' + z_m m + sum_{k < K} z_h[k] hist[k]       the predictor (UniP), from the value s' just computed
 *   z' = (1 - mask) (b_img z_img + b_noise blend_noise) + mask z'            (with mask; the blend touches z' only, never s')
 *   z <- z';  hist[store_m] <- m;  hist[store_s] <- s';  x_next[both CFG halves] <- 16-bit(in_scale z'), channels 4..7 = 0
 * imd_sampler_step stores ONE derived quantity per step, UniPC two, and the second is an intermediate of the same step's predictor:
 * hence a block and a kernel of its own (unipc_step.hip).  hist holds up to solver_order older x0 predictions and last_sample:
 * K = solver_order + 1 <= IMD_SAMPLER_MAX_HISTORY.  The coefficients are host-computed (imagdressing_amd/scheduler.py, plan_fused). */
#define IMD_UNIPC_COEFS 19       /* floats of the device coefficient block: m_x, m_e, s_x, s_m, s_h[4], z_s, z_m, z_h[4], b_img, b_noise,
                                    in_scale, store_m, store_s */
typedef struct imd_unipc_params {
    uint32_t struct_bytes; /* sizeof(imd_unipc_params) in the caller's view; checked on entry */
    float* z;             /* [B, HW, 4] fp32 latent state, updated in place */
    const float* eps;     /* [2B, HW, 4] fp32: rows [0,B) cond pass, [B,2B) uncond pass */
    uint16_t* x_next;     /* [2B, HW, 8] 16-bit next UNet input (channels 4..7 = 0) or NULL */
    float* hist;          /* [K][B HW 4] fp32, ONE contiguous buffer owned by the caller (NULL iff K == 0).  A slot may be read and
                           * overwritten by the same launch: every thread reads its element of each slot before it stores */
    int B, HW, K;         /* K: history slots, 0..IMD_SAMPLER_MAX_HISTORY */
    int dtype;            /* element type of x_next */
    float guidance;
    const float* guidance_rows; /* NULL, or DEVICE [B] fp32: the guidance scale of each latent row, read instead of `guidance` */
    float m_x, m_e, s_x, s_m;
    float s_h[4];         /* by PHYSICAL slot; a slot whose coefficient is 0 in s_h AND z_h is not read */
    float z_s, z_m;
    float z_h[4];
    float b_img, b_noise, in_scale;
    int store_m, store_s; /* physical slots that receive m and s', -1: none; equal non-negative values are refused */
    const float* mask;    /* NULL, or [B, HW] inpaint mask; then z_img and blend_noise [B, HW, 4] are required */
    const float* z_img;
    const float* blend_noise;
    const float* coefs;   /* NULL, or DEVICE pointer to IMD_UNIPC_COEFS fp32 read by the kernel INSTEAD of m_x .. store_s above (the stores
                           * as floats holding the integers; a value outside 0..K-1 stores nothing): a captured HIP graph of a step then
                           * holds no pointer or scalar that changes between replays -- the host refreshes 76 bytes per step */
} imd_unipc_params;

/* CFG rescale (imd_guidance_rescale): Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", section 3.4 --
 * diffusers' rescale_noise_cfg with the standard deviation over all non-batch dimensions.  Per latent row b with phi != 0, in fp32
 * (t = eps[b], u = eps[B + b], N = 4 HW):
 *   e = u + g (t - u);   mu_t = (sum t) / N,  mu_e = (sum e) / N;   S_t = sum (t - mu_t)^2,  S_e = sum (e - mu_e)^2
 *   r = sqrt(S_t / S_e)  (1 if S_e == 0);   f = phi r + (1 - phi);   eps[b] = eps[B + b] = f e
 * Both CFG halves receive the rescaled guided prediction, so the step launch that follows recovers it exactly whatever guidance it
 * is given (eps_c - eps_u == 0): the launch goes between the UNet and ANY of the step entry points, none of which changes.  A row
 * with phi == 0 is neither read nor written.  The reduction order is a function of HW alone (guidance_rescale.hip). */
typedef struct imd_guidance_rescale_params {
    uint32_t struct_bytes; /* sizeof(imd_guidance_rescale_params) in the caller's view; checked on entry */
    float* eps;            /* [2B, HW, 4] fp32, in place: rows b and B + b both receive the rescaled guided prediction */
    int B, HW;
    float guidance;
    const float* guidance_rows; /* NULL, or DEVICE [B] fp32, read instead of `guidance` */
    float rescale;
    const float* rescale_rows;  /* NULL, or DEVICE [B] fp32, read instead of `rescale`; 0 = leave the row alone */
} imd_guidance_rescale_params;

/* Seeded standard-normal noise that belongs to a REQUEST (imd_noise_rows): the four channels of a latent pixel are a pure function
 * of (seed, image, draw, pixel), whatever the batch, the row, the slot of a session or the launch that writes them:
 *   (x0, x1, x2, x3) = Philox4x32-10(counter = (pixel, image, draw, 0), key = (seed_lo, seed_hi))     Salmon et al., SC'11:
 *       multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85 added to the key after each round; a round
 *       maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
 *   u_j = ((x_j >> 9) + 0.5) 2^-23                          exact in fp32, in [2^-24, 1 - 2^-24]
 *   r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2);   out = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3, r1 sin 2 pi u3)      (Box-Muller)
 * `pixel` is the NHWC pixel index inside the latent, in [0, HW).  |out| <= sqrt(2 ln 2^24) = 5.77: the tails beyond are cut (a mass of
 * about 1e-8).  The values are fp32 and are NOT torch's stream.  Draw numbering of the pipelines: draw 0 is a request's initial noise
 * (also the inpainting `noise`), draw 1 + i the variance noise of step index i of the request's full schedule; image j of
 * num_images_per_prompt is counter word image = j.  A row whose `active` word is 0 is neither read nor written.  The launch goes in
 * front of imd_sampler_step / _rows / _rows_at (their `noise` operand), none of which changes. */
#define IMD_NOISE_ROW_WORDS 8   /* per row: [0] seed_lo [1] seed_hi [2] image [3] draw [4] active (0: the row is skipped) [5..7] reserved, 0 */
#define IMD_NOISE_NORMAL 0      /* out: fp32 standard normals */
#define IMD_NOISE_BITS   1      /* out: the four raw uint32 Philox words (for exact tests) */
typedef struct imd_noise_params {
    uint32_t struct_bytes; /* sizeof(imd_noise_params) in the caller's view; checked on entry */
    void* out;             /* [rows, HW, 4] fp32 or uint32, 16-byte aligned */
    const uint32_t* key_rows; /* DEVICE [rows][IMD_NOISE_ROW_WORDS], 16-byte aligned */
    int rows, HW, kind;
} imd_noise_params;

/* soft_mask (imd_image_mask_release, imd_soft_mask_rows): the gray level of an inpainting mask as per-pixel repaint depth --
 * Differential Diffusion (Levin & Fried, 2023).  A call runs n schedule positions k = 0 .. n - 1.  Latent pixel (y, x) of an h x w
 * latent covers, on the H0 x W0 mask window, the bin of torch's adaptive_avg_pool2d: rows [floor(y H0 / h), ceil((y + 1) H0 / h)),
 * columns [floor(x W0 / w), ceil((x + 1) W0 / w)).  With S the integer sum of the bin's bytes and D = 255 cnt,
 *   release = n - ceil(S n / D) = n - (S n + D - 1) / D          (64-bit integers; 0 for an all-255 bin, n for an all-0 bin)
 * and the blend that aims at position k + 1 uses the 0 / 1 mask [k >= release]: the pixel is reset to the re-noised original up to
 * the blend that aims at position `release` and runs its last n - release = ceil(c n) steps free. */
typedef struct imd_image_mask_release_params {
    uint32_t struct_bytes;  /* sizeof(imd_image_mask_release_params) in the caller's view; checked on entry */
    const uint8_t* src;     /* DEVICE "L" mask window [H0][W0], row y at src + y * src_row_stride (a crop window is a view) */
    int64_t src_row_stride; /* bytes, >= W0 */
    uint16_t* out;          /* DEVICE [h * w] release steps, each in [0, n] */
    int H0, W0, h, w;
    int n;                  /* executed schedule positions, in [1, 65535] */
} imd_image_mask_release_params;

/* The 0 / 1 blend mask of one step from the release steps: for every row r with step_rows[r] >= 0,
 *   mask[r][p] = step_rows[r] >= release[r][p] ? 1.0f : 0.0f
 * A row with a negative entry is neither read nor written.  The launch goes in front of any step entry point that takes `mask`
 * (fp32 [B][HW] at a fixed address), none of which changes. */
typedef struct imd_soft_mask_rows_params {
    uint32_t struct_bytes;    /* sizeof(imd_soft_mask_rows_params) in the caller's view; checked on entry */
    const uint16_t* release;  /* DEVICE [B][HW], 8-byte aligned */
    const int32_t* step_rows; /* DEVICE [B]: the step k of the row, negative = leave the row alone */
    float* mask;              /* DEVICE [B][HW] fp32, 16-byte aligned */
    int B, HW;
} imd_soft_mask_rows_params;

/* Per-row LoRA with the low-rank path unfolded (imd_lora_expand_rows).  For a linear layer with LoRA,
 *   y = x W^T + s_row ((x D^T) U^T) = [x | s_row (x D^T)] [W | U]^T
 * so a scale that differs from row to row goes into the ACTIVATIONS and the augmented weight [W | U] (network_alpha / rank folded into
 * U) does not depend on it: the projection launch that follows is the existing one with Cin = C + T.  This launch writes the augmented
 * rows:   out[m, c]     = x[m, c]                                                   c < C, the same bits
 *         out[m, C + j] = 16-bit( row_scale[m / rows_per_entry] * sum_c x[m, c] down[j, c] )       j < T
 * The sum is accumulated in fp32 on the MFMA, the scale multiplies the finished sum in fp32, and the product is rounded ONCE to the
 * element type (round to nearest even).  Bytes of an output row past C + T are not written. */
typedef struct imd_lora_rows_params {
    uint32_t struct_bytes; /* sizeof(imd_lora_rows_params) in the caller's view; checked on entry */
    const uint16_t* x;     /* [M, C] 16-bit, row stride x_ld */
    const uint16_t* down;  /* [T, C] 16-bit, contiguous: the stacked LoRA down matrices of the launch (T = G rank) */
    const float* row_scale; /* DEVICE [E] fp32 */
    uint16_t* out;         /* [M, >= C + T] 16-bit, row stride out_ld; must not overlap x */
    int M, C, T;           /* C: a multiple of 16 in 64..1280; T: a multiple of 16 in 16..384 */
    int E, rows_per_entry; /* M == E * rows_per_entry */
    int x_ld, out_ld;      /* in elements, multiples of 8; x_ld >= C, out_ld >= C + T */
    int dtype;
} imd_lora_rows_params;

/* A scale per batch row on up to 16 tensors at once, in place (imd_residual_scale_rows): the ControlNet residuals of a batch whose
 * requests differ in controlnet_conditioning_scale or in their guidance window.  The zero convs then run with out_scale = 1 and this
 * launch follows them.  Segment k is a contiguous 16-bit [rows, row_elems[k]] tensor; for every segment and every row r
 *   scale_rows[r] == 1.0f:  the row is neither read nor written -- its bytes, NaN payloads included, stay
 *   otherwise:              out = 16-bit( float(x) * scale_rows[r] )     widen, ONE fp32 multiply, round to nearest even
 * 0 and negative values are scales like any other.  Against the folded launch, 16-bit(s (W x + b)), the result 16-bit(s 16-bit(W x + b))
 * carries one more rounding: at most one unit in the last place of the element type, none where s is 1 (bf16: a power of two).
 * Segments must not overlap. */
#define IMD_SCALE_ROWS_MAX_SEGMENTS 16
typedef struct imd_scale_rows_params {
    uint32_t struct_bytes; /* sizeof(imd_scale_rows_params) in the caller's view; checked on entry */
    int dtype;             /* IMD_DTYPE_*: the element type of every segment */
    int rows, segments;    /* rows >= 1; segments in 1..IMD_SCALE_ROWS_MAX_SEGMENTS */
    const float* scale_rows; /* DEVICE [rows] fp32, 4-byte aligned: the same array for all segments */
    void* data[16];        /* [IMD_SCALE_ROWS_MAX_SEGMENTS] segment bases, 16-byte aligned; entries at or past `segments` are not read */
    int row_elems[16];     /* elements per row of each segment: positive multiples of 8 */
} imd_scale_rows_params;

/* The scaled sum of up to 4 sources on up to 16 tensors at once (imd_residual_mix_rows): the residuals of several ControlNets, every
 * net with its own scale per batch row, mixed for the UNet in ONE launch.  The nets run with out_scale = 1 and this launch follows the
 * last of them.  Segment j of source k is a contiguous 16-bit [rows, row_elems[j]] tensor; for every segment j and every row r
 *   acc = nothing
 *   for k = 0 .. sources - 1, in this order:
 *       s = scales[k * rows + r]
 *       if s == 0.0f: continue                      source k's row is NOT read (NaN and Inf in it stay out of the sum)
 *       term = float(src[k][j][r]) * s              widen (exact), ONE fp32 multiply, rounded
 *       acc  = term, or acc + term                  ONE fp32 add, rounded -- never a fused multiply-add
 *   dst[j][r] = 16-bit(acc), round to nearest even; +0 where every source was skipped
 * which is, bit for bit, the same chain of x.float() * torch.tensor(s, dtype=torch.float32) and + on the CPU.  Against K - 1 element-wise
 * adds of 16-bit tensors the sum is rounded to 16 bits once, not K times.  dst[j] may BE src[k][j] (in place on one source; a thread
 * reads all its vectors of a chunk before it stores any); any other overlap of a dst segment with a source or another dst segment is
 * refused.  Sources are otherwise only read. */
#define IMD_MIX_ROWS_MAX_SOURCES 4
#define IMD_MIX_ROWS_MAX_SEGMENTS 16
typedef struct imd_mix_rows_params {
    uint32_t struct_bytes; /* sizeof(imd_mix_rows_params) in the caller's view; checked on entry */
    int dtype;             /* IMD_DTYPE_*: the element type of every segment, sources and dst alike */
    int rows, segments;    /* rows >= 1; segments in 1..IMD_MIX_ROWS_MAX_SEGMENTS */
    int sources;           /* 1..IMD_MIX_ROWS_MAX_SOURCES */
    const float* scales;   /* DEVICE [sources][rows] fp32, 4-byte aligned: source-major, the same array for all segments */
    const void* src[4][16]; /* [IMD_MIX_ROWS_MAX_SOURCES][IMD_MIX_ROWS_MAX_SEGMENTS] bases, 16-byte aligned; entries past `sources` / `segments` are not read */
    void* dst[16];         /* segment bases of the result, 16-byte aligned */
    int row_elems[16];     /* elements per row of each segment: positive multiples of 8 */
} imd_mix_rows_params;

/* Device-side image input (imd_image_resample): separable antialiased resampling of uint8 images, bit-exact with Pillow's 8-bit
 * resampler (libImaging/Resample.c), with a fused output stage -- the work diffusers' VaeImageProcessor / transformers'
 * CLIPImageProcessor do on the host in front of IMAGDressing_v1_pipeline*.py.  Per axis whose size changes the caller passes a
 * coefficient table for `n` outputs: xmin[n], count[n] (int32) and k[n][kmax] (int32 fixed point, 22 fraction bits, zero padded):
 *   h[y][x][c]   = clip8((2^21 + sum_{j < count[x]} src[y][xmin[x] + j][c] * k[x][j]) >> 22)          horizontal, int32 accumulator
 *   res[y][x][c] = clip8((2^21 + sum_{j < count[y]} h[ymin[y] + j][x][c] * k[y][j]) >> 22)            vertical, over the uint8 h
 * An axis whose table pointers are NULL is skipped (then Wres == Win / Hres == Hin is required).  Output stage over the crop window
 * (top, left, crop_h, crop_w) of the resized image, v = res[top + y][left + x][c] (binarize != 0: v = v / 255.0f >= 0.5f ? 255 : 0):
 *   IMD_IMG_U8        uint8 [B, crop_h, crop_w, C]                                       v
 *   IMD_IMG_F32_NCHW  fp32  [B, C, crop_h, crop_w]                                       (float(v) / 255.0f) * a[c] + b[c]
 *   IMD_IMG_16_NHWC8  fp16 / bf16 [B, crop_h, crop_w, 8], channels C..7 zero             the same, rounded to nearest even
 * (IEEE division, then one rounded multiply and one rounded add: no FMA contraction.)
 * Both axes resampled: ONE launch when the horizontally resampled rows that an output tile of IMD_IMG_TILE_H rows needs fit the LDS
 * tile (v_tile_rows * IMD_IMG_TILE_W * C <= IMD_IMG_LDS_BYTES) and IMD_IMG_FORCE_TWO_PASS is not set; otherwise two launches through
 * `tmp`, uint8 [B, Hin, crop_w, C].  imd_image_resample_form answers which, without launching: 1 | 2 launches, 0 = refused. */
enum { IMD_IMG_U8 = 0, IMD_IMG_F32_NCHW = 1, IMD_IMG_16_NHWC8 = 2 };
#define IMD_IMG_FORCE_TWO_PASS 1
#define IMD_IMG_TILE_W 32
#define IMD_IMG_TILE_H 8
#define IMD_IMG_LDS_BYTES 32768
typedef struct imd_image_resample_params {
    uint32_t struct_bytes; /* sizeof(imd_image_resample_params) in the caller's view; checked on entry */
    const uint8_t* src;    /* uint8 [B, Hin, Win, C] */
    int64_t src_row_stride, src_img_stride;   /* bytes from row to row and from image to image */
    void* out;
    uint8_t* tmp;          /* [B, Hin, crop_w, C] uint8: required when both axes are resampled in two launches */
    int B, Hin, Win, C;    /* C: 1 | 3 */
    int Hres, Wres;        /* size of the resized image */
    const int32_t* h_xmin; /* horizontal table (DEVICE pointers, Wres entries), all NULL: the axis is skipped */
    const int32_t* h_count;
    const int32_t* h_k;
    int h_kmax, h_taps;    /* row length of h_k; the largest entry of h_count (refused when above h_kmax) */
    const int32_t* v_xmin; /* vertical table (Hres entries), all NULL: the axis is skipped */
    const int32_t* v_count;
    const int32_t* v_k;
    int v_kmax, v_taps;
    int v_tile_rows;       /* max over tiles t of rows of h that output rows [top + t TILE_H, top + (t + 1) TILE_H) read (both axes resampled) */
                           /* TRUSTED: the library cannot read the device tables.  A value below the true one keeps the single launch where
                            * the rows do not fit: reads are clamped (memory-safe) but pixels are wrong, with no error. */
    int top, left, crop_h, crop_w;
    int kind;              /* IMD_IMG_* */
    int dtype;             /* IMD_DTYPE_* of an IMD_IMG_16_NHWC8 output */
    int binarize;
    int flags;             /* IMD_IMG_FORCE_TWO_PASS */
    float a[3], b[3];
} imd_image_resample_params;

/* Device-side image output (imd_image_pack_u8): 16-bit [B, H, W, ld] (ld = 4 | 8; AutoencoderKL.decode_nhwc) -> uint8 [B, H, W, 3],
 * u = rint(clamp(x / 2 + 0.5, 0, 1) * 255) per value in fp32, rint to nearest even (numpy.round) -- the operations of
 * `(image / 2 + 0.5).clamp(0, 1)` ... `(x * 255).round().astype("uint8")` (IMAGDressing_v1_pipeline.py:544-547 through diffusers'
 * VaeImageProcessor.postprocess), identical for every finite 16-bit input. */
typedef struct imd_image_pack_params {
    uint32_t struct_bytes; /* sizeof(imd_image_pack_params) in the caller's view; checked on entry */
    const uint16_t* src;
    uint8_t* out;
    int B, H, W, ld;
    int dtype;             /* IMD_DTYPE_* of src */
} imd_image_pack_params;

/* Inpainting result composited into the person image on the device (imd_image_overlay): what diffusers' apply_overlay does on the
 * host behind StableDiffusionControlNetInpaintPipeline, as ONE Image.composite(base, orig, mask) -- base = orig with the generated
 * window pasted at (x1, y1) -- per byte, integer only:
 *   inside the box  [y1, y1 + ch) x [x1, x1 + cw):  t = orig * (255 - m) + gen * m + 128;  out = ((t >> 8) + t) >> 8
 *   outside:                                        out = orig
 * with m = mask[b][y][x] (not binarised: a feathered mask feathers the seam); m = 0 returns orig and m = 255 returns gen exactly.
 * Equal to Pillow's Image.composite on all 256^3 (orig, gen, m) triples.  gen is the decoded window already resized to the box
 * (imd_image_resample, IMD_IMG_U8).  orig / mask hold Bo = 1 image shared by the B outputs, or B.  No pointer needs any alignment.
 * Refused: null pointers, an empty image or box, Bo other than 1 or B, a box outside the image, an image of more than 2^31 bytes. */
typedef struct imd_image_overlay_params {
    uint32_t struct_bytes; /* sizeof(imd_image_overlay_params) in the caller's view; checked on entry */
    const uint8_t* orig;   /* uint8 [Bo, H0, W0, 3] */
    const uint8_t* mask;   /* uint8 [Bo, H0, W0] */
    const uint8_t* gen;    /* uint8 [B, ch, cw, 3] */
    uint8_t* out;          /* uint8 [B, H0, W0, 3] */
    int B, Bo;             /* Bo: 1 (orig and mask shared by every output) or B */
    int H0, W0;
    int x1, y1, cw, ch;    /* the box: left, top, width, height */
} imd_image_overlay_params;

/* The ControlNet image of the inpainting script on the device (imd_image_inpaint_condition; make_inpaint_condition,
 * inference_IMAGdressing_controlnetinpainting.py:48-59) from uint8 inputs of one size: per pixel and channel c < 3
 *   v = (float(mask) / 255.0f > 0.5f) ? -1.0f : float(image[c]) / 255.0f          IEEE division
 * rounded to nearest even into fp16 / bf16 [B, H, W, 8], channels 3..7 zero -- the values the IMD_IMG_16_NHWC8 stage of
 * imd_image_resample gives with a = 1, b = 0, and -1 where the mask is set.  out must be 16-byte aligned. */
typedef struct imd_image_inpaint_condition_params {
    uint32_t struct_bytes; /* sizeof(imd_image_inpaint_condition_params) in the caller's view; checked on entry */
    const uint8_t* image;  /* uint8 [B, H, W, 3] */
    const uint8_t* mask;   /* uint8 [B, H, W] */
    void* out;             /* fp16 / bf16 [B, H, W, 8] */
    int B, H, W;
    int dtype;             /* IMD_DTYPE_* of out */
} imd_image_inpaint_condition_params;

/* Mask growing and feathering on the device (imd_image_mask_filter): Pillow's ImageFilter.MaxFilter(2k + 1) followed by
 * ImageFilter.GaussianBlur(radius) on uint8 "L" images, byte for byte, integer only.
 *   window maximum (k >= 1):  out[y][x] = max of in over [y - k, y + k] x [x - k, x + k] clipped at the border (separable)
 *   Gaussian (blur != 0):     Pillow's three extended box blurs per axis.  The caller computes the box in FLOAT32 with passes = 3:
 *       sigma2 = radius * radius / passes;  L = sqrt(12 sigma2 + 1);  l = floor((L - 1) / 2)
 *       a = (2l + 1)(l (l + 1) - 3 sigma2) / (6 (sigma2 - (l + 1)(l + 1)));  fr = l + a
 *       r = int(fr);  ww = uint32(float32(2^24) / (fr * 2 + 1));  fw = (2^24 - (2r + 1) ww) / 2
 *     and one pass along a line of n samples, indices clamped to [0, n - 1] (edge replication), is
 *       out[x] = (ww * sum_{j = -r..r} in[c(x + j)] + fw * (in[c(x - r - 1)] + in[c(x + r + 1)]) + 2^23) >> 24
 *     in uint32 (every intermediate is below 2^32).  Three passes along rows, then three along columns, each over the uint8 result
 *     of the one before.  Any r, also r >= n.
 * src and out are [B, H, W] with row and image strides in bytes; out may be src (in place).  No pointer needs any alignment.
 * bounds (optional, int32 [B][4]): (x_min, y_min, x_max, y_max) of the non-zero pixels of out, (W, H, -1, -1) for an all-zero image.
 * Launches: one per axis and step through LDS -- columns (maximum), rows (maximum and the three row passes), columns (the three
 * column passes); two for one step alone; plus one that initialises bounds -- at most 4.  A line (row or column) longer than
 * IMD_IMG_MASK_LINE_MAX bytes, or IMD_IMG_MASK_FORCE_GLOBAL, takes one launch per pass through tmp, uint8 [B, H, W] contiguous
 * (needed only then).  imd_image_mask_filter_form answers the number of launches without launching, 0 = refused.
 * Refused: null pointers (src / out; tmp where it is needed), an empty image, a stride below the row / image, blur with passes != 3,
 * k < 0, ww / fw inconsistent with r ((2r + 1) ww + 2 fw must be 2^24 or 2^24 - 1), an image of more than 2^31 bytes. */
#define IMD_IMG_MASK_LINE_MAX 16384
#define IMD_IMG_MASK_FORCE_GLOBAL 1
typedef struct imd_image_mask_filter_params {
    uint32_t struct_bytes;   /* sizeof(imd_image_mask_filter_params) in the caller's view; checked on entry */
    const uint8_t* src;      /* uint8 [B, H, W] */
    int64_t src_row_stride;  /* bytes between rows of src (>= W) */
    int64_t src_img_stride;  /* bytes between images of src */
    uint8_t* out;            /* uint8 [B, H, W]; may be src */
    int64_t out_row_stride, out_img_stride;
    uint8_t* tmp;            /* uint8 [B, H, W] contiguous; only for the one-launch-per-pass form */
    int32_t* bounds;         /* optional int32 [B][4] */
    int B, H, W;
    int k;                   /* half-width of the window maximum; 0: skipped */
    int blur;                /* 0: the Gaussian is skipped */
    int passes;              /* box blurs per axis of the Gaussian: 3 */
    uint32_t r, ww, fw;      /* the box, see above */
    int flags;               /* IMD_IMG_MASK_FORCE_GLOBAL */
} imd_image_mask_filter_params;

/* library / device */
int imd_abi_version(void);
const char* imd_last_error(void);
/* 0 iff `device` is a gfx950 part this library was built for. */
int imd_device_check(int device);

/* Implicit-GEMM convolution / linear layer with fused epilogue.
 * Replaces (diffusers==0.24.0, called from dressing_sd/pipelines/IMAGDressing_v1_pipeline.py:466,499,511):
 * ResnetBlock2D.conv1/conv2/conv_shortcut/time_emb_proj, Down/Upsample2D.conv, Transformer2DModel.proj_in/out,
 * Attention.to_q/to_k/to_v/to_out[0], FeedForward (GEGLU), TimestepEmbedding, ControlNet zero-convs; and
 * RefSAttnProcessor2_0.to_k_ref/to_v_ref (adapter/attention_processor.py:600-601), to_k_ip/to_v_ip (:841-842),
 * the nn.Linear layers of adapter/resampler.py.  cfg (rows x channels x K-depth of a workgroup tile): -1 auto, 0: 128x128x64, 1: 128x64x64, 2: 64x64x64,
 * 3: 64x64x64 with 4 K tiles in flight, 4: 128x128x32, 5: 3x3 halo-patch kernel, 6: 64x320x32 (N % 320 == 0: no idle columns),
 * 7: 64x64x32 / 4 in flight, 8: 128x128x32 / 4 in flight, 9: 256x128x32, 10: 256x256x32 and 11: 128x320x64 (8-wave workgroups:
 * fewer operand bytes fetched per MFMA for the wide projections; 11 covers N = 320 k with full-width row blocks); 12..15: row-resident
 * kernels; 16: 256x256x64 and 17: 128x128x32 with a three-stage ring, both operands staged by LDS-DMA (plain linear layers, K % 64 == 0);
 * 18: the gathering form of 17 for 3x3 convolutions (stride 1 | 2, Cin % 32 == 0; K slices allowed for 17 and 18);
 * 19 / 20: 17 / 18 with a four-stage ring (64 KB, two workgroups per CU, three tiles of lead);
 * 21: the halo-patch kernel with 16 x 16 pixel tiles (256 pixels x 128 channels per workgroup, wave tiles 128 x 64: half the weight bytes per MAC);
 * 22: the halo-patch kernel with 8 x 16 pixels x 160 channels per workgroup (wave tiles 32 x 160: N = 320 k runs without idle waves or padded MFMAs);
 * 23: 22 with eight waves = 16 x 16 pixels x 160 channels per workgroup (one staged weight tile serves 256 pixels: 154 instead of 290 bytes of LDS-DMA per MFMA).
 * 25 / 27: the 128 x 128 LDS-DMA tiles of 17 / 19 with 128-BYTE rows (K tile 64), two / three ring stages: the L2 hands a CU whole 128-byte lines, 64-byte
 *     rows use half of each (tools/probes/staging_probe.hip); 26 / 28: the 3x3 gathering form of the same (one tap x 64 channels per tile, Cin % 64 == 0).
 * 29: the halo-patch kernel (5) with 64-channel chunks = 128-byte rows and a two-slot weight ring (80 KB of LDS, two workgroups per CU): measured slower
 *     than 5 on every shape of the UNet (the ring and the third workgroup matter more than the whole lines), kept as a tuning candidate.
 * 24: 3x3 stride-1 convolutions of maps 8 pixels wide (the UNet's lowest level): a workgroup owns all pixels of up to 8 images x 64 channels x one
 *     K slice, so every weight byte is fetched once; K-sliced only (split_k >= 2).
 * Results are identical up to fp32 summation order. */
int imd_conv_gemm(const imd_conv_gemm_params* p, int cfg, void* stream);
int imd_conv_gemm_auto_cfg(int M, int N);
/* suggested number of K slices for tile config `cfg` (1 = do not split) */
int imd_conv_gemm_auto_split(int M, int N, int K, int cfg);

/* Fused dual-softmax attention.  Replaces the two F.scaled_dot_product_attention calls + add of
 * RefSAttnProcessor2_0.__call__ (adapter/attention_processor.py:589-612), LoRAIPAttnProcessor2_0 (:833-856),
 * the single SDPA of CAttnProcessor2_0 (:277-279) / CacheAttnProcessor2_0 (:80-82), and
 * PerceiverAttention's softmax(QK^T)V (adapter/resampler.py:71-74). */
int imd_attention(const imd_attn_params* p, void* stream);
/* The same fused dual-softmax attention for head dim 40 on the MX block-scaled FP8 MFMA (BASELINE.json configs[4]: the
 * 768x576 ControlNet-inpainting configuration "with fp8 MFMA attention").  q / k1 / v1t / k2 / v2t of `p` point to e4m3
 * operands produced by imd_attn_quantize_fp8 (Q8, K8: [.., rows, 64] bytes; V8^T: [.., 64, LP] bytes, keys permuted inside
 * groups of 64); `out` and `dtype` are the 16-bit output.  eq / ek / ev: the power-of-two exponents the operands were
 * scaled by (q * 2^eq ...), 0 <= eq + ek <= 8.  Same reference lines as imd_attention (attention_processor.py:589-612). */
int imd_attention_fp8(const imd_attn_params* p, int eq, int ek, int ev, void* stream);
/* 16-bit head-split attention operands -> the e4m3 operands of imd_attention_fp8.
 * kind 0: Q or K rows [count, 48] -> [count, 64]: columns 0..39 scaled by 2^exp2_scale, columns 40 and 41 = pad_val
 *         (Q: 0; K: 2^(eq+ek), the slots that carry the deferred row maximum), the rest 0;
 * kind 1: V^T [count, 64, LP] -> [count, 64, LP] bytes (rows 0..39), scaled by 2^exp2_scale, key k of every 64-group stored
 *         at position 32 ((k >> 3) & 1) + 8 ((k >> 4) & 3) + (k & 7) (the order the kernel's packed P comes out in). */
int imd_attn_quantize_fp8(const uint16_t* src, uint8_t* dst, int kind, long count, int LP, int exp2_scale, float pad_val, int dtype,
                          void* stream);
/* 1 iff tile config cfg (12 / 13 / 14: the row-resident projections) can normalise its input rows as *p's gn_in_* fields ask */
int imd_row_linear_gn_in_supported(const imd_conv_gemm_params* p, int cfg);
/* 1 iff the finish launch of *p (split_k filled in as imd_conv_gemm will see it) can apply GroupNorm(gn_out_groups) (+ SiLU) to its output */
int imd_conv_gemm_gn_out_supported(const imd_conv_gemm_params* p);
/* 1 iff imd_attention accepts imd_attn_params.out_dup for this head count / query count / head dim (with k_pad_one = 1) */
int imd_attention_dup_supported(int H, int N, int D);
/* 1 iff imd_attention runs phase2_rows / phase2_out at this head dim (the generic kernel: 64, 80, 160) */
int imd_attention_phase_split_supported(int D);
/* padded head dims of the Q/K rows (dpk) and V^T rows (dpv) for head dim D */
int imd_attn_padded_dims(int D, int* dpk, int* dpv);
/* performance knobs (results are identical for every accepted setting up to fp32 summation order).  knob 0: head-dim-40 attention
 * kernel variant (default 13: the static-ring kernel 12 with the deferred-maximum overflow test on a phase's first and last steps
 * only and a workgroup-level re-run as 12 when a softmax denominator comes out non-finite -- bf16, fp16 runs 12; 12: the LDS-DMA
 * kernel with compile-time ring addresses; 10: software-pipelined kernel of attention_d40.hip with the P.V tail on
 * v_mfma_f32_16x16x32, LDS-DMA staging when imd_attn_params.k_pad_one; 11: the same with register staging; 9 / 7: the round-2 kernel with the same two staging
 * rules; 6, 8: scheduling variants of 7; 1..5: round-1 kernel shapes.  Values 20..39 (timing ablations that compute WRONG
 * results) are accepted only by a library built with -DIMD_ABLATIONS; a normal build rejects them);
 * knob 1: XCD-aware work mapping of the attention grid (0|1);
 * knob 2: GEMM operand-fetch bits (bit0: tap-inner K order for 3x3 convs, bit1: weight loads bypass the L1,
 * bit2: XCD-aware tile order -- each XCD's L2 owns whole row tiles or whole channel tiles, whichever moves fewer bytes;
 * bit4: row tiles visited in groups of 8 inside an XCD's range; A/B switches with identical results: bit8 row_linear's staged epilogue,
 * bit9 the halo-patch conv staged through registers, bit10 8-byte stores in the row kernels.  Bits 5..7 are timing ablations of
 * gemm_dma256.hip that compute WRONG results: compiled into, and accepted by, -DIMD_ABLATIONS builds only -- a normal build rejects
 * them, and any bit above 10). */
int imd_set_tuning(int knob, int value);
/* current value of a knob (-1: unknown knob): lets a harness snapshot and restore the process-global settings around an A/B */
int imd_get_tuning(int knob);

/* GroupNorm (+SiLU) over NHWC: diffusers ResnetBlock2D.norm1/norm2, Transformer2DModel.norm, conv_norm_out. */
int imd_groupnorm(const imd_groupnorm_params* p, void* stream);
int imd_groupnorm_workspace_floats(int B, int HW, int C, int G);
/* Statistics only: writes the normalisation of ResnetBlock2D.norm1/norm2 as per-(batch, channel) fp32 coefficients
 * coef_a[B][C], coef_b[B][C] (y = x*a + b; p->y is unused) for imd_conv_gemm's fused prologue (gn_a / gn_b, cfg 5). */
int imd_groupnorm_coeffs(const imd_groupnorm_params* p, float* coef_a, float* coef_b, void* stream);
/* 1 iff tile config 5 (LDS-resident halo patch: 3x3, stride 1, H % 8 == 0, W % 16 == 0, Cin % 32 == 0) can run *p. */
int imd_conv_patch_supported(const imd_conv_gemm_params* p);
/* 1 iff tile config 21 (the halo-patch kernel with 16 x 16 pixel tiles, conv_patch2.hip) takes this geometry */
int imd_conv_patch2_supported(const imd_conv_gemm_params* p);
/* 1 iff tile config 22 (the halo-patch kernel with 160-channel tiles, conv_patch3.hip: N = 320 k without idle waves) takes this geometry */
int imd_conv_patch3_supported(const imd_conv_gemm_params* p);
/* 1 iff tile config 23 (the same kernel with eight waves: 16 x 16 pixels x 160 channels per workgroup) takes this geometry */
int imd_conv_patch4_supported(const imd_conv_gemm_params* p);
/* 1 iff tile config 24 (conv_img.hip: whole maps 8 pixels wide x 64 channels x one K slice per workgroup, split_k >= 2) takes this problem;
 * split_k must be filled in as imd_conv_gemm will see it */
int imd_conv_img_supported(const imd_conv_gemm_params* p);
/* number of statistic partials per image the halo-patch kernel writes for this geometry (gn_stats_out), 0 if it cannot */
int imd_conv_patch_stats_parts(const imd_conv_gemm_params* p);
/* the same for ANY launch: partials per image that imd_conv_gemm(p, cfg) writes through gn_stats_out -- the halo-patch epilogue (cfg 5, no K
 * slices) or, with p->split_k > 1 and a separate finish launch (splitk_counters == NULL), the finish launch itself, which then sums the
 * slices, runs the epilogue AND emits the statistics of the tensor it stores (row-major 16-bit outputs, N / groups >= 8); the halo-patch
 * kernels with 160-channel tiles (cfg 22 / 23) emit them from their own epilogue like cfg 5; 0: none */
int imd_conv_gemm_stats_parts(const imd_conv_gemm_params* p, int cfg);
/* 1 iff tile config 16 (256 x 256 x 64 LDS-DMA tile kernel, gemm_dma.hip: plain linear layer, K % 64 == 0, no K split) can run *p. */
int imd_gemm_dma_supported(const imd_conv_gemm_params* p);

/* Row-resident linear layers: K = 320, N = 64..320 in steps of 64 (row_linear.hip, the 64x64-level token matrix; tile config
 * 12 of imd_conv_gemm) and K = 640 / 1280, N a multiple of 160 with a bias / scale / residual / head-split-Q
 * epilogue (row_linear_k640.hip / row_linear_k1280.hip, the 32x32 / 16x16 levels; tile configs 13 / 14); and the fused q / k / v
 * projection of a 320-channel self-attention layer (K = 320, N = 960, head-split epilogue with Q, K row-major and V transposed,
 * Hout * Wout a multiple of 128: row_qkv.hip, tile config 15 -- norm1 -> to_q / to_k / to_v as one launch when ln != 0).  Same parameter block and fused epilogue as imd_conv_gemm (taps = 1).  Every wave keeps its 32 token rows in registers, the weights stream through LDS by DMA.  ln != 0: LayerNorm
 * WITHOUT affine (eps = ln_eps) is applied to each row of x on the fly -- BasicTransformerBlock.norm2 -> attn2.to_q as one
 * launch; the caller folds the affine part into the layer: W' = W diag(gamma), b' = b + W beta. */
int imd_row_linear(const imd_conv_gemm_params* p, int ln, float ln_eps, void* stream);
int imd_row_linear_supported(const imd_conv_gemm_params* p);

/* BasicTransformerBlock.norm3 + ff (GEGLU feed-forward) + residual as one launch; see imd_ff_params. */
int imd_ff_geglu(const imd_ff_params* p, void* stream);

/* BasicTransformerBlock.norm2 + attn2 (text cross-attention, to_q .. to_out[0]) + residual as one launch; see imd_xattn_params.
 * imd_text_xattn320_supported: 1 iff the geometry in *p (M, C, heads, L, rows_per_image, kv_bdiv, text_rows, x_ld, out_ld, dtype) is one the
 * kernel takes; pointers are not looked at. */
int imd_text_xattn320(const imd_xattn_params* p, void* stream);
int imd_text_xattn320_supported(const imd_xattn_params* p);

/* Upsample2D (nearest-2x interpolate -> 3x3 conv) as four 2x2 PHASE convolutions (conv_ups_phase.hip): out[2y + py, 2x + px] = bias +
 * sum over dy, dx in {0, 1} of W'[py, px][dy, dx] . src[y + py - 1 + dy, x + px - 1 + dx] (out-of-image src = 0) -- 4 taps instead of 9.
 * *p describes the 9-tap problem exactly as imd_conv_gemm takes it (taps = 9, K = 9 Cin, stride = 1, ups = 1, Hout = 2 Hin, Wout = 2 Win),
 * except that p->w holds the PHASE weights [4 phases py * 2 + px][N][4 taps dy * 2 + dx][Cin] in the activation type, the 3x3 taps that
 * fall on one source pixel summed in fp32 and rounded once (rows: py = 0: {ky 0}, {ky 1, 2}; py = 1: {ky 0, 1}, {ky 2}; the same in x;
 * imagdressing_amd/ops.py::pack_upsample_phase, once per layer).
 * imd_conv_ups_phase runs any problem with Cin % 32 == 0, contiguous 16-bit input and output (x_pix_stride = Cin, out_ld = N) below 2 GiB like
 * the phase weights, and the bias as its whole epilogue (no residual, row vector, GroupNorm prologue, statistics, activation, scale, K slices,
 * fp32 or head-split output).  imd_conv_ups_phase_supported: 1 iff it runs *p AND the launch pays against the 9-tap form, whose results it does
 * not reproduce bit for bit: 6/5 of the tile-padded multiply count of the phase form (16 per 8 x 16 tile of the source map) is below that of the
 * 9-tap form (9 per 8 x 16 tile of the output map) -- an 8 x 8 source is refused -- and the grid (images x source tiles x 4 phases x 128-channel
 * tiles) has at least 160 workgroups, the smallest at which a gain over the K-sliced 9-tap launch has been measured (the kernel takes no K slices).
 * Pointers are not looked at. */
int imd_conv_ups_phase(const imd_conv_gemm_params* p, void* stream);
int imd_conv_ups_phase_supported(const imd_conv_gemm_params* p);

/* LayerNorm over the last dim: BasicTransformerBlock.norm1/2/3; adapter/resampler.py:16,43-44,199. */
int imd_layernorm(const imd_layernorm_params* p, void* stream);
/* Row softmax, fp32 in -> 16-bit out: p[r][c] = softmax_c(s[r][:cols]) (the upcast softmax of the single-head, d = 512
 * attention in the VAE mid block -- diffusers AttnProcessor on AutoencoderKL.{encoder,decoder}.mid_block.attentions.0,
 * reached from IMAGDressing_v1_pipeline.py:457-458,:544).  cols <= 16384, row strides in elements. */
int imd_softmax_rows(const float* s, int s_ld, uint16_t* p, int p_ld, int rows, int cols, int dtype, void* stream);

/* CFG combine + DDIM step (+ inpaint blend) + next UNet input:
 * IMAGDressing_v1_pipeline.py:483-488,521-532; ..._pipeline_controlnet_inpainting.py:487-500. */
int imd_ddim_cfg_step(const imd_ddim_params* p, void* stream);
/* The same fused step with the guidance scale read PER LATENT ROW: guidance is a DEVICE [B] fp32 array (row b of z / the
 * cond-uncond pair b, B + b of eps) and p->guidance is ignored; everything else -- coefs, var_noise, the inpaint blend, x_next --
 * as imd_ddim_cfg_step.  One call then serves a batch of requests with different guidance scales (the pipelines'
 * request-batched call).  With every entry equal to g it is bit-identical to imd_ddim_cfg_step with guidance = g. */
int imd_ddim_cfg_step_rows(const imd_ddim_params* p, const float* guidance, void* stream);
/* CFG combine + one step of an affine sampler (+ history update, noise, inpaint blend) + next UNet input as ONE launch; see
 * imd_sampler_params.  Replaces `scheduler.step` of diffusers' DPMSolverMultistepScheduler / EulerDiscreteScheduler /
 * EulerAncestralDiscreteScheduler / PNDMScheduler at the call site IMAGDressing_v1_pipeline.py:530-532 (the pipelines take any
 * KarrasDiffusionSchedulers member, ..._pipeline_controlnet.py:36-41).  Errors without launching: K outside 0..4, store outside
 * -1..K-1 (host coefficients), a mask without z_img / blend_noise, K > 0 without hist, misaligned pointers (16 bytes for the
 * float4 / uint4 tensors, 4 for mask, guidance_rows and coefs). */
int imd_sampler_step(const imd_sampler_params* p, void* stream);
/* The same fused step with the coefficient block read PER LATENT ROW (a denoising session: every row is a request at its own
 * position of its own schedule).  Row b = pixel / HW reads coef_rows[b]; p->coefs and the scalar fields m_x .. store are ignored.
 * Guidance: p->guidance_rows[b], or p->guidance when that pointer is NULL.  History slot k of row b is still p->hist + k B HW at the
 * pixel, so each row has its own physical slot map through its own z_h[] and store (store >= K stores nothing).  A row whose
 * `active` float is 0 is neither read nor written: its z, its pixels of every history slot and of both CFG halves of x_next keep
 * their bytes.  With every row equal and active it is bit-identical to imd_sampler_step.  Errors without launching: a foreign
 * struct_bytes, coef_rows NULL or not 16-byte aligned, and every pointer / K / mask condition of imd_sampler_step. */
#define IMD_SAMPLER_ROW_FLOATS 16   /* per latent row: [0..12] the coefficient block in imd_sampler_params.coefs order,
                                       [13] active (0: the row is skipped), [14..15] reserved, 0 */
int imd_sampler_step_rows(const imd_sampler_params* p, const float* coef_rows /* DEVICE [B][16] fp32 */, void* stream);
/* imd_sampler_step_rows of a COMPACTING session: the forward ran p->B <= slots batch rows, and batch row r carries the request that lives
 * in slot row_slot[r].  Addressed by ROW (p->B of them): eps [2B, HW, 4], x_next [2B, HW, 8] (rows r and B + r), coef_rows and
 * p->guidance_rows [B].  Addressed by SLOT (`slots` of them): z, hist (history plane k starts at hist + k slots HW), noise, mask, z_img
 * and blend_noise.  A row whose coefficient block is inactive, or whose slot is outside [0, slots) (-1 marks an idle row), is skipped
 * whole -- no load, no store -- so the kernel stays inside its buffers whatever the device map holds; slots that no row names keep
 * their bytes.  Two rows must not name one slot.  The per-pixel arithmetic is the one copy imd_sampler_step_rows uses: with row_slot the
 * identity and slots == B the two launches are bit-identical.  Errors without launching: those of imd_sampler_step_rows, row_slot
 * NULL or not 4-byte aligned, slots < 1, B > slots. */
int imd_sampler_step_rows_at(const imd_sampler_params* p, const float* coef_rows /* DEVICE [B][16] fp32 */,
                             const int* row_slot /* DEVICE [B] */, int slots, void* stream);
/* The UNet input of a session's batch rows from the fp32 latents: x_in[r] = x_in[B + r] = 16-bit(in_scale_rows[r] z[row_slot[r]]),
 * channels 4..7 zero, with the pack expression of the step's x_next -- given the in_scale of a request's last step (coefficient [11])
 * it reproduces that step's x_next bit for bit.  z [slots, HW, 4] fp32, x_in [2B, HW, 8] 16-bit, row_slot and in_scale_rows DEVICE [B].
 * Rows with a slot outside [0, slots) are skipped.  Errors without launching: a null pointer, B or HW < 1, slots < 1, B > slots, z or
 * x_in not 16-byte aligned, row_slot or in_scale_rows not 4-byte aligned, an unknown dtype. */
int imd_session_input_rows(const float* z, const int* row_slot, const float* in_scale_rows, void* x_in, int B, int slots, int HW,
                           int dtype_code, void* stream);
/* CFG combine + one UniPC step (x0 prediction, corrector, predictor, both history stores, inpaint blend) + next UNet input as ONE
 * launch; see imd_unipc_params.  Replaces `scheduler.step` of diffusers' UniPCMultistepScheduler at the call site
 * IMAGDressing_v1_pipeline.py:530-532 -- and the three imd_lincomb launches plus the identity imd_ddim_cfg_step this engine spends
 * on it otherwise.  The arithmetic is one fixed sequence of fused multiply-adds, so the three forms below are bit-identical wherever
 * they describe the same step.  Errors without launching: a foreign struct_bytes, K outside 0..4, K > 0 without hist, store_m or
 * store_s outside -1..K-1 or equal and non-negative (host coefficients), a mask without z_img / blend_noise, misaligned pointers
 * (16 bytes for the float4 / uint4 tensors, 4 for mask, guidance_rows and coefs). */
int imd_unipc_step(const imd_unipc_params* p, void* stream);
/* The same step with the coefficient block read PER LATENT ROW (a denoising session).  Row b = pixel / HW reads coef_rows[b];
 * p->coefs and the scalar fields m_x .. store_s are ignored; a store slot outside 0..K-1 stores nothing.  A row whose `active` float
 * is 0 is neither read nor written: its z, its pixels of every history slot and of both CFG halves of x_next keep their bytes.
 * Errors without launching: those of imd_unipc_step (but the store checks), coef_rows NULL or not 16-byte aligned. */
#define IMD_UNIPC_ROW_FLOATS 24     /* per latent row: [0..18] the coefficient block in imd_unipc_params.coefs order,
                                       [19] active (0: the row is skipped), [20..23] reserved, 0 */
int imd_unipc_step_rows(const imd_unipc_params* p, const float* coef_rows /* DEVICE [B][24] fp32 */, void* stream);
/* imd_unipc_step_rows of a COMPACTING session, with the semantics of imd_sampler_step_rows_at.  Addressed by ROW (p->B of them): eps,
 * x_next (rows r and B + r), coef_rows and p->guidance_rows.  Addressed by SLOT (`slots` of them): z, hist (plane k starts at
 * hist + k slots HW), mask, z_img and blend_noise.  A row whose block is inactive, or whose slot is outside [0, slots), is skipped
 * whole; slots that no row names keep their bytes; two rows must not name one slot.  Errors without launching: those of
 * imd_unipc_step_rows, row_slot NULL or not 4-byte aligned, slots < 1, B > slots. */
int imd_unipc_step_rows_at(const imd_unipc_params* p, const float* coef_rows /* DEVICE [B][24] fp32 */,
                           const int* row_slot /* DEVICE [B] */, int slots, void* stream);
/* The CFG rescale of the rows that ask for it, in place on eps, as ONE launch (one workgroup per latent row) in front of any of the
 * step entry points above; see imd_guidance_rescale_params.  A scalar rescale of 0 without rescale_rows launches nothing.  Errors
 * without launching: null params, a foreign struct_bytes, eps NULL or not 16-byte aligned, guidance_rows or rescale_rows not 4-byte
 * aligned, B < 1 or HW < 1, a scalar rescale that is not finite or outside [0, 1], a scalar guidance that is not finite. */
int imd_guidance_rescale(const imd_guidance_rescale_params* p, void* stream);
/* Seeded normals (or the raw Philox words) of every active row as ONE launch (one 16-byte store per pixel, grid (pixels, rows)); see
 * imd_noise_params.  The result depends on the key row and the pixel alone: not on rows, the row position, the grid or the other
 * rows.  Errors without launching: null params, a foreign struct_bytes, out or key_rows NULL or not 16-byte aligned, rows < 1 (or
 * more than 65535), HW < 1, an unknown kind. */
int imd_noise_rows(const imd_noise_params* p, void* stream);

/* Augmented activation rows [x | s_row (x D^T)] of a per-row-scaled LoRA layer; see imd_lora_rows_params (lora_rows.hip).  Errors
 * without launching: a foreign struct_bytes, a null pointer, an unknown dtype, C or T not a multiple of 16, C outside 64..1280, T
 * outside 16..384, M != E * rows_per_entry (or any of them < 1), x_ld < C, out_ld < C + T, a leading dimension that is not a multiple of
 * 8 elements, x / down / out not 16-byte aligned, row_scale not 4-byte aligned, out overlapping x, an operand of 2 GiB or more. */
int imd_lora_expand_rows(const imd_lora_rows_params* p, void* stream);

/* Every row of every segment times its row's scale, in place, as ONE launch (16 KiB chunks numbered through all segments, see
 * residual_scale_rows.hip); see imd_scale_rows_params.  Errors without launching: null params, a foreign struct_bytes, an unknown
 * dtype, segments outside 1..16, rows < 1, scale_rows NULL or not 4-byte aligned, a row_elems that is not a positive multiple of 8,
 * a data pointer that is NULL or not 16-byte aligned, 2^31 chunks or more. */
int imd_residual_scale_rows(const imd_scale_rows_params* p, void* stream);

/* dst = the scaled sum of the sources, row by row, as ONE launch (the chunks of residual_scale_rows.hip; residual_mix_rows.hip); see
 * imd_mix_rows_params.  Errors without launching: null params, a foreign struct_bytes, an unknown dtype, sources outside 1..4, segments
 * outside 1..16, rows < 1, scales NULL or not 4-byte aligned, a row_elems that is not a positive multiple of 8, a src / dst pointer that
 * is NULL or not 16-byte aligned, 2^31 chunks or more, a dst segment that overlaps a source segment (other than dst[j] == src[k][j]) or
 * another dst segment. */
int imd_residual_mix_rows(const imd_mix_rows_params* p, void* stream);

/* Pillow-exact resize (+ crop, normalise, layout) of uint8 images on the device; see imd_image_resample_params.  Errors without
 * launching: a foreign struct size, null src / out, C outside {1, 3}, an incomplete table or a skipped axis whose size changes, a
 * crop outside the resized image, h_taps > h_kmax / v_taps > v_kmax, an unknown output kind or dtype, two launches without tmp.
 * imd_image_resample_form: the number of launches imd_image_resample would make for *p (1 | 2), 0 when it would refuse. */
int imd_image_resample(const imd_image_resample_params* p, void* stream);
int imd_image_resample_form(const imd_image_resample_params* p);
/* Decoder output -> uint8 RGB on the device; see imd_image_pack_params. */
int imd_image_pack_u8(const imd_image_pack_params* p, void* stream);
/* Inpainting result -> the person image, Image.composite per byte; see imd_image_overlay_params. */
int imd_image_overlay(const imd_image_overlay_params* p, void* stream);
/* uint8 image + mask -> the inpainting ControlNet's 16-bit NHWC8 condition; see imd_image_inpaint_condition_params. */
int imd_image_inpaint_condition(const imd_image_inpaint_condition_params* p, void* stream);
/* MaxFilter(2k + 1) then GaussianBlur of uint8 masks, Pillow's bytes; see imd_image_mask_filter_params.  Errors without launching.
 * imd_image_mask_filter_form: the number of launches imd_image_mask_filter would make for *p, 0 when it would refuse. */
int imd_image_mask_filter(const imd_image_mask_filter_params* p, void* stream);
int imd_image_mask_filter_form(const imd_image_mask_filter_params* p);
/* uint8 "L" mask window -> the uint16 release step of every latent pixel for a run of n positions, one wave per latent pixel; see
 * imd_image_mask_release_params.  Errors without launching: null params, a foreign struct_bytes, src or out NULL, h, w, H0 or W0 < 1,
 * src_row_stride < W0, n outside [1, 65535], out not 2-byte aligned, a window of 2^31 bytes or a latent of 2^30 pixels or more. */
int imd_image_mask_release(const imd_image_mask_release_params* p, void* stream);
/* The 0 / 1 blend mask of the rows that ask for it, as ONE launch in front of a step (grid (pixels, rows), four pixels per thread);
 * see imd_soft_mask_rows_params.  Errors without launching: null params, a foreign struct_bytes, release, step_rows or mask NULL,
 * release not 8-byte, step_rows not 4-byte or mask not 16-byte aligned, B < 1 (or more than 65535), HW < 1. */
int imd_soft_mask_rows(const imd_soft_mask_rows_params* p, void* stream);

/* diffusers Timesteps(dim, flip_sin_to_cos=True, freq_shift=0): out[B, dim] fp32 = [cos | sin]. */
int imd_timestep_embedding(const float* t, float* out, int B, int dim, void* stream);

/* out = a + b_scale * b over [rows, C] with row strides (ControlNet residual add,
 * ..._pipeline_ipa_controlnet.py:676-677,687-688; skip + residual). */
int imd_add(const uint16_t* a, int a_ld, const uint16_t* b, int b_ld, uint16_t* out, int out_ld, long rows, int C, float b_scale, int dtype, void* stream);
/* strided 2-D copy (channel concat of UNet skip connections). */
/* Token + position embedding lookup (CLIPTextEmbeddings): out[r][:] = table[ids[r]][:] + pos[r % T][:]; ids are int64. */
int imd_embed_tokens(const uint16_t* table, int vocab, const uint16_t* pos, int T, const int64_t* ids, uint16_t* out, long rows, int C,
                     int dtype, void* stream);
/* ViT sequence assembly (CLIPVisionEmbeddings): out[b][0] = cls + pos[0]; out[b][1 + p] = patches[b][p] + pos[1 + p]. */
int imd_vit_assemble(const uint16_t* patches, const uint16_t* cls, const uint16_t* pos, uint16_t* out, int B, int P, int C, int dtype,
                     void* stream);
/* out[i] = sum_j coefs[j] * xs[j][i] over n <= 8 fp32 tensors of `numel` elements (xs / coefs are HOST arrays; out may alias an
 * input): the latent arithmetic of the multistep UniPC sampler (x0 prediction with CFG, predictor and corrector updates). */
int imd_lincomb(const float* const* xs, const float* coefs, int n, float* out, long numel, void* stream);
int imd_copy2d(const uint16_t* a, int a_ld, uint16_t* out, int out_ld, long rows, int C, void* stream);
/* out[r, 0:Ca] = a[r, :], out[r, Ca:Ca+Cb] = b[r, :] (+ b_add[r, :] when given): torch.cat([x, skip (+ ControlNet residual)], dim=1) of
 * an up block (diffusers UNet2DConditionModel up path; ..._pipeline_ipa_controlnet.py:676-688) in one launch; contiguous rows.
 * b_rows: 0 (= rows), or a divisor of rows -- b then holds b_rows rows and row r reads b[r % b_rows] (one skip tensor serving both
 * halves of a CFG batch whose halves are identical up to that layer). */
int imd_concat2(const uint16_t* a, int Ca, const uint16_t* b, int Cb, const uint16_t* b_add, uint16_t* out, long rows, long b_rows, int dtype, void* stream);
/* imd_concat2 over B images of HW pixels that ALSO writes the GroupNorm(G) statistics of its output -- the ResnetBlock2D.norm1 that
 * follows every skip concatenation of the up path (diffusers unet_2d_blocks.py CrossAttnUpBlock2D / UpBlock2D.forward: cat, then resnet) --
 * as partial[B][imd_groupnorm_parts(B, HW, Ca + Cb)][G][2] fp32 (sum, sum of squares), the layout imd_groupnorm_params.nparts takes.
 * Same chunking and summation order as imd_groupnorm's own statistics launch on the finished tensor: bit-identical partials, one sweep
 * less.  b holds b_B images (a divisor of B; image i reads b[i % b_B]). */
int imd_concat2_gn_stats(const uint16_t* a, int Ca, const uint16_t* b, int Cb, const uint16_t* b_add, uint16_t* out, int B, int HW, int b_B, int G,
                         float* partial, int dtype, void* stream);
/* number of per-image statistic partials imd_groupnorm's own statistics launch (and imd_concat2_gn_stats) writes for this tensor; 0 if C % 8 */
int imd_groupnorm_parts(int B, int HW, int C);
/* FreeU (Si et al., CVPR 2024; diffusers 0.24 apply_freeu / fourier_filter) inside the skip concatenation of an up block, one launch:
 *   out[.., c]      = round16(a[.., c] * backbone_scale)                 c < Ca / 2        (one product, one rounding)
 *   out[.., c]      = a[.., c]                                           Ca / 2 <= c < Ca
 *   out[.., Ca + c] = round16(filter(v)[.., c]),  v = round16(b + b_add) (imd_concat2's sum; v = b when b_add is NULL)
 * for NHWC tensors a [B, H, W, Ca], b and b_add [B, H, W, Cb].  filter = fourier_filter(threshold 1, scale skip_scale) per (image, channel)
 * map in its closed form -- y = v + (skip_scale - 1) / (H W) * sum over the waves (mean; row 2 pi n / H when H > 1; column 2 pi m / W when
 * W > 1; the diagonal 2 pi (n / H + m / W) when both) of A cos(phi) + B sin(phi), A = sum v cos(phi), B = sum v sin(phi) -- in fp32, no FFT.
 * part non-NULL: also the GroupNorm(G) (sum, sum of squares) partials of the ROUNDED values stored, as
 * part[B][imd_concat2_freeu_parts(B, H, W, Ca, Cb, G)][G][2] fp32, the layout imd_groupnorm_params.nparts takes; every float is written.
 * Refused without a launch: a null a, b or out; Ca % 16 or Cb % 8; B, H or W < 1; H or W > 256 (the twiddle table); B > 65535; b_batch != B
 * (every image filters its own skip); (Ca + Cb) % G, G > 64 or 5 .. 7 channels per group with part given; an unknown dtype; a, b, b_add or out
 * not 16-byte aligned (part: 4-byte); a scale that is not finite or <= 0.  skip_scale = 1 and backbone_scale = 1 store imd_concat2's bits. */
int imd_concat2_freeu(const uint16_t* a, int Ca, const uint16_t* b, int Cb, const uint16_t* b_add, uint16_t* out, int B, int H, int W, int b_batch, int G,
                      float* part, float backbone_scale, float skip_scale, int dtype, void* stream);
/* pure query: statistic partials per (image, group) imd_concat2_freeu writes for this tensor; 0 = it cannot produce the statistics (pass part = NULL) */
int imd_concat2_freeu_parts(int B, int H, int W, int Ca, int Cb, int G);
/* fp32 -> 16-bit element cast (round to nearest even). */
int imd_f32_to_16(const float* a, uint16_t* out, long n, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMAGDRESSING_HIP_H */
