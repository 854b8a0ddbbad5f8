// Text cross-attention of a 320-channel transformer block (64x64 level) as ONE row-resident launch:
//
//   out[m, :] = x[m, :] + b_o + W_o . concat_h( softmax(q_h Kt_h^T) Vt_h ),      q = LN(x[m, :]) . W_q'^T + b_q'
//
// = BasicTransformerBlock.norm2 -> attn2.to_q -> scaled-dot-product attention over the <= 96 text keys of the row's
// conditioning -> attn2.to_out[0] + bias + block residual (diffusers==0.24.0 BasicTransformerBlock, un-vendored; reference
// call sites adapter/attention_processor.py:568 (to_q), :589-612 (attention), :617 (to_out)).  The chain is row-local, so
// Q, P and O never exist in memory: the launch reads x and writes the block output.
//
// Row-resident scheme (row_common.h), geometry = row_linear.hip: 512 threads own 128 token rows; wave (rb, chh) keeps ITS 32 rows x 320 channels in 80 VGPRs
// in MFMA B-operand layout (LayerNorm prologue in registers, affine folded into W_q' / b_q' by the caller) and everything
// else streams through a 3 x 40 KB LDS ring by LDS-DMA as ONE sequence of 15 chunks, one barrier per chunk:
//   chunks 0..5   W_q' with every head padded to 48 rows: wave half chh owns heads 4 chh .. 4 chh + 3 (192 rows = six 32-row
//                 blocks); a block's accumulators are scaled, rounded and turned into two B-operand fragments of
//                 S^T = Kt q^T by the v_permlane32_swap pair of the wide epilogue -- q never touches LDS;
//   chunks 6..9   text K / V^T images of the head pair (p, p + 4), built once per conditioning by the host exactly as they sit
//                 in LDS (ops.pack_text_kv): K [96 keys][48 dims] (column 40 = 0 for a key, a large negative value for a pad
//                 key; q's slot 40 is 1), V^T [48][96 keys] with an all-ones row 40 (softmax denominator through the P.V
//                 MFMA) and the key columns ordered like the accumulator registers of S^T, so that exp2'd, packed scores ARE
//                 the B operand of O^T += V^T P^T.  All keys of a head are resident: the row maximum is exact, there is no
//                 deferred maximum and no overflow path.  The two waves of a row block swap their heads' O (16-bit) through a
//                 double-buffered 20 KB exchange area, published by the next chunk's barrier;
//   chunks 10..14 W_o with its input channels ordered like the O registers (ops.pack_text_xattn), multiplied against the 20
//                 O fragments; every 32 x 32 block leaves through the wide direct epilogue of row_linear.hip (bias from LDS,
//                 residual = the un-normalised x re-read from L2 one chunk ahead) while the next chunk is multiplied.
// 16-bit rounding points (the same four as the three-launch path): q (after bias and scale), P = exp2(s - max), O = sum / l,
// out.  All chunk images carry their LDS swizzle on the source side: every DMA piece is a linear 1 KB copy.
#include "row_common.h"

namespace {

constexpr int XA_C = 320;
constexpr int XA_STEPS = XA_C / 16;                 // 20 MFMA k-steps of the two projections
constexpr int XA_ROWB = XA_C * 2;                   // bytes per weight row
constexpr int XA_CHUNK = 64 * XA_ROWB;              // 40960: one ring slot
constexpr int XA_PIECES = ROW_PIECES;               // DMA pieces per wave per chunk: 5
constexpr int XA_RING = ROW_RING;
constexpr int XA_BM = 128;
constexpr int XA_NQ = 6, XA_NKV = 4, XA_NO = 5;     // chunks of the three stages
constexpr int XA_NCHUNK = XA_NQ + XA_NKV + XA_NO;
constexpr int XA_LMAX = 96;                         // text keys resident per head
constexpr int XA_KROW = 96;                         // bytes per K row (48 dims): six 16-byte pieces, rows 8..15 (mod 16) rotated by three
constexpr int XA_VROW = 208;                        // bytes per V^T row: 12 pieces of keys + 1 of padding (odd piece count: conflict-free as is)
constexpr int XA_KBYTES = XA_LMAX * XA_KROW;        // 9216
constexpr int XA_HEADB = XA_KBYTES + 48 * XA_VROW;  // 19200 bytes per head; a chunk = heads (p, p + 4) + padding
constexpr int XA_XB = 8 * 5 * 512;                  // O exchange buffer of one head: 8 waves x 5 channel groups x 64 lanes x 8 bytes
constexpr int XA_OFF_X = XA_RING * XA_CHUNK;        // exchange area (2 buffers); its first bytes hold b_q' during the Q stage and b_o during the out stage
constexpr int XA_LDS = XA_OFF_X + 2 * XA_XB;        // 163840: all of a CU's LDS
static_assert(XA_CHUNK == ROW_CHUNK, "the ring of the family: 40 KB chunks in five pieces per wave");
static_assert(2 * XA_HEADB <= XA_CHUNK && XA_LDS <= 160 * 1024, "LDS budget");
static_assert(64 * XA_NQ * 4 <= XA_XB && XA_C * 4 <= XA_XB, "bias tables live in the exchange area");

template <bool F16>
__global__ __launch_bounds__(512, 1) void text_xattn320_kernel(const imd_xattn_params p) {
    using E = El<F16>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, col = lane & 31;
    const int rb = wave & 3;            // 32-token block of the workgroup's 128 rows
    const int chh = wave >> 2;          // heads 4 chh .. 4 chh + 3; 32-channel half of every 64-channel weight chunk
    const int m0 = blockIdx.x * XA_BM;

    // ---- activations: this wave's 32 rows, all 320 channels, straight into B-operand fragments ----
    const uint32_t x_bytes = (uint32_t)(((size_t)(p.M - 1) * p.x_ld + XA_C) * 2);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.x), 0, x_bytes, 0x00020000);
    const int m = m0 + rb * 32 + col;
    const uint32_t xoff = (uint32_t)m * (uint32_t)(p.x_ld * 2) + hi * 16;
    uint4 xf[XA_STEPS];
    load_rows(xf, rs_x, m < p.M, xoff, 32);
    float bq_v = 0.f, bo_v = 0.f;      // requested behind the activation rows; parked in LDS when their stage begins
    if (tid < 64 * XA_NQ) bq_v = p.bq[tid];
    if (tid < XA_C) bo_v = p.bo[tid];

    // ---- operand stream: chunk c of the sequence W_q' (6) | K / V^T images of this workgroup's conditioning (4) | W_o (5) ----
    const int tb = (m0 / p.rows_per_image) / p.kv_bdiv;                      // text batch row of the workgroup's image
    const v4i_t ds_w = raw_rsrc(p.w, (uint32_t)((XA_NQ + XA_NO) * XA_CHUNK));
    const v4i_t ds_kv = raw_rsrc(reinterpret_cast<const char*>(p.kv) + (size_t)tb * XA_NKV * XA_CHUNK, (uint32_t)(XA_NKV * XA_CHUNK));
    const uint32_t loff = (uint32_t)wave * 1024u + (uint32_t)lane * 16u;     // piece j of a chunk: bytes [8192 j + loff, + 16) -> the same LDS bytes
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    auto stage = [&](int c) {
        const uint32_t base = lds0 + (uint32_t)((c % XA_RING) * XA_CHUNK) + (uint32_t)wave * 1024u;
        const bool kvc = c >= XA_NQ && c < XA_NQ + XA_NKV;
        const uint32_t src = loff + (uint32_t)((kvc ? c - XA_NQ : c < XA_NQ ? c : c - XA_NKV) * XA_CHUNK);
#pragma unroll
        for (int j = 0; j < XA_PIECES; ++j) dma16(kvc ? ds_kv : ds_w, base + j * 8192u, src + j * 8192u);
    };
    stage(0);
    stage(1);
    pin_rows(xf);
    float* bias_s = reinterpret_cast<float*>(smem + XA_OFF_X);
    if (tid < 64 * XA_NQ) bias_s[tid] = bq_v;                                // published by the first barrier of the chunk loop

    ln_rows_inplace<F16, XA_C>(xf, p.ln_eps);      // norm2 (affine folded into W_q' / b_q' by the caller)

    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int wrow = chh * 32 + col;                                     // weight row inside a chunk
    const uint32_t a16 = (uint32_t)((hi ^ ((wrow >> 1) & 7)) << 4);      // piece 2s + hi of row wrow sits at ((2s) ^ (hi ^ f)) * 16
    const char* wlane = smem + wrow * XA_ROWB;

    // ---- stage 1: q of this wave's four heads (12 B-operand fragments: head hl = fragment / 3, dims 16 (fragment % 3) + 8 hi .. + 7) ----
    uint4 qf[2 * XA_NQ];
#pragma unroll
    for (int c = 0; c < XA_NQ; ++c) {
        dma_wait_keep_n<XA_PIECES>();                                         // this wave's pieces of chunk c have landed (chunk c + 1 may still fly)
        __syncthreads();                                          // ... and everybody else's; all waves are done with chunk c - 1
        stage(c + 2);
        const char* Ws = wlane + (c % XA_RING) * XA_CHUNK;
        f32x16 acc = zero16;
#pragma unroll
        for (int s = 0; s < XA_STEPS; ++s) {
            const uint4 wf = *reinterpret_cast<const uint4*>(Ws + ((uint32_t)(s * 32) ^ a16));
            acc = E::mfma(wf, xf[s], acc);
        }
        v2u pk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 bb = *reinterpret_cast<const float4*>(bias_s + c * 64 + chh * 32 + 8 * j + 4 * hi);
            pk[j] = v2u{E::pack2((acc[4 * j] + bb.x) * p.q_scale, (acc[4 * j + 1] + bb.y) * p.q_scale),
                        E::pack2((acc[4 * j + 2] + bb.z) * p.q_scale, (acc[4 * j + 3] + bb.w) * p.q_scale)};
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {      // groups 2 t, 2 t + 1 (4 rows each per lane half) -> rows 16 t + 8 hi + 0..7 of the block
            const v4u w = quads_to_wide(pk[2 * t], pk[2 * t + 1]);
            qf[2 * c + t] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    // q slot 40 of every head = 1: it meets K column 40 (0 for a key, a large negative value for a pad key)
    {
        const uint32_t one = (uint32_t)E::fromf(1.0f);
#pragma unroll
        for (int hl = 0; hl < 4; ++hl)
            if (hi == 1) qf[3 * hl + 2].x = (qf[3 * hl + 2].x & 0xffff0000u) | one;
    }

    // ---- stage 2: attention of head 4 chh + hl over the resident text keys, hl = 0..3 ----
    uint2 og[4][5], pg[4][5];       // O (16-bit) of this wave's / the partner wave's heads: group j = dims 8 j + 4 hi .. + 3
    const int krot = 3 * ((col >> 3) & 1);
    const char* xown = smem + XA_OFF_X + wave * (5 * 512) + lane * 8;
    const char* xpar = smem + XA_OFF_X + (wave ^ 4) * (5 * 512) + lane * 8;
#pragma unroll
    for (int hl = 0; hl < XA_NKV; ++hl) {
        const int c = XA_NQ + hl;
        dma_wait_keep_n<XA_PIECES>();
        __syncthreads();
        stage(c + 2);
        if (hl > 0) {
#pragma unroll
            for (int j = 0; j < 5; ++j) pg[hl - 1][j] = *reinterpret_cast<const uint2*>(xpar + ((hl - 1) & 1) * XA_XB + j * 512);
        }
        const char* Ks = smem + (c % XA_RING) * XA_CHUNK + chh * XA_HEADB;
        const char* Vs = Ks + XA_KBYTES;
        f32x16 sc[3];
#pragma unroll
        for (int kb = 0; kb < 3; ++kb) {
            sc[kb] = zero16;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const uint4 kf = *reinterpret_cast<const uint4*>(Ks + (kb * 32 + col) * XA_KROW + ((2 * t + hi + krot) % 6) * 16);
                sc[kb] = E::mfma(kf, qf[3 * hl + t], sc[kb]);
            }
        }
        float mx = sc[0][0];
#pragma unroll
        for (int kb = 0; kb < 3; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[kb][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        f32x16 o0 = zero16, o1 = zero16;     // O^T rows 0..31 / 32..47 (row 40 = softmax denominator; rows 48..63 repeat 32..47, unread)
#pragma unroll
        for (int kb = 0; kb < 3; ++kb)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                uint4 pf;
                pf.x = E::pack2(__builtin_amdgcn_exp2f(sc[kb][8 * g + 0] - mx), __builtin_amdgcn_exp2f(sc[kb][8 * g + 1] - mx));
                pf.y = E::pack2(__builtin_amdgcn_exp2f(sc[kb][8 * g + 2] - mx), __builtin_amdgcn_exp2f(sc[kb][8 * g + 3] - mx));
                pf.z = E::pack2(__builtin_amdgcn_exp2f(sc[kb][8 * g + 4] - mx), __builtin_amdgcn_exp2f(sc[kb][8 * g + 5] - mx));
                pf.w = E::pack2(__builtin_amdgcn_exp2f(sc[kb][8 * g + 6] - mx), __builtin_amdgcn_exp2f(sc[kb][8 * g + 7] - mx));
                const int pc = (2 * (2 * kb + g) + hi) * 16;
                const uint4 v0 = *reinterpret_cast<const uint4*>(Vs + col * XA_VROW + pc);
                const uint4 v1 = *reinterpret_cast<const uint4*>(Vs + (32 + (col & 15)) * XA_VROW + pc);
                o0 = E::mfma(v0, pf, o0);
                o1 = E::mfma(v1, pf, o1);
            }
        const float inv = 1.0f / __shfl(o1[4], col);      // row 40 = register 4 of the lower lane half
#pragma unroll
        for (int j = 0; j < 4; ++j)
            og[hl][j] = make_uint2(E::pack2(o0[4 * j] * inv, o0[4 * j + 1] * inv), E::pack2(o0[4 * j + 2] * inv, o0[4 * j + 3] * inv));
        og[hl][4] = make_uint2(E::pack2(o1[0] * inv, o1[1] * inv), E::pack2(o1[2] * inv, o1[3] * inv));
        // (buffer hl & 1 was last read behind the barrier of chunk c - 1; its readers have all passed the barrier of chunk c)
#pragma unroll
        for (int j = 0; j < 5; ++j) *reinterpret_cast<uint2*>(const_cast<char*>(xown) + (hl & 1) * XA_XB + j * 512) = og[hl][j];
    }

    // ---- stage 3: to_out + bias + residual.  B fragment s = channel groups 2 s, 2 s + 1 of the list (head h, group j) -> 5 h + j ----
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, 0x80000000u, 0x00020000);
    const uint32_t obase = m < p.M ? (uint32_t)m * (uint32_t)(p.out_ld * 2) : OOB;
    const uint32_t roff = (uint32_t)m * (uint32_t)(p.x_ld * 2) + (uint32_t)(chh * 64);
    uint4 rraw[2][2];               // residual of a chunk: 8 consecutive channels per load, consumed one chunk later
    auto load_res = [&](int c) {
#pragma unroll
        for (int t = 0; t < 2; ++t) rraw[c & 1][t] = buf_load16(rs_x, m < p.M ? roff + (uint32_t)(c * 128 + t * 32 + hi * 16) : OOB);
    };
    f32x16 acc[XA_NO];
    auto emit = [&](int c) {
        uint2 rres[4];              // residual in accumulator layout: group j = channels 8 j + 4 hi .. + 3
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint4 r = wide_to_quads(rraw[c & 1][t]);
            rres[2 * t] = make_uint2(r.x, r.y); rres[2 * t + 1] = make_uint2(r.z, r.w);
        }
        v2u pk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 bb = *reinterpret_cast<const float4*>(bias_s + c * 64 + chh * 32 + 8 * j + 4 * hi);
            const float v0 = acc[c][4 * j] + bb.x + E::lo(rres[j].x), v1 = acc[c][4 * j + 1] + bb.y + E::hi(rres[j].x);
            const float v2 = acc[c][4 * j + 2] + bb.z + E::lo(rres[j].y), v3 = acc[c][4 * j + 3] + bb.w + E::hi(rres[j].y);
            pk[j] = v2u{E::pack2(v0, v1), E::pack2(v2, v3)};
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const v4u w = quads_to_wide(pk[2 * t], pk[2 * t + 1]);
            const uint32_t off = (uint32_t)((c * 64 + chh * 32 + 16 * t + 8 * hi) * 2);
            __builtin_amdgcn_raw_buffer_store_b128(w, rs_o, (int)(obase == OOB ? OOB : obase + off), 0, 0);
        }
    };
    uint4 of[XA_STEPS];
#pragma unroll
    for (int co = 0; co < XA_NO; ++co) {
        const int c = XA_NQ + XA_NKV + co;
        // stores and residual loads are in flight next to the DMA pieces and do not retire in order with them: drain (row_linear.hip)
        dma_wait();
        __syncthreads();
        if (co == 0) {
#pragma unroll
            for (int j = 0; j < 5; ++j) pg[3][j] = *reinterpret_cast<const uint2*>(xpar + XA_XB + j * 512);
            if (tid < XA_C) bias_s[tid] = bo_v;       // exchange buffer 0 was last read behind the previous barrier; published by the next one
#pragma unroll
            for (int s = 0; s < XA_STEPS; ++s) {
                uint2 g2[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int G = 2 * s + e, h = G / 5, j = G % 5;
                    const uint2 mine = og[h & 3][j], theirs = pg[h & 3][j];
                    const bool own = (h >> 2) == chh;
                    g2[e] = make_uint2(own ? mine.x : theirs.x, own ? mine.y : theirs.y);
                }
                of[s] = make_uint4(g2[0].x, g2[0].y, g2[1].x, g2[1].y);
            }
        }
        if (co > 0) emit(co - 1);
        if (c + 2 < XA_NCHUNK) stage(c + 2);
        load_res(co);
        const char* Ws = wlane + (c % XA_RING) * XA_CHUNK;
        acc[co] = zero16;
#pragma unroll
        for (int s = 0; s < XA_STEPS; ++s) {
            const uint4 wf = *reinterpret_cast<const uint4*>(Ws + ((uint32_t)(s * 32) ^ a16));
            acc[co] = E::mfma(wf, of[s], acc[co]);
        }
    }
    emit(XA_NO - 1);
}

}  // namespace

bool imd_text_xattn320_supported_of(const imd_xattn_params& p) {
    return p.C == XA_C && p.heads == 8 && p.L >= 1 && p.L <= XA_LMAX && p.M > 0 && p.rows_per_image > 0 && (p.rows_per_image % XA_BM) == 0 &&
           (p.M % p.rows_per_image) == 0 && p.kv_bdiv >= 1 && p.text_rows >= 1 && (p.M / p.rows_per_image) == p.text_rows * p.kv_bdiv &&
           p.x_ld >= XA_C && (p.x_ld % 8) == 0 && p.out_ld >= XA_C && (p.out_ld % 8) == 0 &&
           (p.dtype == IMD_DTYPE_BF16 || p.dtype == IMD_DTYPE_F16);
}

int imd_launch_text_xattn320(const imd_xattn_params& p, hipStream_t s) {
    if (!imd_text_xattn320_supported_of(p))
        return imd_set_error("text_xattn320: needs C = 320, 8 heads, 1..96 text keys, rows per image a multiple of 128 and M / rows_per_image == text_rows * kv_bdiv "
                             "(got C=%d heads=%d L=%d M=%d rows_per_image=%d text_rows=%d kv_bdiv=%d x_ld=%d out_ld=%d dtype=%d)",
                             p.C, p.heads, p.L, p.M, p.rows_per_image, p.text_rows, p.kv_bdiv, p.x_ld, p.out_ld, p.dtype);
    if (((size_t)(p.M - 1) * p.x_ld + XA_C) * 2 >= 0x80000000ull || ((size_t)(p.M - 1) * p.out_ld + XA_C) * 2 >= 0x80000000ull)
        return imd_set_error("text_xattn320: operand larger than 2 GiB");
    if (!(p.ln_eps > 0.f)) return imd_set_error("text_xattn320: LayerNorm needs eps > 0");
    const bool h = p.dtype == IMD_DTYPE_F16;
    const void* kern = h ? reinterpret_cast<const void*>(text_xattn320_kernel<true>) : reinterpret_cast<const void*>(text_xattn320_kernel<false>);
    if (int rc_attr = imd_lds_attr(kern, XA_LDS, "text_xattn320")) return rc_attr;
    const dim3 grid((unsigned)(p.M / XA_BM));
    if (h) hipLaunchKernelGGL(text_xattn320_kernel<true>, grid, dim3(512), XA_LDS, s, p);
    else hipLaunchKernelGGL(text_xattn320_kernel<false>, grid, dim3(512), XA_LDS, s, p);
    return imd_check_launch("text_xattn320");
}
