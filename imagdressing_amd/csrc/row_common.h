// Building blocks of the row-resident kernel family (row_linear.hip, row_linear_k640.hip, row_linear_k1280.hip, row_qkv.hip,
// ff_fused.hip, row_xattn.hip): a wave keeps its token rows in registers as MFMA B-operand fragments for the whole kernel and
// the weights stream past them through a three-slot ring in LDS, filled by LDS-DMA.  What is specific to a member -- how it
// cuts rows, K and output channels over waves and workgroups, and why -- is told at the head of its file; the blocks every
// member repeats live here, each with its explanation.
//
// RULE: these helpers only move text.  A kernel uses one only if it compiles to the same instructions as with the block
// written out (compare the device assembly); where it does not, the kernel keeps the block inline and says so in one line.
// Arrays are taken by reference and every opaque touch stays a statement of its own: both decide what hipcc emits.  So does
// the shape of a helper: where a form below looks roundabout (one piece or one fragment per call with the loop at the caller, a
// uint4 by value), the straighter form moved instructions or registers in one of the kernels.
#pragma once
#include "gemm_common.h"
#include "lds_dma.h"

namespace {

typedef __attribute__((__vector_size__(2 * sizeof(uint32_t)))) uint32_t v2u;      // (v4u: gemm_common.h)

// ---- the weight ring: 3 slots of 40 KB; a chunk is fetched by the 8 waves as 5 pieces of 1 KB each (piece q of the chunk
// lands at LDS bytes [1024 q, + 1024) of its slot) ----
constexpr int ROW_RING = 3;
constexpr int ROW_CHUNK = 40960;
constexpr int ROW_PIECES = ROW_CHUNK / (8 * 1024);      // 5: the counted waits of the chunk loops are dma_wait_keep_n<ROW_PIECES>()

// ------------------------------------------------------------------------------------------
// row fragments
// ------------------------------------------------------------------------------------------
// Opaque touch of a fragment array (pin_row: of one fragment).  Two uses:
//   * behind the first ring_stage calls: hipcc counts only its own (activation) loads, so this pins their wait THERE, where
//     it also covers chunks 0 and 1 that were requested with them, instead of in front of the last MFMA of chunk 0 where it
//     would drain chunk 2 as well;
//   * between the passes of the LayerNorm: keeps hipcc from holding all unpacked values of the row alive across the passes.
template <int S>
__device__ __forceinline__ void pin_rows(uint4 (&xf)[S]) {
#pragma unroll
    for (int s = 0; s < S; ++s) asm volatile("" : "+v"(xf[s].x), "+v"(xf[s].y), "+v"(xf[s].z), "+v"(xf[s].w));
}
__device__ __forceinline__ void pin_row(uint4& x) { asm volatile("" : "+v"(x.x), "+v"(x.y), "+v"(x.z), "+v"(x.w)); }

// A lane's S fragments of its row: 16 bytes at `off`, `off + stride`, ... (stride 32 = the k-step of the 32x32x16 MFMA, 64 = of
// the 16x16x32 one), requested back to back; rows past the end (`valid` false) read as zero.
template <int S>
__device__ __forceinline__ void load_rows(uint4 (&xf)[S], const __amdgpu_buffer_rsrc_t& rs, bool valid, uint32_t off, int stride) {
#pragma unroll
    for (int s = 0; s < S; ++s) xf[s] = buf_load16(rs, valid ? off + s * stride : OOB);
}

// ---- LayerNorm (no affine: folded into the weights by the caller) of the rows in place, two-pass fp32.  Each pass goes over
// the packed fragments again; pin_rows between the passes (see there).  What a lane holds is a PART of a row: the caller
// completes sum and squared deviations over the lanes / waves that share the row. ----
template <bool F16, int S>
__device__ __forceinline__ float rows_sum(const uint4 (&xf)[S]) {
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        float f[8];
        unpack8<F16>(xf[s], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += f[e];
    }
    return sum;
}
template <bool F16, int S>
__device__ __forceinline__ float rows_sqdev(const uint4 (&xf)[S], float mean) {
    float sq = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        float f[8];
        unpack8<F16>(xf[s], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = f[e] - mean; sq = fmaf(d, d, sq); }
    }
    return sq;
}
template <bool F16, int S>
__device__ __forceinline__ void rows_scale_shift(uint4 (&xf)[S], float rstd, float shift) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        float f[8];
        unpack8<F16>(xf[s], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = fmaf(f[e], rstd, shift);
        xf[s] = pack8<F16>(f);
    }
}
// the whole of it where lanes l and l ^ 32 share a row of K channels (the K = 320 kernels).  (pin_row in loops, not pin_rows: that
// nesting moved an instruction in one instantiation of row_linear.hip)
template <bool F16, int K, int S>
__device__ __forceinline__ void ln_rows_inplace(uint4 (&xf)[S], float eps) {
    float sum = rows_sum<F16>(xf);
    sum += __shfl_xor(sum, 32);
    const float mean = sum * (1.0f / K);
#pragma unroll
    for (int s = 0; s < S; ++s) pin_row(xf[s]);
    float sq = rows_sqdev<F16>(xf, mean);
    sq += __shfl_xor(sq, 32);
    const float rstd = rsqrtf(sq * (1.0f / K) + eps);
    const float shift = -mean * rstd;
#pragma unroll
    for (int s = 0; s < S; ++s) pin_row(xf[s]);
    rows_scale_shift<F16>(xf, rstd, shift);
}

// ------------------------------------------------------------------------------------------
// weight ring
// ------------------------------------------------------------------------------------------
// Source offset of this lane's piece j (of five) of a chunk whose rows (first row n0 of the matrix) are PPR 16-byte pieces long.
// Rows are stored unpadded in LDS with piece `pos` of row r at pos ^ ((r >> SW_SHIFT) & SW_MASK), applied here on the SOURCE
// side (a DMA piece is lane-linear in LDS): that makes the ds_read_b128 fragment reads conflict-free.  <40, 1, 7> for 640-byte
// rows, <80, 0, 15> / <160, 0, 15> for 1280- / 2560-byte rows.
template <int PPR, int SW_SHIFT, int SW_MASK>
__device__ __forceinline__ uint32_t ring_offset(int j, int wave, int lane, int n0 = 0) {
    const int q = (j * 8 + wave) * 64 + lane;
    const int row = q / PPR, pos = q - row * PPR;
    return (uint32_t)((n0 + row) * (PPR * 16) + ((pos ^ ((row >> SW_SHIFT) & SW_MASK)) << 4));
}
// chunk c of the matrix into slot c % 3 (lds0 = LDS aperture offset of the ring)
__device__ __forceinline__ void ring_stage(const v4i_t& ds_w, uint32_t lds0, int wave, const uint32_t (&woff)[ROW_PIECES], int c) {
    const uint32_t base = lds0 + (uint32_t)((c % ROW_RING) * ROW_CHUNK) + (uint32_t)wave * 1024u;
#pragma unroll
    for (int j = 0; j < ROW_PIECES; ++j) dma16(ds_w, base + j * 8192u, woff[j] + (uint32_t)c * ROW_CHUNK);
}

// ------------------------------------------------------------------------------------------
// direct epilogue
// ------------------------------------------------------------------------------------------
// WIDE stores: the accumulator layout of the 32x32 MFMA gives a lane 4 channels of a row, so an 8-byte store instruction puts
// 16 contiguous bytes into each of 32 rows -- fragments the L2 takes at its REQUEST rate (measured on the GEMM epilogues:
// 16-byte fragments drain at 2.5 TB/s, a plain fill writes at 6.2, profiles/r5d_write_bw_probe.jsonl).  One v_permlane32_swap
// per packed register pair turns two 4-channel groups (a: channels 4 hi .. + 3, b: 8 + 4 hi .. + 3 of a 16-channel block; hi =
// lane >> 5) into 8 consecutive channels 8 hi .. + 7 per lane: half as many store requests, 32 contiguous bytes per row.
__device__ __forceinline__ v4u quads_to_wide(const v2u& a, const v2u& b) {
    const auto r0 = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
    return v4u{r0[0], r1[0], r0[1], r1[1]};
}
// the inverse, for a residual loaded as 8 consecutive channels: (x, y) = group a, (z, w) = group b of the accumulator layout
__device__ __forceinline__ uint4 wide_to_quads(uint4 r) {
    const auto sx = __builtin_amdgcn_permlane32_swap(r.x, r.z, false, false);
    const auto sy = __builtin_amdgcn_permlane32_swap(r.y, r.w, false, false);
    return make_uint4(sx[0], sy[0], sx[1], sy[1]);
}

// head-split Q destination (p.hd[0], [B, H, L, DP] row-major per head): byte offset of channel n relative to (image, head 0, token)
// of its row.  (That row base stays written out in the three kernels that need it: from a helper, in whatever form it takes its
// arguments, hipcc commutes the operands of its 64-bit multiply.)
__device__ __forceinline__ uint32_t heads_channel_offset(const ConvGemmParams& p, int n) {
    const int h = n / p.hD, dd = n - h * p.hD;
    return (uint32_t)((h * p.hd[0].L * p.hd[0].DP + dd) * 2);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// can the output leave straight from the accumulators?  (16-bit row-major or head-split Q; bias / scale / residual only)
inline bool row_direct_epilogue(const ConvGemmParams& p) {
    return p.act == ACT_NONE && !p.out_f32 && p.rowvec == nullptr &&
           (p.mode == OUT_ROWMAJOR || (p.hd[0].kind == 0 && p.hd[0].ptr != nullptr && p.N == p.hC));
}
// the direct epilogues address output and residual with 31-bit byte offsets
inline bool row_out_below_2g(const ConvGemmParams& p) {
    const size_t ob = p.mode == OUT_HEADS ? (size_t)(p.M / (p.Hout * p.Wout)) * p.hH * p.hd[0].L * p.hd[0].DP * 2 : ((size_t)(p.M - 1) * p.out_ld + p.N) * 2;
    const size_t rb = p.res ? ((size_t)(p.M - 1) * p.res_ld + p.N) * 2 : 0;
    return ob < 0x80000000ull && rb < 0x80000000ull;
}
// sizes of the two buffer descriptors (32 bits); refuses in the kernel's name, `why` = its wording
inline int row_operand_bytes(ConvGemmParams& p, const char* name, const char* why = "operand too large") {
    const size_t xb = ((size_t)(p.M - 1) * p.x_pix_stride + p.K) * 2, wb = (size_t)p.N * p.K * 2;
    if (xb >= 0xffffffffull) return imd_set_error("%s: %s", name, why);
    p.x_bytes = (uint32_t)xb;
    p.w_bytes = (uint32_t)wb;
    return 0;
}

// ---- the K = 640 / K = 1280 members: workgroups of BM rows x 160 output channels, direct epilogue only ----
constexpr int ROW_NG = 160;
using RowLaunchFn = int (*)(const ConvGemmParams&, float, hipStream_t);

template <int K>
inline bool row_wide_supported(const ConvGemmParams& p) {
    return row_direct_epilogue(p) && p.taps == 1 && p.K == K && p.Cin == K && p.stride == 1 && !p.ups && p.Hin == p.Hout && p.Win == p.Wout &&
           p.N >= ROW_NG && (p.N % ROW_NG) == 0 && p.split_k <= 1 && p.gn_a == nullptr && (p.x_pix_stride % 8) == 0 &&
           (p.mode != OUT_HEADS || (p.hD % 4) == 0);
}
// grid: whole row blocks per XCD (the kernels undo it: hardware workgroup b runs on XCD b % 8)
template <int BM, typename Kern>
int row_wide_launch_kernel(Kern kern, int lds, const char* name, const ConvGemmParams& p, float eps, hipStream_t s) {
    if (int rc_attr = imd_lds_attr(reinterpret_cast<const void*>(kern), lds, name)) return rc_attr;
    const unsigned grid = (unsigned)((((p.M + BM - 1) / BM + 7) / 8) * 8 * (p.N / ROW_NG));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, s, p, eps);
    return imd_check_launch(name);
}
// kern[0 GroupNorm prologue | 1 LayerNorm prologue | 2 neither][0 fp16 | 1 bf16]; flags = the kernel's p.flags
template <int K, int BM>
int row_wide_launch(const ConvGemmParams& p_in, int ln, float ln_eps, hipStream_t s, const char* name, int flags, const RowLaunchFn (&kern)[3][2]) {
    ConvGemmParams p = p_in;
    if (p_in.res_rows != 0) return imd_set_error("%s: a periodic residual (res_rows) exists in the K = 320 row-resident projection only", name);
    if (!row_wide_supported<K>(p))
        return imd_set_error("%s: needs a plain linear layer with K = %d, N a multiple of 160 and a bias / scale / residual epilogue "
                             "(got N=%d K=%d taps=%d act=%d)", name, K, p.N, p.K, p.taps, p.act);
    if (p.dtype != IMD_DTYPE_BF16 && p.dtype != IMD_DTYPE_F16) return imd_set_error("%s: unknown dtype %d", name, p.dtype);
    if (int rc = row_operand_bytes(p, name)) return rc;
    if (!row_out_below_2g(p)) return imd_set_error("%s: operand too large", name);
    p.split_k = 1;
    p.flags = flags;
    if (p.gn_in_partial != nullptr && (ln || !gn_in_ok(p, K, BM)))
        return imd_set_error("%s: gn_in_* needs K = %d, K %% groups == 0, groups <= 64, H W %% %d == 0 and no LayerNorm prologue (ask imd_row_linear_gn_in_supported())", name, K, BM);
    return kern[p.gn_in_partial != nullptr ? 0 : ln ? 1 : 2][p.dtype == IMD_DTYPE_F16 ? 0 : 1](p, ln_eps, s);
}

}  // namespace
