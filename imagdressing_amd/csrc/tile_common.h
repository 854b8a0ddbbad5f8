// Building blocks of the tiled GEMM / implicit-GEMM family (conv_gemm.hip, gemm_dma.hip, gemm_dma256.hip), from which the halo-patch
// kernels (patch_common.h includes this file) and the row-resident kernels (row_common.h) were copied: a workgroup owns a BM x BN output
// tile, K runs past it in BK-deep operand tiles staged in LDS (through registers, or by LDS-DMA into unpadded swizzled rows), the waves
// multiply 32 x 32 blocks with 16-deep MFMA steps, and the fp32 tile leaves through LDS as 8 consecutive channels per thread
// (gemm_common.h::epilogue8).  A member's tile and schedule are told at the head of its file; the blocks every member repeats live here.
//
// RULE: these helpers only move text.  A kernel uses one only if it compiles to the same instructions as
// with the block written out (compare the device assembly); where it does not, the kernel keeps the block inline and says so in one
// line.  hipcc's output follows a helper's shape: what is here is the shape that kept every user's assembly.  (What stayed written out, and
// the assembly diffs that kept it there: DESIGN.md section 2.2e.)
#pragma once
#include "gemm_common.h"
#include "lds_dma.h"

namespace {

// ---- row swizzle of the LDS-DMA operand tiles.  A DMA piece lands lane-linear, so operand rows cannot be padded: rows of ROWB bytes lie
// back to back and piece c (16 bytes) of row r is stored at position c ^ lds_row_swz<ROWB>(r), applied on the SOURCE side (the lane
// that fills slot s of a row fetches piece s ^ swz).  A ds_read_b128 is serviced in groups of 16 lanes that read the same piece of 16
// rows, and the LDS has 16 slots of 16 bytes per bank row: 64-byte rows put rows r, r + 4, r + 8, r + 12 on the same four slots, so
// (r >> 2) & 3 spreads them; 128-byte rows put every second row on the same eight slots, so (r >> 1) & 7 does.  Either way the 16 rows
// of a group -- 16 consecutive rows, or the 8 + 8 of the halo patch -- fall on 16 distinct slots: conflict-free fragment reads.
// (row_common.h::ring_offset is the relative for the 640 ... 2560-byte rows of the row-resident weight ring.) ----
template <int ROWB> __device__ __forceinline__ constexpr int lds_row_swz(int r) {
    static_assert(ROWB == 64 || ROWB == 128, "BK = 32 or BK = 64 elements per row");
    return ROWB == 64 ? (r >> 2) & 3 : (r >> 1) & 7;
}

// ---- byte offset of a lane's fragment of 16-deep slice kk inside a swizzled tile: row `col` of a 32-row block, piece 2 kk + hi.  Block
// bases are multiples of 32 rows, so the swizzle term of row (base + col) is col's. ----
template <int ROWB> __device__ __forceinline__ int frag_offset(int col, int hi, int kk) { return col * ROWB + (((2 * kk + hi) ^ lds_row_swz<ROWB>(col)) << 4); }

// ---- K tiles per K slice: slice s of split_k owns tiles [s per, min(nk_total, s per + per)), possibly none.  Only this much is shared,
// and not by gemm_dma128_kernel: through it an s_add got its operands swapped there (as patch_common.h::k_slice records for its own form). ----
__host__ __device__ __forceinline__ int k_tiles_per_slice(int nk_total, int split_k) { return (nk_total + split_k - 1) / split_k; }

// ---- epilogue: one 32 x 32 accumulator fragment -> the fp32 tile in LDS (row stride CLD_ floats).  The MFMA is issued swapped (weight
// rows as the A operand), so the lane owns tile row `row` (its MFMA column; the halo-patch kernels map it through kColPix) and register
// quad j holds the 4 consecutive channels c0 + 8 j + 4 hi ----
template <int CLD_> __device__ __forceinline__ void acc_to_lds(float* Cs, int row, int c0, int hi, const f32x16& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        *reinterpret_cast<float4*>(Cs + row * CLD_ + c0 + 8 * j + 4 * hi) = make_float4(acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]);
}

// ---- one accumulator fragment to zero (the loops stay with the kernel: a helper over the whole array renumbered gemm_dma.hip's registers) ----
__device__ __forceinline__ void zero_frag(f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}

// ---- one 16-deep MFMA step of a wave tile of NA x NB blocks of 32 x 32: NA weight fragments (rows 32 a of Ws) and NB activation
// fragments (rows 32 b of Xs), STEP = bytes between two 32-row blocks, `off` = the lane's fragment offset inside a block, then NA x NB
// MFMAs.  W_FIRST: which operand is read first -- each kernel's own order.  (`off` apart: added to the bases at the caller, one
// instantiation of gemm_dma128_kernel took another register.) ----
template <bool F16, bool W_FIRST, int STEP, int NA, int NB>
__device__ __forceinline__ void mfma_step16(const char* Ws, const char* Xs, uint32_t off, f32x16 (&acc)[NA][NB]) {
    uint4 wf[NA], xf[NB];
    if (W_FIRST) {
#pragma unroll
        for (int a = 0; a < NA; ++a) wf[a] = *reinterpret_cast<const uint4*>(Ws + a * STEP + off);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) xf[b] = *reinterpret_cast<const uint4*>(Xs + b * STEP + off);
    if (!W_FIRST) {
#pragma unroll
        for (int a = 0; a < NA; ++a) wf[a] = *reinterpret_cast<const uint4*>(Ws + a * STEP + off);
    }
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = El<F16>::mfma(wf[a], xf[b], acc[a][b]);
}

// ---- epilogue: the 8 values of tile row `row`, channels cc .. cc + 7, back from the fp32 tile acc_to_lds wrote (two ds_read_b128).
// By value: with two float4& results the chunk loops of gemm_dma.hip compiled differently. ----
struct TileChunk8 { float4 v0, v1; };
template <int CLD_> __device__ __forceinline__ TileChunk8 lds_read8(const float* Cs, int row, int cc) {
    return TileChunk8{*reinterpret_cast<const float4*>(Cs + row * CLD_ + cc), *reinterpret_cast<const float4*>(Cs + row * CLD_ + cc + 4)};
}

// ---- host side: the launch itself.  Kernels with dynamic LDS get the attribute that lifts the 64 KB default (once per kernel and
// device: imd_lds_attr), then `grid` workgroups of `threads`, then the launch check in the launcher's name ----
typedef void (*tile_kern_t)(const ConvGemmParams);
static int tile_launch(tile_kern_t kern, const ConvGemmParams& p, dim3 grid, int threads, int lds, const char* what, hipStream_t s) {
    if (int rc_attr = lds > 0 ? imd_lds_attr(reinterpret_cast<const void*>(kern), lds, what) : 0) return rc_attr;
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, s, p);
    return imd_check_launch(what);
}

}  // namespace
