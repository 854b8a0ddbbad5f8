// Augmented activation rows of a LoRA layer whose scale differs from row to row (imd_lora_expand_rows):
//
//   out[m, 0 .. C)     = x[m, :]                                                      the same bits
//   out[m, C + j]      = 16-bit( row_scale[m / rows_per_entry] * sum_c x[m, c] down[j, c] )        j < T
//
// so that the projection which follows is the EXISTING launch on [x | s (x D^T)] . [W | U]^T with Cin = C + T: the per-row scale lives in
// the activations, the augmented weight does not depend on it.  Sum in fp32 on the MFMA, scale in fp32 on the finished sum, one
// rounding (RNE) to the element type.
//
// A member of the row-resident family (row_common.h): a wave keeps its token rows in registers as MFMA B-operand fragments for the whole
// kernel, the `down` matrix streams past them through LDS.  How it is cut, and why:
//   * ROWS.  A workgroup is 4 waves and owns 64 token rows; a wave owns 16 of them and uses the 16x16x32 MFMA: lane l holds row l & 15,
//     channels 32 s + 8 (l >> 4) .. + 7 of k-step s -- one 16-byte load per step, C / 32 steps, at most 40 fragments = 160 VGPRs at
//     C = 1280.  (The 32x32x16 form of the other members would need 320 VGPRs for a whole row of 1280 channels; they split K over waves
//     and meet in LDS, which a kernel whose output is only T <= 384 wide has no use for.)  x is therefore read from memory ONCE: the
//     fragment a lane multiplies is also the 16 bytes it stores to out[m, 32 s + 8 (l >> 4)], the pass-through copy.
//   * C is not cut: every lane group (l >> 4) holds its quarter of every k-step, and the MFMA sums over them.  A ragged C (80, 208 ..,
//     any multiple of 16) runs the same body: fragments at or past C are zero on both operands and store nothing.  S, the number of
//     k-steps that are compiled in (3 | 5 | 10 | 20 | 24 | 40 for C <= 96 | 160 | 320 | 640 | 768 | 1280), only sizes the register
//     array; steps past C are skipped by a wave-uniform branch.  There is no separate fallback instantiation.
//   * T is cut in chunks of 32 `down` rows.  A chunk (32 x C, at most 80 KB) is staged into LDS by all 256 threads with plain 16-byte
//     loads (8 lanes per row: whole 128-byte lines) -- not by the family's LDS-DMA ring, whose 40 KB chunks and compile-time row
//     lengths fit K = 320 / 640 / 1280 only.  One buffer, two barriers per chunk: with <= 256 VGPRs and <= 80 KB two workgroups share
//     a CU, and one stages while the other multiplies.  Where the rows alone cannot fill the chip (M <= 12288: the 16x16 and 8x8 levels) the
//     chunks of a row block are dealt over several workgroups (gridDim.y, see the launcher); only then are rows read more than once.
//     Two 16x16 tiles per chunk, their A rows permuted -- MFMA row 4 g + r of tile a is down row 8 g + r of the chunk, of tile b row
//     8 g + 4 + r -- so that lane (g = l >> 4, token l & 15) ends up with the 8 CONSECUTIVE tail channels 8 g .. 8 g + 7 of its token in
//     its 2 x 4 accumulators: the tail leaves as 16-byte stores like the pass-through (16-byte store fragments, not bandwidth, were the
//     "write wall" of README round 5).  A chunk with 16 valid rows (T = 16, 48, ..) stores from lane groups 0 and 1 only.
//   * LDS rows are unpadded (2 x 80 KB is all of the CU's LDS at C = 1280); the 16-byte pieces of row r are rotated by
//     (r & 3) | ((r >> 3) << 2) -- the MFMA row that reads them -- which spreads the 16 rows a lane group reads together over 16 bank
//     groups where the row length is a multiple of 256 bytes; other lengths are spread by the length itself.
// No scratch, no atomics; every store is a 16-byte vector store of this lane's own row.
#include "row_common.h"

namespace {

constexpr int LR_ROWS = 64;          // token rows per workgroup (16 per wave)
constexpr int LR_TN = 32;            // down rows per chunk
constexpr int LR_THREADS = 256;

template <bool F16, int S>
__global__ __launch_bounds__(LR_THREADS, 2) void lora_expand_rows_kernel(const LoraRowsParams p) {
    using E = El<F16>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, col = lane & 15;
    const int C = p.C, T = p.T;
    const int PPR = C >> 3;                                   // 16-byte pieces per row (>= 8)
    const int rowb = C * 2;                                   // bytes per down / LDS row
    const int m = blockIdx.x * LR_ROWS + wave * 16 + col;
    const bool mv = m < p.M;

    const uint32_t x_bytes = (uint32_t)(((size_t)(p.M - 1) * p.x_ld + C) * 2);
    const uint32_t o_bytes = (uint32_t)(((size_t)(p.M - 1) * p.out_ld + C + T) * 2);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.x), 0, x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.down), 0, (uint32_t)(T * rowb), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, o_bytes, 0x00020000);

    // ---- this lane's quarter of its row, all k-steps: B-operand fragments and pass-through payload in one ----
    const uint32_t xoff = (uint32_t)m * (uint32_t)(p.x_ld * 2) + (uint32_t)(g * 16);
    uint4 xf[S];
#pragma unroll
    for (int s = 0; s < S; ++s) xf[s] = buf_load16(rs_x, (mv && 32 * s + 8 * g < C) ? xoff + 64 * s : OOB);
    const float sc = mv ? p.row_scale[m / p.rows_per_entry] : 0.f;
    const uint32_t ooff = (uint32_t)m * (uint32_t)(p.out_ld * 2);

    // ---- staging of a chunk: thread = (row tid >> 3, pieces (tid & 7) + 8 i); rows at or past T read as zero ----
    const int srow = tid >> 3, sp0 = tid & 7;
    const int srot = (srow & 3) | ((srow >> 3) << 2);
    char* const drow = smem + srow * rowb;
    auto stage = [&](int j0) {
        const bool rv = j0 + srow < T;
        const uint32_t src = (uint32_t)(j0 + srow) * (uint32_t)rowb;
#pragma unroll 1
        for (int pb = sp0; pb < PPR; pb += 32) {
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pos = pb + 8 * u;
                v[u] = buf_load16(rs_d, (rv && pos < PPR) ? src + (uint32_t)(pos * 16) : OOB);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pos = pb + 8 * u;
                if (pos < PPR) {
                    int rp = pos + srot;                      // < PPR + 16 <= 3 PPR
                    if (rp >= PPR) rp -= PPR;
                    if (rp >= PPR) rp -= PPR;
                    *reinterpret_cast<uint4*>(drow + rp * 16) = v[u];
                }
            }
        }
    };

    // ---- A-operand rows of this lane: MFMA row `col` of tile a = chunk row 8 (col >> 2) + (col & 3), of tile b four rows further; both rotated by `col` ----
    const char* const la = smem + (8 * (col >> 2) + (col & 3)) * rowb;
    const char* const lb = la + 4 * rowb;
    int rp0 = g + col;                                        // piece g of step 0, rotated
    if (rp0 >= PPR) rp0 -= PPR;
    if (rp0 >= PPR) rp0 -= PPR;

    // chunks blockIdx.y, blockIdx.y + gridDim.y, ...: gridDim.y > 1 only where the rows alone cannot fill the chip (see the launcher)
    const int nch = (T + LR_TN - 1) / LR_TN;
    const int c_first = (int)blockIdx.y, c_step = (int)gridDim.y;
#pragma unroll 1
    for (int c = c_first; c < nch; c += c_step) {
        const int j0 = c * LR_TN;
        if (c > c_first) __syncthreads();                     // every wave is done reading the previous chunk
        stage(j0);
        __syncthreads();
        if (c == 0) {                                         // the pass-through copy (workgroups of chunk 0 only) leaves under the first chunk's MFMAs
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const v4u w = {xf[s].x, xf[s].y, xf[s].z, xf[s].w};
                __builtin_amdgcn_raw_buffer_store_b128(w, rs_o, (int)((mv && 32 * s + 8 * g < C) ? ooff + (uint32_t)(64 * s + 16 * g) : OOB), 0, 0);
            }
        }
        f32x4 aa = {0.f, 0.f, 0.f, 0.f}, ab = {0.f, 0.f, 0.f, 0.f};
        int rp = rp0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (32 * s < C) {                                 // wave-uniform
                uint4 wa = *reinterpret_cast<const uint4*>(la + rp * 16);
                uint4 wb = *reinterpret_cast<const uint4*>(lb + rp * 16);
                if (32 * s + 32 > C && 32 * s + 8 * g >= C) {   // ragged last step: this lane's k slots lie past C (the read above hit a wrapped piece)
                    wa = make_uint4(0, 0, 0, 0);
                    wb = make_uint4(0, 0, 0, 0);
                }
                aa = E::mfma16(wa, xf[s], aa);
                ab = E::mfma16(wb, xf[s], ab);
                rp += 4;
                if (rp >= PPR) rp -= PPR;
            }
        }
        // lane (g, token): aa[r] = tail channel j0 + 8 g + r, ab[r] = j0 + 8 g + 4 + r
        float v[8] = {aa[0] * sc, aa[1] * sc, aa[2] * sc, aa[3] * sc, ab[0] * sc, ab[1] * sc, ab[2] * sc, ab[3] * sc};
        const uint4 o = pack8<F16>(v);
        const v4u w = {o.x, o.y, o.z, o.w};
        const int j = j0 + 8 * g;
        __builtin_amdgcn_raw_buffer_store_b128(w, rs_o, (int)((mv && j < T) ? ooff + (uint32_t)((C + j) * 2) : OOB), 0, 0);
    }
}

template <bool F16, int S>
int launch_lr(const LoraRowsParams& p, hipStream_t s) {
    auto kern = lora_expand_rows_kernel<F16, S>;
    const int lds = LR_TN * p.C * 2;
    if (int rc_attr = imd_lds_attr(reinterpret_cast<const void*>(kern), LR_TN * 32 * S * 2, "lora_expand_rows")) return rc_attr;
    // Few rows (the 16x16 / 8x8 levels: 40 row blocks at 2560 rows): the T chunks are dealt over gridDim.y workgroups per row block as well, as many as
    // it takes to put about 1.5 workgroups on each of the 256 CUs, in equal shares.  Those workgroups re-read their rows (from the L2: the whole
    // x is a few MB there); every output element is still computed by exactly one of them, the same way, so the split does not change a bit.
    const int row_blocks = (p.M + LR_ROWS - 1) / LR_ROWS, nch = (p.T + LR_TN - 1) / LR_TN;
    int ys = 384 / row_blocks;
    ys = ys < 1 ? 1 : ys > nch ? nch : ys;
    const int per = (nch + ys - 1) / ys;
    ys = (nch + per - 1) / per;
    hipLaunchKernelGGL(kern, dim3((unsigned)row_blocks, (unsigned)ys), dim3(LR_THREADS), lds, s, p);
    return imd_check_launch("lora_expand_rows");
}

template <bool F16>
int launch_lr_c(const LoraRowsParams& p, hipStream_t s) {
    if (p.C <= 96) return launch_lr<F16, 3>(p, s);
    if (p.C <= 160) return launch_lr<F16, 5>(p, s);
    if (p.C <= 320) return launch_lr<F16, 10>(p, s);
    if (p.C <= 640) return launch_lr<F16, 20>(p, s);
    if (p.C <= 768) return launch_lr<F16, 24>(p, s);
    return launch_lr<F16, 40>(p, s);
}

}  // namespace

int imd_launch_lora_expand_rows(const LoraRowsParams& p, hipStream_t s) {
    const char* n = "lora_expand_rows";
    if (p.dtype != IMD_DTYPE_BF16 && p.dtype != IMD_DTYPE_F16) return imd_set_error("%s: unknown dtype %d", n, p.dtype);
    if (p.C % 16 || p.T % 16) return imd_set_error("%s: C (%d) and T (%d) must be multiples of 16", n, p.C, p.T);
    if (p.C < 64 || p.C > 1280) return imd_set_error("%s: C (%d) outside 64..1280", n, p.C);
    if (p.T < 16 || p.T > 384) return imd_set_error("%s: T (%d) outside 16..384", n, p.T);
    if (p.M < 1 || p.E < 1 || p.rows_per_entry < 1 || (long long)p.E * p.rows_per_entry != p.M)
        return imd_set_error("%s: M (%d) is not E (%d) x rows_per_entry (%d)", n, p.M, p.E, p.rows_per_entry);
    if (p.x_ld < p.C) return imd_set_error("%s: x_ld (%d) < C (%d)", n, p.x_ld, p.C);
    if (p.out_ld < p.C + p.T) return imd_set_error("%s: out_ld (%d) < C + T (%d)", n, p.out_ld, p.C + p.T);
    if (p.x_ld % 8 || p.out_ld % 8) return imd_set_error("%s: leading dimensions (x_ld %d, out_ld %d) must be multiples of 8 elements", n, p.x_ld, p.out_ld);
    if (((uintptr_t)p.x | (uintptr_t)p.down | (uintptr_t)p.out) & 15) return imd_set_error("%s: x, down and out must be 16-byte aligned", n);
    if ((uintptr_t)p.row_scale & 3) return imd_set_error("%s: row_scale must be 4-byte aligned", n);
    const size_t xb = ((size_t)(p.M - 1) * p.x_ld + p.C) * 2, ob = ((size_t)(p.M - 1) * p.out_ld + p.C + p.T) * 2;
    if (xb >= 0x80000000ull || ob >= 0x80000000ull) return imd_set_error("%s: operand too large (2 GiB or more)", n);
    const uintptr_t x0 = (uintptr_t)p.x, o0 = (uintptr_t)p.out;
    if (x0 < o0 + ob && o0 < x0 + xb) return imd_set_error("%s: out overlaps x", n);
    return p.dtype == IMD_DTYPE_F16 ? launch_lr_c<true>(p, s) : launch_lr_c<false>(p, s);
}
