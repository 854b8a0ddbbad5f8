// Flash attention for head dim 512 on gfx950: the single-head attention of the SD1.5 VAE mid block (N = L = latent tokens, d = 512) in ONE
// launch for the whole batch, without an N x N tensor.
//
//   O[b, q, h*512:(h+1)*512] = softmax(Q K^T) V
//
// Operand layouts and conventions are those of attention.hip (so the host side is the same call):
//   Q   [B , H, N, 512]    already multiplied by  512^-1/2 * log2(e)   (softmax runs on exp2)
//   K   [Bk, H, L, 512]    rows = keys
//   V^T [Bk, H, 512, LP]   rows = head dim, keys contiguous, LP = L rounded up to 64 (zero padded)
// and the kv batch entry of batch b is b / kv1_bdiv.  One key set only; no causal mask, fused out-projection, out_dup or phase split.
//
// Why not attention.hip's template at D = 512: its 64-key K / V^T tiles would be 2 x 139 KB of LDS.  Here a tile is 32 keys, staged by LDS-DMA
// (lds_dma.h: global memory -> LDS without a VGPR round trip; the register file has none to spare):
//   K tile   32 rows x 1024 B = 32 KB, a ring of three        V^T tile   512 rows x 64 B = 32 KB, two stages        = 160 KB, all of a CU's LDS
// LDS-DMA pieces are lane-linear, so rows cannot be padded; the 16-byte chunk a lane fetches is chosen so that the b128 fragment reads are
// conflict-free (the maps are next to the staging code).
//
// Structure: one workgroup = 4 waves = 128 query rows of one (batch, head); wave w owns rows 32 w .. 32 w + 31 for the WHOLE head dim:
//   Q fragments      32 x uint4 = 128 VGPRs (read once)
//   O^T accumulator  16 blocks of 32x32 fp32 = 256 registers (the AGPR half of the 512-entry file at one wave per SIMD)
// Per tile a wave runs 32 + 32 v_mfma_f32_32x32x16 (S^T = K Q^T, then O^T += V^T P^T) on 64 KB of LDS fragments.  32 query rows per wave is the
// most the register file holds; with fewer (16 rows, v_mfma_f32_16x16x32) every wave would still read the whole 64 KB per tile, i.e. twice the
// LDS bytes and twice the staged bytes per FLOP.  The price of the 128-row workgroup is a small grid: N / 128 workgroups per (batch, head), one
// per CU (160 KB of LDS), so a 64x64 latent at batch 1 occupies 32 of the 256 CUs.
// As in attention.hip the MFMA rows of S^T are permuted (swap23), so that after exp2 and packing a lane's registers ARE the B operand of the
// P.V MFMA: no LDS round trip for P.  The running maximum is exact (raised whenever a tile's maximum exceeds it), the denominator a per-lane
// fp32 sum; the two half-waves that share a query row exchange one value per tile (max) and one at the end (sum).
// One barrier per tile.  Measured on MI355X (fp16, kernel alone, per tile of one workgroup): MFMAs and softmax without staging 2.05 us, staging
// without compute 1.05 us, this kernel 3.8 us at 4096 keys and 3.05 us at 16384 -- the two do not overlap yet at one wave per SIMD; 705 TFLOP/s
// at B = 4, N = 16384.
#include "attn_common.h"

namespace {

constexpr int HD = 512;                    // head dim
constexpr int KT = 32;                     // keys per tile
constexpr int NKT = HD / 16;               // QK^T MFMA steps per tile
constexpr int NDT = HD / 32;               // 32-row blocks of O^T
constexpr int KROW = HD * 2;               // bytes per K LDS row (unpadded: LDS-DMA pieces are lane-linear)
constexpr int VROW = KT * 2;               // bytes per V^T LDS row
constexpr int VBYTES = HD * VROW;          // 32 KB
constexpr int KBYTES = KT * KROW;          // 32 KB
constexpr int KOFF = 2 * VBYTES;           // LDS: V^T stages 0 / 1, then a ring of three K tiles
constexpr int LDS_BYTES = KOFF + 3 * KBYTES;   // 160 KB: all of a CU's LDS
constexpr int PIECES = KBYTES / 1024 / 4;  // 1 KB LDS-DMA pieces per wave and operand tile (8)
static_assert(KBYTES == 4 * PIECES * 1024 && VBYTES == 4 * PIECES * 1024, "a tile is a whole number of pieces per wave");

// x * alpha for an accumulator element that LIVES in an AGPR: read, multiply, write back in one statement.  Written out because hipcc, handed
// `o[dt][r] *= alpha` over the 256-register accumulator, moves the whole accumulator to VGPRs at the top of the tile loop and spills the Q
// fragments to scratch (1 KB per lane); with the "a" constraint the accumulator stays where the MFMAs want it.  The only producers of these
// registers are VALU writes and the P.V MFMAs of the PREVIOUS tile, which have retired behind that tile's barrier and this tile's 32 QK^T MFMAs
// (MFMAs of a wave issue in order), so no wait states are owed in front of the read.
__device__ __forceinline__ float acc_scale(float x, float alpha) {
    float tmp;
    asm volatile("v_accvgpr_read_b32 %1, %0\n\tv_mul_f32 %1, %1, %2\n\tv_accvgpr_write_b32 %0, %1" : "+a"(x), "=&v"(tmp) : "v"(alpha));
    return x;
}

template <bool F16>
__global__ __launch_bounds__(256, 1) void attn_d512_kernel(const AttnParams p) {
    using E = El<F16>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int col = lane & 31;
    int wx, h, b;
    {
        const unsigned w = attn_work_index<WORK_XCD>(p);          // XCD-aware work list, no plain-order knob (split inline: through attn_work_split 128 lines differ)
        const unsigned gx = gridDim.x, gz = gridDim.z;
        wx = (int)(w % gx);
        b = (int)((w / gx) % gz);
        h = (int)(w / (gx * gz));
    }
    const int q0 = (wx * 4 + wave) * 32;
    const int q = q0 + col;

    // ---- Q fragments (B operand of S^T = K Q^T): lane = query column, 8 head-dim values per fragment; rows past N are zero ----
    uint4 qf[NKT];
    {
        const bf16_t* qbase = p.q + (size_t)(b * p.H + h) * p.N * HD;
        const __amdgpu_buffer_rsrc_t rs_q = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(qbase), 0, (uint32_t)p.N * HD * 2, 0x00020000);
#pragma unroll
        for (int t = 0; t < NKT; ++t) qf[t] = buf_load16(rs_q, (uint32_t)q * (HD * 2) + t * 32 + hi * 16);      // (q >= N: past the end, zero)
    }

    f32x16 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int L = p.L1, LP = p.L1P;
    const int kvb = b / p.kv1_bdiv;
    const bf16_t* kbase = p.k1 + (size_t)(kvb * p.H + h) * L * HD;
    const bf16_t* vbase = p.v1t + (size_t)(kvb * p.H + h) * HD * LP;
    const int ntiles = (L + KT - 1) / KT;
    // buffer descriptors over this (batch, head)'s K rows / V^T rows: offsets past the end read as zero (the launcher bounds both below 2 GiB)
    const v4i_t ds_k = raw_rsrc(kbase, (uint32_t)L * HD * 2), ds_v = raw_rsrc(vbase, (uint32_t)LP * HD * 2);
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    // One tile = 32 K pieces (piece = key row r of the tile, 64 chunks of 16 B) + 32 V^T pieces (piece = 16 head-dim rows of 4 chunks); wave w
    // issues pieces 8 w .. 8 w + 7 of each.  LDS rows are unpadded; bank conflicts are avoided by WHICH chunk a lane fetches:
    //   K:   chunk c of row r is stored at position c ^ (r & 15)        V^T: chunk c of row d at position c ^ ((d >> 2) & 3)
    // -- every lane group of a ds_read_b128 covers all 16 residues of its row index, hence 16 distinct 16-byte bank slots.
    // (the source offsets are derived from the thread index at every piece, behind an empty asm: as loop invariants they would cost 16 VGPRs)
    auto k_piece = [&](int t, int slot, int i) {          // piece i of this wave of K tile t -> ring slot `slot`
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        l &= 63;
        const int r = wave * PIECES + i;
        dma16(ds_k, lds0 + (uint32_t)(KOFF + slot * KBYTES + r * 1024), (uint32_t)(t * KT + r) * (uint32_t)KROW + (uint32_t)((l ^ (r & 15)) << 4));
    };
    auto v_piece = [&](int t, int i) {                    // piece i of this wave of V^T tile t -> stage t & 1
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        l &= 63;
        const int pc = wave * PIECES + i;
        const int d = pc * 16 + (l >> 2), c = (l & 3) ^ ((l >> 4) & 3);          // ((d >> 2) & 3 == (l >> 4) & 3: pc * 16 is a multiple of 16)
        dma16(ds_v, lds0 + (uint32_t)((t & 1) * VBYTES + pc * 1024), ((uint32_t)d * (uint32_t)LP + (uint32_t)(t * KT + c * 8)) * 2u);
    };

#pragma unroll
    for (int i = 0; i < PIECES; ++i) { k_piece(0, 0, i); v_piece(0, i); }
    if (ntiles > 1) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i) k_piece(1, 1, i);
    }
    dma_wait();
    __syncthreads();

    const int krow = swap23(col);                                  // permuted key row of this lane
    const int kfrag = krow * KROW, kswz = (hi ^ (krow & 15)) << 4;      // chunk 2 tk + hi sits at (2 tk + hi) ^ (krow & 15): low four bits only
    const int vfrag = col * VROW, vswz = (col >> 2) & 3;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int kslot = 0;                                                 // t % 3
    for (int t = 0; t < ntiles; ++t) {
        const char* Vs = smem + (t & 1) * VBYTES;
        const char* Ks = smem + KOFF + kslot * KBYTES;
        const bool more = t + 1 < ntiles, more2 = t + 2 < ntiles;
        const int nslot = kslot == 0 ? 2 : kslot - 1;              // (t + 2) % 3: the slot tile t - 1 was read from
        // Both MFMA phases run in 8 groups of 4 MFMAs.  A group's four fragments are read from LDS one group ahead, and every group carries ONE
        // LDS-DMA piece: 16 pieces issued back to back fill the memory pipeline's queue and hold the wave's only instruction stream for about a
        // microsecond (measured: staging alone 1.05 us per tile, compute alone 2.05 us, both with all pieces at the top of the tile 4.05 us).
        //   QK^T groups:  V^T tile t + 1  -> the stage last read by the P.V of tile t - 1
        //   P.V  groups:  K tile t + 2    -> the ring slot last read by the QK^T of tile t - 1; it has a whole tile to land
        uint4 fr[2][4];
        auto kread = [&](int g, uint4* dst) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int tk = 4 * g + j;
                dst[j] = *reinterpret_cast<const uint4*>(Ks + kfrag + (tk >> 3) * 256 + (((tk & 7) * 32) ^ kswz));
            }
        };
        auto vread = [&](int g, uint4* dst) {             // fragments of O^T blocks 2 g, 2 g + 1: [block][key octet]
#pragma unroll
            for (int j = 0; j < 4; ++j)
                dst[j] = *reinterpret_cast<const uint4*>(Vs + (2 * g + (j >> 1)) * 32 * VROW + vfrag + (((2 * (j & 1) + hi) ^ vswz) << 4));
        };

        // ---- S^T = K Q^T ----
        f32x16 s;
        kread(0, fr[0]);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            if (g < 7) kread(g + 1, fr[(g + 1) & 1]);
            if (more) v_piece(t + 1, g);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = E::mfma(fr[g & 1][j], qf[4 * g + j], (g == 0 && j == 0) ? zero16 : s);
            __builtin_amdgcn_sched_barrier(0);
        }
        vread(0, fr[0]);                      // the first P.V group's fragments travel under the softmax

        // ---- online softmax (base 2; Q carries the scale): reg r of half hi is key 32 t + 8 hi + (r & 7) + 16 (r >> 3) ----
        if ((t + 1) * KT > L) {               // pad keys of the last tile get weight exactly 0
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (t * KT + 8 * hi + (r & 7) + 16 * (r >> 3) >= L) s[r] = -INFINITY;
        }
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        if (__any(m_new != m_run)) {          // rescale only when some row's running maximum moved (alpha == 1 otherwise)
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] = acc_scale(o[dt][r], alpha);
            m_run = m_new;
        }
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(s[r] - m_new);
            psum += s[r];
        }
        l_run += psum;
        uint4 pf[2];                          // P^T fragments: octet g = keys 16 g + 8 hi .. + 7 of the tile, rounded to the element type
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            pf[g].x = E::pack2(s[8 * g + 0], s[8 * g + 1]);
            pf[g].y = E::pack2(s[8 * g + 2], s[8 * g + 3]);
            pf[g].z = E::pack2(s[8 * g + 4], s[8 * g + 5]);
            pf[g].w = E::pack2(s[8 * g + 6], s[8 * g + 7]);
        }

        // ---- O^T += V^T P^T ----
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            if (g < 7) vread(g + 1, fr[(g + 1) & 1]);
            if (more2) k_piece(t + 2, nslot, g);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[2 * g + (j >> 1)] = E::mfma(fr[g & 1][j], pf[j & 1], o[2 * g + (j >> 1)]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // V^T tile t + 1 (issued in this tile's first half) and K tile t + 1 (issued a tile ago) must have landed; K tile t + 2, this wave's
        // youngest eight pieces, stays in flight
        if (more2) dma_wait_keep_n<PIECES>(); else dma_wait();
        __syncthreads();                      // ... everybody's pieces; all waves are done reading tile t
        kslot = kslot == 2 ? 0 : kslot + 1;
    }

    // ---- normalise: o * (1 / l), one rounding; rows past N are not stored ----
    // The lane's output position is derived AGAIN from the thread index, behind an empty asm the compiler cannot look through: kept live across
    // the tile loop, these values (row, half, 64-bit row pointer) were the ones that went to scratch at 256 VGPRs.
    const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32));
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const int hi_e = (tid_e >> 5) & 1;
    const int q_e = (wx * 4 + (tid_e >> 6)) * 32 + (tid_e & 31);
    if (q_e >= p.N) return;
    bf16_t* orow = p.out + ((size_t)b * p.N + q_e) * p.out_ld + h * HD;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dd = dt * 32 + 8 * j + 4 * hi_e;        // accumulator row of regs 4 j .. 4 j + 3 (mfma_row)
            *reinterpret_cast<uint2*>(orow + dd) = make_uint2(E::pack2(o[dt][4 * j + 0] * inv, o[dt][4 * j + 1] * inv),
                                                              E::pack2(o[dt][4 * j + 2] * inv, o[dt][4 * j + 3] * inv));
        }
}

template <bool F16>
int launch_d512(const AttnParams& p, hipStream_t s) {
    constexpr int lds = LDS_BYTES;
    auto kern = attn_d512_kernel<F16>;
    if (int rc_attr = imd_lds_attr(reinterpret_cast<const void*>(kern), lds, "attention (head dim 512)")) return rc_attr;
    dim3 grid((p.N + 127) / 128, p.H, p.B);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, p);
    return imd_check_launch("attention (head dim 512)");
}

}  // namespace

// imd_launch_attention has validated B / H / N / L1 / L1P / kv1_bdiv / dtype (and B, H <= 65535) before it dispatches here.
int imd_launch_attention_d512(const AttnParams& p, hipStream_t s) {
    if (p.k2 != nullptr || p.v2t != nullptr || p.scale2 != nullptr)
        return imd_set_error("attention: head dim 512 takes one key set: k2 / v2t / scale2 must be NULL");
    if (p.causal) return imd_set_error("attention: head dim 512 has no causal mask (causal must be 0)");
    if (p.proj_w != nullptr) return imd_set_error("attention: head dim 512 has no fused out-projection (proj_w must be NULL)");
    if (p.out_dup != nullptr) return imd_set_error("attention: head dim 512 has no duplicated output (out_dup must be NULL)");
    if (p.phase2_out != nullptr || p.phase2_rows != 0) return imd_set_error("attention: head dim 512 has no phase-split launch (phase2_out must be NULL, phase2_rows 0)");
    if (p.k_pad_one) return imd_set_error("attention: head dim 512 has no K pad column (k_pad_one must be 0)");
    if ((size_t)p.N * HD * 2 >= 0x80000000ull) return imd_set_error("attention: head dim 512: Q of one (batch, head) beyond 2 GiB (N = %d)", p.N);
    if ((size_t)p.L1P * HD * 2 >= 0x80000000ull) return imd_set_error("attention: head dim 512: K / V^T of one (batch, head) beyond 2 GiB (L1P = %d)", p.L1P);
    if ((reinterpret_cast<uintptr_t>(p.q) | reinterpret_cast<uintptr_t>(p.k1) | reinterpret_cast<uintptr_t>(p.v1t)) & 15)
        return imd_set_error("attention: head dim 512 needs 16-byte aligned q / k1 / v1t");
    if (reinterpret_cast<uintptr_t>(p.out) & 7) return imd_set_error("attention: head dim 512 needs an 8-byte aligned out");
    return p.dtype == IMD_DTYPE_F16 ? launch_d512<true>(p, s) : launch_d512<false>(p, s);
}
