// Row-resident linear layer for the 32x32-level token matrix (K = 640, N a multiple of 160): the K = N = 640 projections of
// the level-1 transformer blocks (proj_in, attn1.to_out, attn2.to_q, attn2.to_out, proj_out -- 25 launches per denoising step,
// M = 8192 rows) and `norm2 -> attn2.to_q` as one launch.  Row-resident scheme (row_common.h); same reference arithmetic and
// same reasons as row_linear.hip (the tiled kernel walks K in ten dependent round trips to memory per workgroup and runs at
// ~0.11 of the MFMA peak on this shape).
//
// A full 640-wide row block does not fit a wave's registers next to the accumulators, and M = 8192 gives only 64 blocks of
// 128 rows, so the work is cut differently from the K = 320 kernel:
//   * grid = (M / 128 row blocks) x (N / 160 channel groups) -- 64 x 4 = 256 workgroups for the 640 -> 640 layers;
//   * inside a workgroup, wave (tb, kh) holds token block tb (32 rows) x K-HALF kh (320 k) in 80 VGPRs (B-operand layout,
//     loaded straight from global memory) and multiplies it with the matching half of every weight row: 20 MFMAs per
//     32-channel chunk, partial sums;
//   * the 160 weight rows of the group stream through LDS in 5 chunks of 32 rows x 640 k (40 KB, LDS-DMA, 3-slot ring, rows
//     unpadded with piece p of row r stored at p ^ (r & 15) -> conflict-free ds_read_b128);
//   * the two waves (tb, 0) and (tb, 1) own HALF of the 32 x 32 result each (register quads {0,1} / {2,3}): each hands the
//     quads it does not own to its partner through 2 KB of LDS (double buffered, published by the next chunk's barrier), adds
//     what it receives and stores its 2 x 4 channels per token straight from registers -- bias from LDS, residual fetched one
//     chunk ahead -- while the next chunk is being multiplied;
//   * LayerNorm prologue: each wave sees half a row; the two halves exchange (sum, sum of squared deviations) through LDS.
#include "row_common.h"

namespace {

constexpr int R6_K = 640, R6_KH = 320;
constexpr int R6_STEPS = R6_KH / 16;              // 20 k-steps per wave and chunk
constexpr int R6_ROWB = R6_K * 2;                 // 1280 bytes per weight row = 80 pieces
constexpr int R6_CHUNK = 32 * R6_ROWB;            // 40960
constexpr int R6_RING = ROW_RING;
constexpr int R6_NG = ROW_NG;                     // channels per workgroup
static_assert(R6_CHUNK == ROW_CHUNK, "ring_stage moves 40 KB chunks");
constexpr int R6_NC = R6_NG / 32;                 // 5 chunks
constexpr int R6_OFF_RED = R6_RING * R6_CHUNK;    // 122880: partial-sum exchange, 2 buffers x 8 waves x 2 KB
constexpr int R6_OFF_BIAS = R6_OFF_RED + 2 * 8 * 2048;     // 155648
constexpr int R6_OFF_LN = R6_OFF_BIAS + R6_NG * 4;         // 156288: LayerNorm partials, 8 waves x 64 lanes x 8 B
constexpr int R6_LDS = R6_OFF_LN + 8 * 64 * 8;             // 160384 <= 163840

// GN (round 6): GroupNorm (+ SiLU) of the rows from the statistic partials of x (gn_in_*; see row_linear.hip)
template <bool F16, bool LN, bool GN = false>
__global__ __launch_bounds__(512, 1) void row_linear_k640_kernel(const ConvGemmParams p, const float ln_eps) {
    static_assert(!(LN && GN), "one prologue at a time");
    using E = El<F16>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, col = lane & 31;
    const int tb = wave & 3, kh = wave >> 2;
    // hardware workgroup b runs on XCD b % 8: give every XCD whole row blocks (all channel groups of a row block share one L2,
    // so the activation rows cross the fabric once)
    const int n_groups = p.N / R6_NG;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int mblk = (slot / n_groups) * 8 + xcd, grp = slot % n_groups;
    if (mblk * 128 >= p.M) return;
    const int m0 = mblk * 128, n0 = grp * R6_NG;
    const int m = m0 + tb * 32 + col;

    GnInReq<R6_K> gnreq;
    if constexpr (GN) gn_in_request<R6_K>(p, m0 / (p.Hout * p.Wout), gnreq);      // (ahead of the activation loads: they come back first)
    // ---- activations: 32 rows x 320 k (this wave's K half) straight into B-operand fragments ----
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.x), 0, p.x_bytes, 0x00020000);
    const uint32_t xoff = (uint32_t)m * (uint32_t)(p.x_pix_stride * 2) + (uint32_t)(kh * (R6_KH * 2) + hi * 16);
    uint4 xf[R6_STEPS];
    load_rows(xf, rs_x, m < p.M, xoff, 32);
    float bias_v = 0.f;
    if (tid < R6_NG && p.bias) bias_v = p.bias[n0 + tid];

    // ---- weight stream ----
    const v4i_t ds_w = raw_rsrc(p.w, p.w_bytes);
    uint32_t woff[ROW_PIECES];
#pragma unroll
    for (int j = 0; j < ROW_PIECES; ++j) woff[j] = ring_offset<80, 0, 15>(j, wave, lane, n0);
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    auto stage = [&](int c) { ring_stage(ds_w, lds0, wave, woff, c); };
    stage(0);
    stage(1);
    pin_rows(xf);
    if (tid < R6_NG) reinterpret_cast<float*>(smem + R6_OFF_BIAS)[tid] = bias_v;

    if constexpr (LN) {      // LayerNorm without affine over all 640 channels: the K halves meet in LDS twice (sum, squared deviations)
        float2* lnx = reinterpret_cast<float2*>(smem + R6_OFF_LN);
        float sum = 0.f;      // (rows_sum / rows_sqdev written out: through the helpers hipcc commutes the additions of the partner's partials below)
#pragma unroll
        for (int s = 0; s < R6_STEPS; ++s) {
            float f[8];
            unpack8<F16>(xf[s], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) sum += f[e];
        }
        sum += __shfl_xor(sum, 32);
        lnx[wave * 64 + lane].x = sum;
        __syncthreads();
        const float mean = (sum + lnx[(wave ^ 4) * 64 + lane].x) * (1.0f / R6_K);
        float sq = 0.f;
        pin_rows(xf);
#pragma unroll
        for (int s = 0; s < R6_STEPS; ++s) {
            float f[8];
            unpack8<F16>(xf[s], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = f[e] - mean; sq = fmaf(d, d, sq); }
        }
        sq += __shfl_xor(sq, 32);
        lnx[wave * 64 + lane].y = sq;
        __syncthreads();
        const float rstd = rsqrtf((sq + lnx[(wave ^ 4) * 64 + lane].y) * (1.0f / R6_K) + ln_eps);
        const float shift = -mean * rstd;
        pin_rows(xf);
        rows_scale_shift<F16>(xf, rstd, shift);
    }

    if constexpr (GN) {      // (scratch = ring slot 2: nothing lands there before stage(2), issued behind the chunk loop's first barrier)
        const float *ga, *gs;
        gn_in_coeffs<R6_K>(p, m0 / (p.Hout * p.Wout), gnreq, reinterpret_cast<float*>(smem + 2 * R6_CHUNK), ga, gs);
        const bool silu = p.gn_in_silu != 0;
#pragma unroll
        for (int s = 0; s < R6_STEPS; ++s) {       // (one fragment at a time: see row_linear.hip)
            xf[s] = gn_in_apply8<F16>(xf[s], ga, gs, kh * R6_KH + 16 * s + 8 * hi, silu);
            asm volatile("" ::: "memory");        // (keeps the coefficient reads of the next fragment behind this one)
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- output side: this wave stores quads {2 kh, 2 kh + 1} of every chunk: channels n0 + 32 c + 8 q + 4 hi .. + 3 ----
    const int HWo = p.Hout * p.Wout;
    const bool heads = !GN && p.mode == OUT_HEADS;        // (GN: row-major output without residual only, see row_linear.hip)
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(heads ? (void*)p.hd[0].ptr : p.out, 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.res), 0, 0x80000000u, 0x00020000);
    uint32_t obase = OOB;
    if (m < p.M) {
        if (heads) { const int bi = m / HWo, tok = m - bi * HWo; obase = (uint32_t)(((size_t)bi * p.hH * p.hd[0].L + tok) * p.hd[0].DP * 2); }
        else obase = (uint32_t)m * (uint32_t)(p.out_ld * 2);
    }
    const bool has_res = !GN && p.res != nullptr;
    const uint32_t roff = (uint32_t)m * (uint32_t)(p.res_ld * 2);
    uint4 rraw[2];                     // residual of a chunk: (quad 2 kh | quad 2 kh + 1) in accumulator layout or, wide, 8 consecutive channels
    const bool wide = GN || (p.flags & 1024) != 0;      // 16-byte stores / residual loads of 8 consecutive channels (row_linear.hip: "WIDE stores"); knob 2 bit 10 = the 8-byte form
    auto load_res = [&](int c) {
        if (wide) rraw[c & 1] = buf_load16(rs_r, m < p.M ? roff + (uint32_t)((n0 + 32 * c + 16 * kh + 8 * hi) * 2) : OOB);
        else {
            const uint2 a = buf_load8(rs_r, m < p.M ? roff + (uint32_t)((n0 + 32 * c + 8 * (2 * kh) + 4 * hi) * 2) : OOB);
            const uint2 b = buf_load8(rs_r, m < p.M ? roff + (uint32_t)((n0 + 32 * c + 8 * (2 * kh + 1) + 4 * hi) * 2) : OOB);
            rraw[c & 1] = make_uint4(a.x, a.y, b.x, b.y);
        }
    };
    float4* red = reinterpret_cast<float4*>(smem + R6_OFF_RED);          // [2][8 waves][2 quads][64 lanes]
    const float* bias_s = reinterpret_cast<const float*>(smem + R6_OFF_BIAS);
    const float osc = heads ? p.out_scale * p.hd[0].scale : p.out_scale;
    float own[8];                      // this wave's two quads of the previous chunk (its own partial sums)
    auto emit = [&](int c) {           // chunk c: own partial + the partner's, bias, scale, residual, one 16-byte (or two 8-byte) stores
        v2u pk[2];
        uint2 rres[2];                 // residual in accumulator layout
        if (has_res) {
            uint4 r = rraw[c & 1];
            if (wide) r = wide_to_quads(r);
            rres[0] = make_uint2(r.x, r.y); rres[1] = make_uint2(r.z, r.w);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float4 o = red[((c & 1) * 8 + (wave ^ 4)) * 128 + j * 64 + lane];
            const int nl = 32 * c + 8 * (2 * kh + j) + 4 * hi;       // channel inside the group
            const float4 bb = *reinterpret_cast<const float4*>(bias_s + nl);
            float v0 = (own[4 * j] + o.x + bb.x) * osc, v1 = (own[4 * j + 1] + o.y + bb.y) * osc;
            float v2 = (own[4 * j + 2] + o.z + bb.z) * osc, v3 = (own[4 * j + 3] + o.w + bb.w) * osc;
            if (has_res) {
                v0 += E::lo(rres[j].x); v1 += E::hi(rres[j].x);
                v2 += E::lo(rres[j].y); v3 += E::hi(rres[j].y);
            }
            pk[j] = v2u{E::pack2(v0, v1), E::pack2(v2, v3)};
        }
        auto offset_of = [&](int n) -> uint32_t { return heads ? heads_channel_offset(p, n) : (uint32_t)(n * 2); };
        if (wide) {                    // quads 2 kh (channels 16 kh + 4 hi ..) and 2 kh + 1 (16 kh + 8 + 4 hi ..) -> channels 16 kh + 8 hi + 0..7 of the chunk
            const v4u w = quads_to_wide(pk[0], pk[1]);
            __builtin_amdgcn_raw_buffer_store_b128(w, rs_o, (int)(obase == OOB ? OOB : obase + offset_of(n0 + 32 * c + 16 * kh + 8 * hi)), 0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                __builtin_amdgcn_raw_buffer_store_b64(pk[j], rs_o, (int)(obase == OOB ? OOB : obase + offset_of(n0 + 32 * c + 8 * (2 * kh + j) + 4 * hi)), 0, 0);
        }
    };

    const uint32_t pb = (uint32_t)(kh * 40 + hi), sw = (uint32_t)(col & 15);
    const char* wlane = smem + col * R6_ROWB;
#pragma unroll
    for (int c = 0; c <= R6_NC; ++c) {
        dma_wait();                    // stores are in flight with the DMA pieces: no counted wait (see row_linear.hip)
        __syncthreads();               // chunk c landed for everybody; the partials of chunk c - 1 are published; slot of chunk c - 1 is free
        if (c > 0) emit(c - 1);
        if (c + 2 < R6_NC) stage(c + 2);
        if (c < R6_NC) {
            if (has_res) load_res(c);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const char* Ws = wlane + (c % R6_RING) * R6_CHUNK;
#pragma unroll
            for (int s = 0; s < R6_STEPS; ++s) {
                const uint4 wf = *reinterpret_cast<const uint4*>(Ws + (((pb + 2 * s) ^ sw) << 4));
                acc = E::mfma(wf, xf[s], acc);
            }
            // keep quads {2 kh, 2 kh + 1}, hand the other two to the partner wave (tb, 1 - kh)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float4 lo = make_float4(acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]);
                const float4 hi4 = make_float4(acc[8 + 4 * j], acc[9 + 4 * j], acc[10 + 4 * j], acc[11 + 4 * j]);
                const float4 mine = kh ? hi4 : lo, theirs = kh ? lo : hi4;
                own[4 * j] = mine.x; own[4 * j + 1] = mine.y; own[4 * j + 2] = mine.z; own[4 * j + 3] = mine.w;
                red[((c & 1) * 8 + wave) * 128 + j * 64 + lane] = theirs;
            }
        }
    }
}

template <bool F16, bool LN, bool GN = false>
int launch_r6(const ConvGemmParams& p, float eps, hipStream_t s) {
    return row_wide_launch_kernel<128>(row_linear_k640_kernel<F16, LN, GN>, R6_LDS, "row_linear_k640", p, eps, s);
}
constexpr RowLaunchFn R6_KERNELS[3][2] = {{launch_r6<true, false, true>, launch_r6<false, false, true>},
                                          {launch_r6<true, true>, launch_r6<false, true>},
                                          {launch_r6<true, false>, launch_r6<false, false>}};

}  // namespace

bool imd_row_linear_k640_supported(const ConvGemmParams& p) { return row_wide_supported<R6_K>(p); }

int imd_launch_row_linear_k640(const ConvGemmParams& p, int ln, float ln_eps, hipStream_t s) {
    // flags bit 10: wide (16-byte) stores of the direct epilogue
    return row_wide_launch<R6_K, 128>(p, ln, ln_eps, s, "row_linear_k640", (g_gemm_flags & 1024) ? 0 : 1024, R6_KERNELS);
}
