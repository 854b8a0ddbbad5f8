// Nearest-2x upsample + 3x3 conv as four 2x2 PHASE convolutions (Upsample2D: interpolate -> conv) (gfx950, bf16 / fp16 MFMA).
//
// After a nearest-2x upsample the four pixels of a 2 x 2 output block see the same 2 x 2 source pixels, so for output phase (py, px)
//   out[2y + py, 2x + px] = bias + sum_{dy, dx in {0, 1}} W'[py, px][dy, dx] . src[y + py - 1 + dy, x + px - 1 + dx]
// with W' the 3x3 taps that fall on one source pixel pre-summed (rows: py = 0: {ky 0}, {ky 1, 2}; py = 1: {ky 0, 1}, {ky 2}; the same in x;
// ops.pack_upsample_phase, once per layer): four taps instead of nine.  A workgroup owns an 8 x 16 tile of SOURCE pixels of one image x 128
// output channels x one phase and stages the (8+2) x (16+2) source patch of a 32-channel chunk as the 9-tap kernel (conv_patch.hip) does -- directly, no
// source pixel more than once.  The problem is laid out as N' = 4 N weight rows [phase][channel][tap][Cin]; the phase is the FAST part of the
// channel-tile index, so the four phases of a pixel tile run next to each other and share the patch in the XCD's L2.
// Schedule: the three-slot weight ring of the 9-tap kernel with the flattened tap index it = 4 chunk + tap (tap it + 2 in flight while tap it
// is multiplied); ring slot it % 3 and patch buffer chunk % 2 repeat every 6 chunks = 24 taps, which are unrolled with every LDS address a
// compile-time offset.  The next chunk's patch is fetched at tap 1 BEHIND that tap's weight pieces; in-order retirement then gives the waits:
//   end of tap 1: in flight W[it+1], W[it+2], P      -> keep WPW + APW
//   end of tap 2: in flight W[it+1], P, W[it+2]      -> keep WPW + APW   (W[k] = weight pieces of flattened tap k, `it` = this tap)
//   end of tap 3: in flight P, W[it+1], W[it+2]      -> keep WPW: the patch has landed before the next chunk's tap 0
//   end of tap 0: in flight W[it+1], W[it+2]         -> keep WPW
// Epilogue: bias only (the consumers -- the skip concatenation, the VAE's GroupNorm -- take their own statistics); source pixel (y, x) is
// stored to output row (b 2H + 2y + py) 2W + 2x + px.
//
// Tile constants, the MFMA-column -> pixel table, the tile decode, the LDS-DMA geometry PD<32>, the staging piece and the launch body are
// the halo-patch family's: patch_common.h.
#include "patch_common.h"

namespace {

template <bool F16>
__global__ __launch_bounds__(256, 3) void conv_ups_phase_kernel(const ConvGemmParams p) {
    using G = PD<32>;
    using E = El<F16>;
    constexpr int CKD = 32, NT = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm0 = (wave >> 1) * 64;          // 2 x 2 waves, each 64 pixels x 64 channels
    const int wn0 = (wave & 1) * 64;
    const int hi = lane >> 5, col = lane & 31;
    const int cpix = kColPix[col];

    const int H = p.Hin, W = p.Win;            // the SOURCE map: tiles, patch and halo live there
    const HaloTile tl = halo_tile<TH, TW, BN, 4>(p, H, W);         // (channel tile, phase), phase fastest
    const int phase = tl.tile_n & 3, py = phase >> 1, px = phase & 1;
    const int b = tl.b, y0 = tl.ty * TH, x0 = tl.tx * TW, n0 = (tl.tile_n >> 2) * BN;
    const int nch = p.Cin / CKD;               // >= 1 (launcher)

    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t smem_base = (uint32_t)(uintptr_t)smem;
    const v4i_t dx = raw_rsrc(p.x, p.x_bytes), dw = raw_rsrc(p.w, p.w_bytes);
    constexpr uint32_t FAR = 0x80000000u;      // out-of-range under every running add (operands < 2 GiB: launcher)
    uint32_t acur[G::APW], wcur[G::WPW], adst[G::APW], wdst[G::WPW];
#pragma unroll
    for (int i = 0; i < G::APW; ++i) {
        const int slot = (wv * G::APW + i) * 64 + lane, pp = slot / G::LPR, piece = (slot % G::LPR) ^ G::swz(pp);
        acur[i] = FAR;
        if (pp < NPIX) {
            const int iy = y0 - 1 + pp / PW, ix = x0 - 1 + pp % PW;
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                acur[i] = (uint32_t)(((b * H + iy) * W + ix) * p.x_pix_stride + piece * 8) * 2u;
        }
        adst[i] = smem_base + (uint32_t)((wv * G::APW + i) * 1024);
    }
    const int Kp = NT * p.Cin;                 // elements of a packed weight row: [tap][Cin]
#pragma unroll
    for (int i = 0; i < G::WPW; ++i) {
        const int slot = (wv * G::WPW + i) * 64 + lane, row = slot / G::LPR, piece = (slot % G::LPR) ^ G::swz(row);
        wcur[i] = (n0 + row < p.N) ? (uint32_t)((((size_t)phase * p.N + n0 + row) * Kp + piece * 8) * 2) : FAR;
        wdst[i] = smem_base + (uint32_t)(2 * G::AB + (wv * G::WPW + i) * 1024);
    }
    const uint32_t w_tap = (uint32_t)(p.Cin * 2), w_chunk = (uint32_t)(CKD * 2) - (uint32_t)(NT - 1) * w_tap;     // next tap / tap 3 -> tap 0 of the next chunk
    auto dma_patch = [&](auto buf_c) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < G::APW; ++i) dma16_run<decltype(buf_c)::value * G::AB>(dx, adst[i], acur[i], (uint32_t)(CKD * 2));
    };
    auto dma_w = [&](auto ring_c) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < G::WPW; ++i) dma16_run<decltype(ring_c)::value * G::WB>(dw, wdst[i], wcur[i], w_tap);
    };
    int w_fr[2], xa[NT][2];       // fragment addresses of the 16-deep slice kk = 0 (slice kk: the same address ^ (kk << 5)), loop-invariant
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int row = wn0 + a * 32 + col;
        w_fr[a] = row * G::RB + ((hi ^ G::swz(row)) << 4);
    }
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const int q = wm0 + bb * 32 + cpix, r0 = (q / TW) * PW + (q % TW);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int rw = r0 + (py + (t >> 1)) * PW + (px + (t & 1));      // tap (dy, dx) of phase (py, px): patch rows + py + dy, columns + px + dx
            xa[t][bb] = rw * G::RB + ((hi ^ G::swz(rw)) << 4);
        }
    }
    const bool live = __builtin_amdgcn_readfirstlane((int)(n0 + (wv & 1) * 64 < p.N)) != 0;      // scalar: the whole wave or nothing

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
            zero_frag(acc[a][bb]);

    const std::integral_constant<int, 0> i0{}; const std::integral_constant<int, 1> i1{}; const std::integral_constant<int, 2> i2{};
    dma_patch(i0);
    dma_w(i0);
    dma_w(i1);
    dma_wait();
    __syncthreads();
    auto chunk = [&](auto j_c) __attribute__((always_inline)) {           // chunk 6 k + J: patch buffer J % 2, ring position (4 J) % 3
        constexpr int J = decltype(j_c)::value, AB = J & 1;
        const char* As = smem + AB * G::AB;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int cur = (NT * J + t) % 3, nxt = (NT * J + t + 2) % 3;           // (compile-time after unrolling)
            if (nxt == 0) dma_w(i0); else if (nxt == 1) dma_w(i1); else dma_w(i2);
            if (t == 1) {                      // (the piece just staged was tap 3: the next one is tap 0 of the next chunk)
#pragma unroll
                for (int i = 0; i < G::WPW; ++i) wcur[i] += w_chunk - w_tap;
                dma_patch(std::integral_constant<int, AB ^ 1>{});            // (always APW pieces: the counted waits rely on it)
            }
            if (live) {
                const char* Wsm = smem + 2 * G::AB + cur * G::WB;
                uint4 wf[2][2], xf[2][2];
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
                    for (int a = 0; a < 2; ++a) wf[kk][a] = *reinterpret_cast<const uint4*>(Wsm + (w_fr[a] ^ (kk * 32)));
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb) xf[kk][bb] = *reinterpret_cast<const uint4*>(As + (xa[t][bb] ^ (kk * 32)));
                }
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int bb = 0; bb < 2; ++bb) acc[a][bb] = E::mfma(wf[kk][a], xf[kk][bb], acc[a][bb]);
            }
            if (t == 1 || t == 2) dma_wait_keep_n<G::WPW + G::APW>(); else dma_wait_keep_n<G::WPW>();      // (derivation: head of the kernel)
            __syncthreads();
        }
    };
    {
        int left = nch;
#pragma unroll 1
        for (;;) {
            chunk(std::integral_constant<int, 0>{}); if (--left == 0) break;
            chunk(std::integral_constant<int, 1>{}); if (--left == 0) break;
            chunk(std::integral_constant<int, 2>{}); if (--left == 0) break;
            chunk(std::integral_constant<int, 3>{}); if (--left == 0) break;
            chunk(std::integral_constant<int, 4>{}); if (--left == 0) break;
            chunk(std::integral_constant<int, 5>{}); if (--left == 0) break;
        }
    }
    dma_wait();                  // pieces staged past the end are still landing: the epilogue reuses this LDS
    __syncthreads();

    // ---- epilogue: one 64-pixel wave-row group at a time through LDS, + bias, 16-byte stores to the phase's output pixels ----
    float* Cs = reinterpret_cast<float*>(smem);
    constexpr int CPR = BN / 8;
    const int cc = (tid % CPR) * 8, n = n0 + cc;
    const int nv = (n + 8 <= p.N) ? 8 : 4;
    float4 b0 = make_float4(0, 0, 0, 0), b1 = b0;
    if (p.bias != nullptr && n < p.N) {
        b0 = *reinterpret_cast<const float4*>(p.bias + n);
        if (nv == 8) b1 = *reinterpret_cast<const float4*>(p.bias + n + 4);
    }
    bf16_t* const outp = reinterpret_cast<bf16_t*>(p.out);
#pragma unroll
    for (int wr = 0; wr < 2; ++wr) {
        if ((wave >> 1) == wr) {
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                for (int a = 0; a < 2; ++a) acc_to_lds<CLD>(Cs, bb * 32 + cpix, wn0 + a * 32, hi, acc[a][bb]);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid + 256 * i) / CPR;                  // 0 .. 63 (the column block `cc` is the same for every i: 256 % CPR == 0)
            const int q = wr * EROWS + row;
            const int sy = y0 + q / TW, sx = x0 + q % TW;
            if (n >= p.N || sy >= H || sx >= W) continue;
            const size_t m = ((size_t)(b * 2 * H + 2 * sy + py)) * (size_t)(2 * W) + (size_t)(2 * sx + px);
            const float4 v0 = *reinterpret_cast<const float4*>(Cs + row * CLD + cc);
            const float4 v1 = *reinterpret_cast<const float4*>(Cs + row * CLD + cc + 4);
            const float v[8] = {v0.x + b0.x, v0.y + b0.y, v0.z + b0.z, v0.w + b0.w, v1.x + b1.x, v1.y + b1.y, v1.z + b1.z, v1.w + b1.w};
            bf16_t* dst = outp + m * (size_t)p.out_ld + n;
            if (nv == 8) *reinterpret_cast<uint4*>(dst) = pack8<F16>(v);
            else *reinterpret_cast<uint2*>(dst) = make_uint2(E::pack2(v[0], v[1]), E::pack2(v[2], v[3]));
        }
        if (wr == 0) __syncthreads();
    }
}

}  // namespace

// tile-padded multiply counts per image and output channel, in units of 128 pixels x one tap: the phase form runs 4 phases x 4 taps per
// 8 x 16 SOURCE tile, the 9-tap form 9 taps per 8 x 16 tile of the OUTPUT map
static long ups_phase_units(int Hin, int Win) { return 16L * ((Hin + TH - 1) / TH) * ((Win + TW - 1) / TW); }
static long ups_9tap_units(int Hout, int Wout) { return 9L * ((Hout + TH - 1) / TH) * ((Wout + TW - 1) / TW); }

// Upsample2D as four phase convolutions: p describes the 9-tap problem (taps = 9, K = 9 Cin, ups = 1), p.w holds the PHASE weights.
// What the kernel can RUN (the launcher's own check) ...
static bool ups_phase_can_run(const ConvGemmParams& p) {
    if (!(p.taps == 9 && p.stride == 1 && p.ups && !p.pad_br_only && p.Hin > 0 && p.Win > 0 && p.Hout == 2 * p.Hin && p.Wout == 2 * p.Win)) return false;
    if (p.Cin < CK || (p.Cin % CK) != 0 || p.K != 9 * p.Cin || p.N <= 0 || (p.N % 4) != 0 || p.M <= 0 || (p.M % (p.Hout * p.Wout)) != 0) return false;
    if (p.x_pix_stride != p.Cin || p.out_ld != p.N || p.out_f32 || p.mode != OUT_ROWMAJOR) return false;                 // contiguous 16-bit input and output
    if (p.dtype != IMD_DTYPE_BF16 && p.dtype != IMD_DTYPE_F16) return false;
    // bias only
    if (p.res != nullptr || p.res_rows != 0 || p.rowvec != nullptr || p.gn_a != nullptr || p.gn_b != nullptr || p.gn_stats_out != nullptr || p.gn_in_partial != nullptr ||
        p.gn_out_gamma != nullptr || p.act != ACT_NONE || p.split_k > 1 || p.out_scale != 1.0f)
        return false;
    const size_t xb = (size_t)(p.M / 4) * p.Cin * 2, wb = (size_t)16 * p.N * p.Cin * 2, ob = (size_t)p.M * p.N * 2;
    return xb < 0x80000000ull && wb < 0x80000000ull && ob < 0x80000000ull;
}

static long ups_phase_blocks(const ConvGemmParams& p) { return (long)(p.M / (p.Hout * p.Wout)) * 4 * halo_tiles(p.Hin, p.Win, p.N, TH, TW, BN); }

// ... and where it PAYS (the query a dispatcher asks): only there does a layer leave the 9-tap path, whose results it does not reproduce bit for bit
constexpr long UPS_PHASE_MIN_BLOCKS = 160;
bool imd_conv_ups_phase_supported_of(const ConvGemmParams& p) {
    if (!ups_phase_can_run(p)) return false;
    // The kernel takes no K slices, so a grid that leaves most CUs idle loses to the K-sliced 9-tap launch: measured 41.2 against 43.4 us (launch + finish) at
    // 80 workgroups (one image, 16 x 16 source, 1280 channels) -- no gain -- and 24.5 against 44.4 / 43.0 against 69.4 us at 160 (one image 32 x 32 x 640 / two
    // images 16 x 16 x 1280).  160 is the smallest grid at which a gain has been measured; smaller layers stay where they were
    if (ups_phase_blocks(p) < UPS_PHASE_MIN_BLOCKS) return false;
    // The phase form must do clearly fewer tile-padded multiplies than the 9-tap form.  It stages 4 weight tiles per patch fetch instead of 9
    // (about 18 % more staged bytes per MFMA), so its count is weighted 6 / 5: an 8 x 8 source (16 units against the 18 of its 16 x 16 output map:
    // the half-empty source tile eats the gain) is refused, the 2.25 x of whole tiles is not
    return 6 * ups_phase_units(p.Hin, p.Win) < 5 * ups_9tap_units(p.Hout, p.Wout);
}

int imd_launch_conv_ups_phase(const ConvGemmParams& p_in, hipStream_t s) {
    // (the launcher runs whatever the kernel computes correctly; whether the launch pays is the query's business)
    if (!ups_phase_can_run(p_in))
        return imd_set_error("conv_ups_phase: unsupported problem (needs 3x3 stride 1 with ups, Hout = 2 Hin, Wout = 2 Win, Cin %% 32 == 0, contiguous 16-bit input / output "
                             "< 2 GiB, bias only)");
    ConvGemmParams p = p_in;
    const unsigned tag = (unsigned)p_in.flags & IMD_TUNING_TAG_MASK;
    if (tag != 0 && tag != (unsigned)IMD_TUNING_PER_CALL)
        return imd_set_error("conv_ups_phase: flags = 0x%x on entry is neither 0 nor IMD_TUNING_PER_CALL | bits (an uninitialised parameter block?)", (unsigned)p_in.flags);
    const int gf = (tag == (unsigned)IMD_TUNING_PER_CALL) ? ((p_in.flags & 31) | (g_gemm_flags & ~31)) : g_gemm_flags;
    p.flags = (gf & 4) ? (4 | (gf & 16)) : 0;          // row-tile major: the four phases (and all channel tiles) of a pixel tile share one XCD's L2
    p.x_bytes = (uint32_t)((size_t)(p.M / 4) * p.Cin * 2);
    p.w_bytes = (uint32_t)((size_t)16 * p.N * p.Cin * 2);
    const bool h = p.dtype == IMD_DTYPE_F16;
    const long blocks = ups_phase_blocks(p);
    if (blocks > 0x7fffffffL) return imd_set_error("conv_ups_phase: grid too large");
    return tile_launch(h ? conv_ups_phase_kernel<true> : conv_ups_phase_kernel<false>, p, dim3((unsigned)blocks, (unsigned)1), 256, PD<32>::LDS, "conv_ups_phase", s);
}
