// FreeU (Si et al., CVPR 2024; diffusers 0.24 utils/torch_utils.py::apply_freeu / fourier_filter, restated) inside the skip concatenation of an
// up block: out = cat([a with its lower channel half scaled, fourier_filter(b (+ b_add))], channel) for NHWC 16-bit tensors, plus the GroupNorm(G)
// statistics of the stored tensor -- imd_concat2_gn_stats with the two FreeU operations applied on the way, still one launch per concat site.
//
// The filter.  fourier_filter(x, threshold = 1, scale = s) multiplies the centred 2 x 2 block of the shifted spectrum by s: the frequencies
// ky in {0, -1 mod H}, kx in {0, -1 mod W} as SETS (one row frequency when H = 1, 0 and Nyquist when H = 2).  For a real map that is
//     y[n, m] = x[n, m] + (s - 1) / (H W) * sum over the (ky, kx) of  A cos(phi) + B sin(phi),   phi = 2 pi (ky n / H + kx m / W),
//     A = sum x cos(phi),  B = sum x sin(phi)
// and A cos + B sin is even in phi, so the waves are taken at +1: the mean, the row wave 2 pi n / H (H > 1), the column wave 2 pi m / W (W > 1) and
// ONE diagonal wave 2 pi (n / H + m / W) (both): seven real sums per map, then one pass over its pixels.  No FFT: the maps are 8 x 8 .. 32 x 40.
//
// Mapping.  A map needs its sums before any pixel of it is written, so the owner of a map's channels reads it twice: one workgroup per (image,
// FU_COLS vector columns of 8 channels) over ALL H W pixels -- thread = (column, pixel lane), FU_LANES pixel lanes, 16-byte loads and stores.  The
// second read of the <= 1280 px x 64 B a workgroup owns comes from the L2.  Nothing is shared between workgroups.
//   pass 1 (columns of the skip only; skipped when skip_scale == 1): v = round16(b + b_add) and the seven sums of every channel in registers
//          (56 fp32 accumulators per thread), folded over the pixel lanes by 4 xor-shuffles inside the wave and over the 4 waves through the LDS;
//   pass 2: the value is rebuilt, corrected (skip) / scaled or copied (backbone), rounded ONCE, stored, and the rounded value enters the
//          GroupNorm sums of the one or two groups its vector feeds (the split of gn_stats_kernel).
// Twiddles: cos / sin of 2 pi k / H and 2 pi k / W from a per-workgroup LDS table built with sincospif (exact at quarter turns); the diagonal
// wave is the angle sum of the two table entries -- no phase is accumulated from pixel to pixel.
//
// Statistics.  Workgroup w owns vector columns 4 w .. 4 w + 3; group g lies in workgroups wlo(g) .. whi(g).  Partial slot (w - wlo(g)) of group g
// is written by workgroup w, and workgroup whi(g) zero-fills the slots up to nparts = max over g of the span (imd_concat2_freeu_parts): the
// [B][nparts][G][2] layout imd_groupnorm folds through imd_groupnorm_params.nparts, every float of it written, no atomics, deterministic.
#include <math.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "imd_kernels.h"

namespace {

constexpr int FU_COLS = 4;                         // 8-channel vector columns per workgroup (64 B of every pixel)
constexpr int FU_LANES = 64;                       // pixel lanes
constexpr int FU_THREADS = FU_COLS * FU_LANES;     // 4 waves; a wave holds 16 pixel lanes x 4 columns
constexpr int FU_WAVES = FU_THREADS / 64;
constexpr int FU_MAX_DIM = 256;                    // bound of the twiddle table: H, W <= 256
constexpr int FU_SUMS = 7;                         // mean; row cos, sin; column cos, sin; diagonal cos, sin

struct FreeuParams {
    const bf16_t* a; const bf16_t* b; const bf16_t* b_add; bf16_t* out; float* part;
    int Ca, Cb, B, H, W, G, nparts;
    float backbone_scale;
    float k;                                       // (skip_scale - 1) / (H W); 0 = no filter
};

__host__ __device__ inline int fu_wlo(int g, int cpg) { return (g * cpg / 8) / FU_COLS; }
__host__ __device__ inline int fu_whi(int g, int cpg) { return (((g + 1) * cpg - 1) / 8) / FU_COLS; }

template <bool F16>
__global__ __launch_bounds__(FU_THREADS) void concat2_freeu_kernel(const FreeuParams p) {
    __shared__ float tw[4][FU_MAX_DIM];                                  // cos H, sin H, cos W, sin W
    __shared__ float red[FU_WAVES][FU_COLS][FU_SUMS * 8];
    __shared__ float tot[FU_COLS][FU_SUMS * 8];
    __shared__ float sred[FU_WAVES][FU_COLS][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = tid % FU_COLS, pl = tid / FU_COLS;
    const int wg = blockIdx.x, img = blockIdx.y;
    const int C = p.Ca + p.Cb, vpp = C / 8, HW = p.H * p.W;
    const int vec = wg * FU_COLS + col;
    const bool valid = vec < vpp;
    const int c0 = vec * 8;
    const bool from_a = c0 < p.Ca;
    const bool skip_col = valid && !from_a;
    const bool filter = p.k != 0.f && (wg * FU_COLS + FU_COLS) * 8 > p.Ca;       // (workgroup-uniform: some column of it belongs to the skip)
    const int cs = from_a ? c0 : c0 - p.Ca;
    const int ld = from_a ? p.Ca : p.Cb;
    const bf16_t* src = (from_a ? p.a : p.b) + (size_t)img * HW * ld + cs;
    const bf16_t* add = (skip_col && p.b_add) ? p.b_add + (size_t)img * HW * p.Cb + cs : nullptr;

    // v = round16(b + b_add) (concat2_kernel's arithmetic: summed in fp32, rounded once), or the operand itself
    auto load_v = [&](int pix, float* x) -> uint4 {
        uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)pix * ld);
        if (add) {
            const uint4 w = *reinterpret_cast<const uint4*>(add + (size_t)pix * ld);
            float s[8], t[8];
            unpack8<F16>(v, s);
            unpack8<F16>(w, t);
            v = make_uint4(El<F16>::pack2(s[0] + t[0], s[1] + t[1]), El<F16>::pack2(s[2] + t[2], s[3] + t[3]),
                           El<F16>::pack2(s[4] + t[4], s[5] + t[5]), El<F16>::pack2(s[6] + t[6], s[7] + t[7]));
        }
        unpack8<F16>(v, x);
        return v;
    };

    float coef[FU_SUMS * 8];
#pragma unroll
    for (int i = 0; i < FU_SUMS * 8; ++i) coef[i] = 0.f;

    if (filter) {
        for (int i = tid; i < p.H; i += FU_THREADS) sincospif(2.0f * (float)i / (float)p.H, &tw[1][i], &tw[0][i]);
        for (int i = tid; i < p.W; i += FU_THREADS) sincospif(2.0f * (float)i / (float)p.W, &tw[3][i], &tw[2][i]);
        __syncthreads();
        float acc[FU_SUMS * 8];
#pragma unroll
        for (int i = 0; i < FU_SUMS * 8; ++i) acc[i] = 0.f;
        if (skip_col) {
            for (int pix = pl; pix < HW; pix += FU_LANES) {
                float x[8];
                load_v(pix, x);
                const int n = pix / p.W, m = pix - n * p.W;
                const float cr = tw[0][n], sr = tw[1][n], cc = tw[2][m], sc = tw[3][m];
                const float cd = cr * cc - sr * sc, sd = sr * cc + cr * sc;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    acc[e] += x[e];
                    acc[8 + e] += x[e] * cr;  acc[16 + e] += x[e] * sr;
                    acc[24 + e] += x[e] * cc; acc[32 + e] += x[e] * sc;
                    acc[40 + e] += x[e] * cd; acc[48 + e] += x[e] * sd;
                }
            }
        }
        // pixel lanes of one column sit FU_COLS lanes apart inside the wave
#pragma unroll
        for (int i = 0; i < FU_SUMS * 8; ++i) {
#pragma unroll
            for (int off = FU_COLS; off < 64; off <<= 1) acc[i] += __shfl_xor(acc[i], off);
        }
        if (lane < FU_COLS) {
#pragma unroll
            for (int i = 0; i < FU_SUMS * 8; ++i) red[wave][col][i] = acc[i];
        }
        __syncthreads();
        if (tid < FU_COLS * FU_SUMS * 8) {
            const int cl = tid / (FU_SUMS * 8), i = tid % (FU_SUMS * 8);
            float t = ((red[0][cl][i] + red[1][cl][i]) + (red[2][cl][i] + red[3][cl][i])) * p.k;
            // the frequency SETS: no row wave on a one-row map, no column wave on a one-column map, the diagonal only with both
            const int kind = i / 8;
            if (p.H == 1 && (kind == 1 || kind == 2 || kind >= 5)) t = 0.f;
            if (p.W == 1 && kind >= 3) t = 0.f;
            tot[cl][i] = t;
        }
        __syncthreads();
        if (skip_col) {
#pragma unroll
            for (int i = 0; i < FU_SUMS * 8; ++i) coef[i] = tot[col][i];
        }
    }

    // pass 2: store, and the GroupNorm sums of the ROUNDED values
    const int cpg = p.part ? C / p.G : 8;
    const int g0 = c0 / cpg;
    const int split = min(8, (g0 + 1) * cpg - c0);               // channels [0, split) -> g0, the rest -> g0 + 1
    float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
    if (valid) {
        const bool scaled = from_a && c0 < p.Ca / 2;
        bf16_t* ob = p.out + (size_t)img * HW * C + c0;
        for (int pix = pl; pix < HW; pix += FU_LANES) {
            float x[8];
            uint4 v = load_v(pix, x);
            if (scaled) {
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] *= p.backbone_scale;
                v = pack8<F16>(x);
            } else if (skip_col && filter) {
                const int n = pix / p.W, m = pix - n * p.W;
                const float cr = tw[0][n], sr = tw[1][n], cc = tw[2][m], sc = tw[3][m];
                const float cd = cr * cc - sr * sc, sd = sr * cc + cr * sc;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    x[e] += coef[e] + (coef[8 + e] * cr + coef[16 + e] * sr) + (coef[24 + e] * cc + coef[32 + e] * sc) + (coef[40 + e] * cd + coef[48 + e] * sd);
                v = pack8<F16>(x);
            }
            *reinterpret_cast<uint4*>(ob + (size_t)pix * C) = v;
            if (p.part) {
                float f[8];
                unpack8<F16>(v, f);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e < split) { s0 += f[e]; q0 += f[e] * f[e]; }
                    else           { s1 += f[e]; q1 += f[e] * f[e]; }
                }
            }
        }
    }
    if (!p.part) return;                                         // (uniform)
#pragma unroll
    for (int off = FU_COLS; off < 64; off <<= 1) {
        s0 += __shfl_xor(s0, off); q0 += __shfl_xor(q0, off);
        s1 += __shfl_xor(s1, off); q1 += __shfl_xor(q1, off);
    }
    if (lane < FU_COLS) { sred[wave][col][0] = s0; sred[wave][col][1] = q0; sred[wave][col][2] = s1; sred[wave][col][3] = q1; }
    __syncthreads();
    // thread t folds group gfirst + t of the groups this workgroup's channels touch (at most 32 / cpg + 2)
    const int cfirst = wg * FU_COLS * 8, clast = min(cfirst + FU_COLS * 8, C) - 1;
    const int g = cfirst / cpg + tid;
    if (g <= clast / cpg) {
        float S = 0.f, Q = 0.f;
        for (int cl = 0; cl < FU_COLS; ++cl) {
            const int v = wg * FU_COLS + cl;
            if (v >= vpp) break;
            const int vg0 = (v * 8) / cpg;
            for (int w = 0; w < FU_WAVES; ++w) {
                const float* e = sred[w][cl];
                if (vg0 == g) { S += e[0]; Q += e[1]; }
                else if (vg0 + 1 == g) { S += e[2]; Q += e[3]; }
            }
        }
        const int wlo = fu_wlo(g, cpg), whi = fu_whi(g, cpg);
        float* dst = p.part + ((size_t)img * p.nparts * p.G + g) * 2;
        const size_t slot_ld = (size_t)p.G * 2;
        dst[(wg - wlo) * slot_ld] = S;
        dst[(wg - wlo) * slot_ld + 1] = Q;
        if (wg == whi)
            for (int sl = whi - wlo + 1; sl < p.nparts; ++sl) { dst[sl * slot_ld] = 0.f; dst[sl * slot_ld + 1] = 0.f; }
    }
}

}  // namespace

int imd_concat2_freeu_parts_of(int B, int H, int W, int Ca, int Cb, int G) {
    if (B < 1 || H < 1 || W < 1 || Ca <= 0 || Cb <= 0 || Ca % 16 || Cb % 8 || G < 1 || G > 64) return 0;
    const long C = (long)Ca + Cb;
    if (C > (1 << 20) || C % G) return 0;
    const int cpg = (int)(C / G);
    if (cpg < 4 || (cpg < 8 && cpg != 4)) return 0;           // groupnorm's own condition: an 8-channel vector spans at most two groups
    int n = 1;
    for (int g = 0; g < G; ++g) n = std::max(n, fu_whi(g, cpg) - fu_wlo(g, cpg) + 1);
    return n;
}

int imd_launch_concat2_freeu(const bf16_t* a, int Ca, const bf16_t* b, int Cb, const bf16_t* b_add, bf16_t* out, int B, int H, int W, int b_batch, int G,
                             float* part, float backbone_scale, float skip_scale, int dtype, hipStream_t s) {
    if (!a || !b || !out) return imd_set_error("concat2 + freeu: null pointer (a, b and out are required)");
    if (Ca <= 0 || Cb <= 0 || Ca % 16 || Cb % 8 || (long)Ca + Cb > (1 << 20))
        return imd_set_error("concat2 + freeu: channel counts: Ca must be a positive multiple of 16 (its lower half is scaled in 8-channel vectors) and Cb of 8 (got %d + %d)", Ca, Cb);
    if (B < 1 || H < 1 || W < 1) return imd_set_error("concat2 + freeu: empty tensor (B = %d, H = %d, W = %d must be >= 1)", B, H, W);
    if (B > 65535) return imd_set_error("concat2 + freeu: at most 65535 images per launch (got %d)", B);
    if (H > FU_MAX_DIM || W > FU_MAX_DIM) return imd_set_error("concat2 + freeu: map %d x %d exceeds the twiddle table bound of %d per side", H, W, FU_MAX_DIM);
    if (b_batch != B) return imd_set_error("concat2 + freeu: b_batch (%d) must equal B (%d): every image filters its own skip", b_batch, B);
    if (dtype != IMD_DTYPE_BF16 && dtype != IMD_DTYPE_F16) return imd_set_error("concat2 + freeu: unknown dtype %d", dtype);
    if (!(backbone_scale > 0.f) || !(skip_scale > 0.f) || !std::isfinite(backbone_scale) || !std::isfinite(skip_scale))
        return imd_set_error("concat2 + freeu: scales must be finite and > 0 (backbone_scale = %g, skip_scale = %g)", (double)backbone_scale, (double)skip_scale);
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)b_add | (uintptr_t)out) % 16 || (uintptr_t)part % 4)
        return imd_set_error("concat2 + freeu: misaligned pointer (a, b, b_add and out need 16-byte alignment, part 4-byte)");
    int nparts = 0;
    if (part) {
        if (G < 1 || (Ca + Cb) % G) return imd_set_error("concat2 + freeu: statistics: Ca + Cb (%d) must be a multiple of G (%d)", Ca + Cb, G);
        nparts = imd_concat2_freeu_parts_of(B, H, W, Ca, Cb, G);
        if (nparts == 0) return imd_set_error("concat2 + freeu: statistics: G (%d) must be <= 64 and the channels per group (%d) 4 or >= 8", G, (Ca + Cb) / G);
    }
    FreeuParams p{};
    p.a = a; p.b = b; p.b_add = b_add; p.out = out; p.part = part;
    p.Ca = Ca; p.Cb = Cb; p.B = B; p.H = H; p.W = W; p.G = G; p.nparts = nparts;
    p.backbone_scale = backbone_scale;
    p.k = skip_scale == 1.0f ? 0.f : (float)(((double)skip_scale - 1.0) / ((double)H * (double)W));
    const dim3 grid(((Ca + Cb) / 8 + FU_COLS - 1) / FU_COLS, B);
    if (dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(concat2_freeu_kernel<true>, grid, dim3(FU_THREADS), 0, s, p);
    else hipLaunchKernelGGL(concat2_freeu_kernel<false>, grid, dim3(FU_THREADS), 0, s, p);
    return imd_check_launch("concat2 + freeu");
}
