// guidance_rescale: the CFG rescale of Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", section 3.4
// (diffusers' rescale_noise_cfg) as ONE launch over the fp32 eps [2B, HW, 4] between the UNet and the step (gfx950) --
// imd_guidance_rescale_params.  For each latent row b whose phi is not 0, in fp32 (t = eps[b] cond, u = eps[B + b] uncond):
//   e   = u + g (t - u)                                 the guided prediction, the step kernels' expression: fmaf(g, t - u, u)
//   mu_t = (sum t) / N,  mu_e = (sum e) / N             N = 4 HW, a true division, once per row
//   S_t = sum (t - mu_t)^2,  S_e = sum (e - mu_e)^2     a second pass over the same values: centred
//   r   = sqrt(S_t / S_e)  (1 if S_e == 0),   f = phi r + (1 - phi)
//   eps[b] = eps[B + b] = f e
// Both halves receive f e, so the step that follows computes eps_u + g (eps_c - eps_u) = f e + g * 0 = f e whatever g it is given:
// no step kernel and no parameter block of theirs changes.  A row with phi == 0 is neither read nor written.
//
// This is the one CFG operation that is not element-wise: two reductions over a whole row.  ONE workgroup of 1024 threads (16 waves)
// owns one latent row; thread i owns the pixels (float4) i, i + 1024, i + 2048, ...  Up to GR_REG pixels per thread (rows of up to
// 8192 pixels: 512 x 640 and below) t and e stay in registers between the three passes; longer rows are read again (a row is 32 HW
// bytes: 640 KB at 1024 x 1280, L2-resident).  Every access is one float4.
// Reduction order -- a function of HW ALONE, never of B, of the row index or of which other rows are active (no atomics, no
// arrival-order combine): per thread its pixels in ascending order, each pixel folded to one value first; then the xor butterfly over
// the 64 lanes (offsets 32, 16, .., 1); then the 16 wave partials in LDS, added in ascending wave order by every thread.
// The longest chain of sequential fp32 additions is therefore  L(HW) = ceil(HW / 1024) + 3 + 6 + 15  (the pixels of a thread, the
// three additions inside a pixel's squared deviations, the butterfly, the wave partials); both routes share the order, hence the bits.
#include <math.h>

#include "common.h"
#include "imd_kernels.h"

namespace {

constexpr int GR_THREADS = 1024;
constexpr int GR_WAVES = GR_THREADS / 64;
constexpr int GR_REG = 8;                                  // pixels per thread held in registers: 2 planes x 8 float4 = 64 VGPRs

// block-wide sum, the same bits in every thread; `lds` holds GR_WAVES floats (the leading barrier frees it from the previous use)
__device__ __forceinline__ float gr_block_sum(float v, float* lds) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = lds[0];
#pragma unroll
    for (int w = 1; w < GR_WAVES; ++w) s += lds[w];
    return s;
}

__device__ __forceinline__ float4 gr_guided(const float4 t, const float4 u, float g) {
    return make_float4(fmaf(g, t.x - u.x, u.x), fmaf(g, t.y - u.y, u.y), fmaf(g, t.z - u.z, u.z), fmaf(g, t.w - u.w, u.w));
}

__device__ __forceinline__ float gr_sum4(const float4 v) { return (v.x + v.y) + (v.z + v.w); }

// the squared deviations of one pixel: explicit fmaf, so both routes round alike whatever the compiler would contract
__device__ __forceinline__ float gr_sq4(const float4 v, float mu) {
    const float a = v.x - mu, b = v.y - mu, c = v.z - mu, d = v.w - mu;
    return fmaf(a, a, fmaf(b, b, fmaf(c, c, d * d)));
}

__device__ __forceinline__ float gr_factor(float s_t, float s_e, float phi) {
    const float r = s_e == 0.f ? 1.f : sqrtf(s_t / s_e);
    return fmaf(phi, r, 1.f - phi);
}

// REG: the row fits GR_REG pixels per thread (HW <= GR_THREADS * GR_REG) and is read once
template <bool REG>
__global__ __launch_bounds__(GR_THREADS) void guidance_rescale_kernel(const imd_guidance_rescale_params p) {
    __shared__ float lds[GR_WAVES];
    const int b = blockIdx.x;                              // the latent row of this workgroup
    const float phi = p.rescale_rows ? p.rescale_rows[b] : p.rescale;
    if (phi == 0.f) return;                                // (uniform over the workgroup, ahead of every barrier) not read, not written
    const float g = p.guidance_rows ? p.guidance_rows[b] : p.guidance;
    const int HW = p.HW;
    float4* __restrict__ tp = reinterpret_cast<float4*>(p.eps) + (size_t)b * HW;
    float4* __restrict__ up = reinterpret_cast<float4*>(p.eps) + ((size_t)p.B + b) * HW;
    const float n = 4.f * (float)HW;
    const int tid = threadIdx.x;

    if constexpr (REG) {
        float4 t[GR_REG], e[GR_REG];
        float st = 0.f, se = 0.f;
#pragma unroll
        for (int k = 0; k < GR_REG; ++k) {
            const int j = tid + k * GR_THREADS;
            if (j < HW) {
                t[k] = tp[j];
                e[k] = gr_guided(t[k], up[j], g);
                st += gr_sum4(t[k]);
                se += gr_sum4(e[k]);
            }
        }
        const float mu_t = gr_block_sum(st, lds) / n, mu_e = gr_block_sum(se, lds) / n;
        float qt = 0.f, qe = 0.f;
#pragma unroll
        for (int k = 0; k < GR_REG; ++k) {
            if (tid + k * GR_THREADS < HW) {
                qt += gr_sq4(t[k], mu_t);
                qe += gr_sq4(e[k], mu_e);
            }
        }
        const float f = gr_factor(gr_block_sum(qt, lds), gr_block_sum(qe, lds), phi);
#pragma unroll
        for (int k = 0; k < GR_REG; ++k) {
            const int j = tid + k * GR_THREADS;
            if (j < HW) {
                const float4 o = make_float4(f * e[k].x, f * e[k].y, f * e[k].z, f * e[k].w);
                tp[j] = o;
                up[j] = o;
            }
        }
    } else {
        float st = 0.f, se = 0.f;
        for (int j = tid; j < HW; j += GR_THREADS) {
            const float4 t = tp[j];
            st += gr_sum4(t);
            se += gr_sum4(gr_guided(t, up[j], g));
        }
        const float mu_t = gr_block_sum(st, lds) / n, mu_e = gr_block_sum(se, lds) / n;
        float qt = 0.f, qe = 0.f;
        for (int j = tid; j < HW; j += GR_THREADS) {
            const float4 t = tp[j];
            qt += gr_sq4(t, mu_t);
            qe += gr_sq4(gr_guided(t, up[j], g), mu_e);
        }
        const float f = gr_factor(gr_block_sum(qt, lds), gr_block_sum(qe, lds), phi);
        for (int j = tid; j < HW; j += GR_THREADS) {       // every thread reads its own pixels before it overwrites them
            const float4 e = gr_guided(tp[j], up[j], g);
            const float4 o = make_float4(f * e.x, f * e.y, f * e.z, f * e.w);
            tp[j] = o;
            up[j] = o;
        }
    }
}

}  // namespace

int imd_launch_guidance_rescale(const imd_guidance_rescale_params& p, hipStream_t s) {
    auto misaligned = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
    if (!p.eps) return imd_set_error("guidance_rescale: null eps");
    if (misaligned(p.eps, 16)) return imd_set_error("guidance_rescale: eps must be 16-byte aligned");
    if (misaligned(p.guidance_rows, 4) || misaligned(p.rescale_rows, 4))
        return imd_set_error("guidance_rescale: guidance_rows and rescale_rows must be 4-byte aligned");
    if (p.B < 1 || p.HW < 1) return imd_set_error("guidance_rescale: empty latent (B = %d, HW = %d)", p.B, p.HW);
    if (!p.rescale_rows && !(isfinite(p.rescale) && p.rescale >= 0.f && p.rescale <= 1.f))
        return imd_set_error("guidance_rescale: rescale (%g) must be a finite value in [0, 1]", (double)p.rescale);
    if (!p.guidance_rows && !isfinite(p.guidance)) return imd_set_error("guidance_rescale: guidance (%g) must be finite", (double)p.guidance);
    if (!p.rescale_rows && p.rescale == 0.f) return 0;     // no row asks for it: nothing to launch
    if (p.HW <= GR_THREADS * GR_REG) hipLaunchKernelGGL(guidance_rescale_kernel<true>, dim3((unsigned)p.B), dim3(GR_THREADS), 0, s, p);
    else hipLaunchKernelGGL(guidance_rescale_kernel<false>, dim3((unsigned)p.B), dim3(GR_THREADS), 0, s, p);
    return imd_check_launch("guidance_rescale");
}
