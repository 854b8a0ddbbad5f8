// unipc_step: one denoising step of the UniPC multistep sampler (Zhao et al. 2023; diffusers==0.24.0 UniPCMultistepScheduler.step) as
// ONE HBM-bound launch over the [B, HW, 4] latent (gfx950) -- imd_unipc_params.  Per element, in fp32:
//   e  = eps_u + g (eps_c - eps_u)                              classifier-free guidance
//   m  = m_x z + m_e e                                          the x0 prediction made at this position (convert_model_output)
//   s' = s_x z + s_m m + sum_k s_h[k] H[k]                      UniC: the corrected sample, the library's last_sample (no corrector: s' = z)
//   z' = z_s s' + z_m m + sum_k z_h[k] H[k]                     UniP from the value s' JUST computed
//   z' = (1 - mask) (b_img z_img + b_noise blend_noise) + mask z'      the inpainting blend: on z' only, never on s'
//   z <- z';  H[store_m] <- m;  H[store_s] <- s';  x_next[both CFG halves] <- 16-bit(in_scale z'), channels 4..7 = 0
// imd_sampler_step keeps ONE derived quantity per step; UniPC keeps two (m and s'), and s' is an intermediate of the same step's
// predictor, hence a kernel of its own with two affine outputs.  Everything else is sampler_step_kernel's (elementwise.hip): one thread
// per pixel (4 channels = one float4), 256 threads, a grid-stride loop, one uint4 store per CFG half of x_next, history slot k = the
// float4 array hist + k * (rows of z) * HW, a slot whose coefficient is 0 in BOTH s_h and z_h is not read, and every thread reads its
// element of every slot before it stores (a slot may be read and overwritten by one launch).
// Algorithmic traffic per latent element: 3 fp32 reads + 3 fp32 writes + 2 x 4 B of next-input writes, + 1 read per history slot with
// a coefficient (at most 4), + 3 reads with the blend.
//
// The per-pixel arithmetic is unipc_pixel(), written ONCE with explicit fmaf for every multiply-add: no product-sum pair is left for
// the compiler to contract or not, so the three kernels that inline it (coefficients from the parameter block or 19 device floats;
// per latent row; per row through a row -> slot map) round identically wherever they describe the same step.
#include "common.h"
#include "imd_kernels.h"

namespace {

struct UnipcCoefs {
    float m_x, m_e, s_x, s_m;
    float s_h[4];
    float z_s, z_m;
    float z_h[4];
    float b_img, b_noise, in_scale;
    int store_m, store_s;
};

// the 19 floats of IMD_UNIPC_COEFS order (a device block, or the head of a coefficient row); a store slot outside 0..K-1 stores nothing
__device__ __forceinline__ UnipcCoefs unipc_coefs_from(const float* __restrict__ c, int K) {
    UnipcCoefs o;
    o.m_x = c[0]; o.m_e = c[1]; o.s_x = c[2]; o.s_m = c[3];
    o.s_h[0] = c[4]; o.s_h[1] = c[5]; o.s_h[2] = c[6]; o.s_h[3] = c[7];
    o.z_s = c[8]; o.z_m = c[9];
    o.z_h[0] = c[10]; o.z_h[1] = c[11]; o.z_h[2] = c[12]; o.z_h[3] = c[13];
    o.b_img = c[14]; o.b_noise = c[15]; o.in_scale = c[16];
    o.store_m = (int)c[17]; o.store_s = (int)c[18];
    if (o.store_m < 0 || o.store_m >= K) o.store_m = -1;
    if (o.store_s < 0 || o.store_s >= K) o.store_s = -1;
    return o;
}

// One pixel.  `i` / `total` address what the forward produced and consumes (eps, x_next: batch ROWS), `si` / `stotal` what belongs to the
// request (z, the history planes, the blend operands: SLOTS); without a slot map the two pairs are equal.
template <bool F16>
__device__ __forceinline__ void unipc_pixel(const UnipcParams& p, const UnipcCoefs& c, float g, long i, long total, long si, long stotal) {
    const float4 z = reinterpret_cast<const float4*>(p.z)[si];
    const float4 ec = reinterpret_cast<const float4*>(p.eps)[i];
    const float4 eu = reinterpret_cast<const float4*>(p.eps)[i + total];
    const float zz[4] = {z.x, z.y, z.z, z.w};
    const float cc[4] = {ec.x, ec.y, ec.z, ec.w};
    const float uu[4] = {eu.x, eu.y, eu.z, eu.w};
    float hs[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < p.K && (c.s_h[k] != 0.f || c.z_h[k] != 0.f)) h = reinterpret_cast<const float4*>(p.hist)[(long)k * stotal + si];
        hs[k][0] = h.x; hs[k][1] = h.y; hs[k][2] = h.z; hs[k][3] = h.w;
    }
    float mk = 1.f;
    float zi[4] = {0, 0, 0, 0}, nz[4] = {0, 0, 0, 0};
    if (p.mask) {
        mk = p.mask[si];
        const float4 a = reinterpret_cast<const float4*>(p.z_img)[si];
        const float4 n = reinterpret_cast<const float4*>(p.blend_noise)[si];
        zi[0] = a.x; zi[1] = a.y; zi[2] = a.z; zi[3] = a.w;
        nz[0] = n.x; nz[1] = n.y; nz[2] = n.z; nz[3] = n.w;
    }
    float mm[4], ss[4], zo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float eps = fmaf(g, cc[e] - uu[e], uu[e]);
        const float m = fmaf(c.m_e, eps, c.m_x * zz[e]);
        float s = fmaf(c.s_m, m, c.s_x * zz[e]);
#pragma unroll
        for (int k = 0; k < 4; ++k) s = fmaf(c.s_h[k], hs[k][e], s);
        float zn = fmaf(c.z_m, m, c.z_s * s);
#pragma unroll
        for (int k = 0; k < 4; ++k) zn = fmaf(c.z_h[k], hs[k][e], zn);
        if (p.mask) {
            const float proper = fmaf(c.b_noise, nz[e], c.b_img * zi[e]);
            zn = fmaf(mk, zn, (1.f - mk) * proper);
        }
        mm[e] = m; ss[e] = s; zo[e] = zn;
    }
    reinterpret_cast<float4*>(p.z)[si] = make_float4(zo[0], zo[1], zo[2], zo[3]);
    if (c.store_m >= 0) reinterpret_cast<float4*>(p.hist)[(long)c.store_m * stotal + si] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    if (c.store_s >= 0) reinterpret_cast<float4*>(p.hist)[(long)c.store_s * stotal + si] = make_float4(ss[0], ss[1], ss[2], ss[3]);
    if (p.x_next) {
        // (the pack expression of imd_session_input_rows: given this step's in_scale that launch reproduces these bytes)
        const uint4 o = make_uint4(El<F16>::pack2(c.in_scale * zo[0], c.in_scale * zo[1]), El<F16>::pack2(c.in_scale * zo[2], c.in_scale * zo[3]), 0u, 0u);
        reinterpret_cast<uint4*>(p.x_next)[i] = o;
        reinterpret_cast<uint4*>(p.x_next)[i + total] = o;
    }
}

// scalar form: one coefficient block for the whole latent, from the parameter block or from p.coefs (19 device floats: a captured step
// holds nothing that changes between replays)
template <bool F16>
__global__ __launch_bounds__(256) void unipc_step_kernel(const UnipcParams p) {
    const long total = (long)p.B * p.HW;                   // one thread per pixel (4 channels = 16 B)
    UnipcCoefs c;
    if (p.coefs) c = unipc_coefs_from(p.coefs, p.K);
    else {
        c.m_x = p.m_x; c.m_e = p.m_e; c.s_x = p.s_x; c.s_m = p.s_m;
        c.z_s = p.z_s; c.z_m = p.z_m;
#pragma unroll
        for (int k = 0; k < 4; ++k) { c.s_h[k] = p.s_h[k]; c.z_h[k] = p.z_h[k]; }
        c.b_img = p.b_img; c.b_noise = p.b_noise; c.in_scale = p.in_scale;
        c.store_m = p.store_m; c.store_s = p.store_s;      // (checked by the launcher: -1..K-1, distinct)
    }
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const float g = p.guidance_rows ? p.guidance_rows[i / p.HW] : p.guidance;     // the latent row of this pixel
        unipc_pixel<F16>(p, c, g, i, total, i, total);
    }
}

// rows form: the block PER LATENT ROW, IMD_UNIPC_ROW_FLOATS = 24 floats (six float4) at coef_rows + 24 b: [0..18] the block, [19] active.
// An inactive row is skipped whole -- no load and no store of z, eps, the history or x_next.  With ONE trailing UnipcSlotMap argument it
// is the rows_at form of a compacting session (the sampler_step_rows_kernel idiom): row r carries the request of slot row_slot[r]; a row
// whose slot is outside [0, slots) is skipped BEFORE anything is addressed through it, so whatever the device map holds the kernel stays
// inside its buffers.  The coefficient loads are wave-uniform at HW >= 64 and hit two cache lines.
struct UnipcSlotMap {
    const int* row_slot;                                   // DEVICE [B]: the slot of every batch row
    int slots;
};

template <bool F16, typename... Map>
__global__ __launch_bounds__(256) void unipc_step_rows_kernel(const UnipcParams p, const float* __restrict__ coef_rows, const Map... map) {
    static_assert(sizeof...(Map) <= 1, "row == slot (no map) or one UnipcSlotMap");
    const long total = (long)p.B * p.HW;
    long stotal = total;
    if constexpr (sizeof...(Map) == 1) stotal = (((long)map.slots * p.HW), ...);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long b = i / p.HW;                           // the batch row of this pixel
        long si = i;                                       // ... and the pixel in its slot
        if constexpr (sizeof...(Map) == 1) {
            const int slot = (map.row_slot[b], ...);
            if (slot < 0 || slot >= (map.slots, ...)) continue;          // idle row
            si = (long)slot * p.HW + (i - b * p.HW);
        }
        const float4* row = reinterpret_cast<const float4*>(coef_rows) + b * (IMD_UNIPC_ROW_FLOATS / 4);
        const float4 r4 = row[4];
        if (r4.w == 0.f) continue;                         // inactive: neither read nor written
        const float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
        const float blk[IMD_UNIPC_COEFS + 1] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w,
                                                r4.x, r4.y, r4.z, r4.w};
        const UnipcCoefs c = unipc_coefs_from(blk, p.K);
        const float g = p.guidance_rows ? p.guidance_rows[b] : p.guidance;
        unipc_pixel<F16>(p, c, g, i, total, si, stotal);
    }
}

inline unsigned unipc_grid(long work_items) {
    long blocks = (work_items + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

// what the three entry points refuse alike (`rows`: the coefficients, store slots included, live in device memory)
int unipc_step_refusal(const UnipcParams& p, const char* what, bool rows) {
    auto misaligned = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
    if (p.B <= 0 || p.HW <= 0) return imd_set_error("%s: empty latent", what);
    if (p.K < 0 || p.K > IMD_SAMPLER_MAX_HISTORY) return imd_set_error("%s: K (%d) must be 0..%d history slots", what, p.K, IMD_SAMPLER_MAX_HISTORY);
    if (p.K > 0 && !p.hist) return imd_set_error("%s: K = %d history slots without a history buffer", what, p.K);
    if (!rows && !p.coefs) {
        if (p.store_m < -1 || p.store_m >= p.K) return imd_set_error("%s: store_m slot %d outside -1..%d", what, p.store_m, p.K - 1);
        if (p.store_s < -1 || p.store_s >= p.K) return imd_set_error("%s: store_s slot %d outside -1..%d", what, p.store_s, p.K - 1);
        if (p.store_m >= 0 && p.store_m == p.store_s) return imd_set_error("%s: store_m and store_s name the same slot %d", what, p.store_m);
    }
    if (p.mask && (!p.z_img || !p.blend_noise)) return imd_set_error("%s: inpaint mask given without image latents / blend noise", what);
    if (misaligned(p.z, 16) || misaligned(p.eps, 16) || misaligned(p.x_next, 16) || misaligned(p.hist, 16) || misaligned(p.z_img, 16) ||
        misaligned(p.blend_noise, 16))
        return imd_set_error("%s: z, eps, x_next, hist, z_img and blend_noise must be 16-byte aligned", what);
    if (misaligned(p.mask, 4) || misaligned(p.guidance_rows, 4) || (!rows && misaligned(p.coefs, 4)))
        return imd_set_error("%s: mask, guidance_rows and coefs must be 4-byte aligned", what);
    if (p.dtype != IMD_DTYPE_F16 && p.dtype != IMD_DTYPE_BF16) return imd_set_error("%s: unknown dtype %d", what, p.dtype);
    return 0;
}

}  // namespace

int imd_launch_unipc_step(const UnipcParams& p, hipStream_t s) {
    if (unipc_step_refusal(p, "unipc_step", false)) return 1;
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(unipc_step_kernel<true>, dim3(unipc_grid((long)p.B * p.HW)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(unipc_step_kernel<false>, dim3(unipc_grid((long)p.B * p.HW)), dim3(256), 0, s, p);
    return imd_check_launch("unipc_step");
}

int imd_launch_unipc_step_rows(const UnipcParams& p, const float* coef_rows, hipStream_t s) {
    if (!coef_rows) return imd_set_error("unipc_step_rows: null coef_rows");
    if (reinterpret_cast<uintptr_t>(coef_rows) & 15) return imd_set_error("unipc_step_rows: coef_rows must be 16-byte aligned (six float4 per latent row)");
    if (unipc_step_refusal(p, "unipc_step_rows", true)) return 1;
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(unipc_step_rows_kernel<true>, dim3(unipc_grid((long)p.B * p.HW)), dim3(256), 0, s, p, coef_rows);
    else hipLaunchKernelGGL(unipc_step_rows_kernel<false>, dim3(unipc_grid((long)p.B * p.HW)), dim3(256), 0, s, p, coef_rows);
    return imd_check_launch("unipc_step_rows");
}

int imd_launch_unipc_step_rows_at(const UnipcParams& p, const float* coef_rows, const int* row_slot, int slots, hipStream_t s) {
    if (!coef_rows) return imd_set_error("unipc_step_rows_at: null coef_rows");
    if (reinterpret_cast<uintptr_t>(coef_rows) & 15) return imd_set_error("unipc_step_rows_at: coef_rows must be 16-byte aligned (six float4 per batch row)");
    if (!row_slot) return imd_set_error("unipc_step_rows_at: null row_slot");
    if (reinterpret_cast<uintptr_t>(row_slot) & 3) return imd_set_error("unipc_step_rows_at: row_slot must be 4-byte aligned");
    if (slots < 1) return imd_set_error("unipc_step_rows_at: slots (%d) must be >= 1", slots);
    if (unipc_step_refusal(p, "unipc_step_rows_at", true)) return 1;
    if (p.B > slots) return imd_set_error("unipc_step_rows_at: B (%d batch rows) exceeds slots (%d)", p.B, slots);
    const UnipcSlotMap map = {row_slot, slots};
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL((unipc_step_rows_kernel<true, UnipcSlotMap>), dim3(unipc_grid((long)p.B * p.HW)), dim3(256), 0, s, p, coef_rows, map);
    else hipLaunchKernelGGL((unipc_step_rows_kernel<false, UnipcSlotMap>), dim3(unipc_grid((long)p.B * p.HW)), dim3(256), 0, s, p, coef_rows, map);
    return imd_check_launch("unipc_step_rows_at");
}
