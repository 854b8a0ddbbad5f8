// HBM-bound elementwise kernels of the sampling loop (gfx950).
//
// ddim_cfg_step fuses, over the [B, HW, 4] latent:
//   classifier-free guidance      eps = eps_u + g (eps_c - eps_u)
//       (/root/reference/dressing_sd/pipelines/IMAGDressing_v1_pipeline.py:521-527)
//   the DDIM update (eta = 0)     x0 = (z - sqrt(1-a_t) eps) / sqrt(a_t);  z' = sqrt(a_prev) x0 + sqrt(1-a_prev) eps
//       (diffusers==0.24.0 DDIMScheduler.step, call site :530-532)
//   the inpainting blend          z' = (1-m) add_noise(z_img, noise, t_next) + m z'
//       (..._pipeline_controlnet_inpainting.py:487-500)
//   and the next step's UNet input: bf16, channels padded 4 -> 8, duplicated for the cond and
//   uncond halves (torch.cat([latents]*2), :483-488; scale_model_input is the identity for DDIM).
// Algorithmic traffic per latent element: 3 fp32 reads + 1 fp32 write (+3 reads with inpaint)
// + 2 x 4 B of bf16 next-input writes.
// Per-row guidance (imd_ddim_cfg_step_rows): the instantiation with ONE trailing `const float*` argument reads the guidance
// scale of each latent row from that device [B] fp32 array instead of p.guidance -- one batched call serving requests with
// different guidance scales.  The scalar instantiation (empty pack) keeps the one-argument signature, hence the same
// kernarg layout and instruction stream as before the variant existed.
#include "common.h"
#include "imd_kernels.h"

namespace {

template <bool F16, typename... RowGuidance>
__global__ __launch_bounds__(256) void ddim_cfg_step_kernel(const DdimParams p, const RowGuidance*... guidance_rows) {
    static_assert(sizeof...(RowGuidance) <= 1, "scalar step (no array) or one per-row guidance array");
    const long total = (long)p.B * p.HW;                   // one thread per pixel (4 channels = 16 B)
    float sa_t = p.sqrt_a_t, s1_t = p.sqrt_1m_a_t, sa_p = p.sqrt_a_prev, s1_p = p.sqrt_1m_a_prev, sa_n = p.sqrt_a_next, s1_n = p.sqrt_1m_a_next;
    if (p.coefs) {                                         // schedule coefficients from device memory (HIP-graph replay of a step)
        sa_t = p.coefs[0]; s1_t = p.coefs[1]; sa_p = p.coefs[2]; s1_p = p.coefs[3]; sa_n = p.coefs[4]; s1_n = p.coefs[5];
    }
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const float4 z = reinterpret_cast<const float4*>(p.z)[i];
        const float4 ec = reinterpret_cast<const float4*>(p.eps)[i];
        const float4 eu = reinterpret_cast<const float4*>(p.eps)[i + total];
        float zz[4] = {z.x, z.y, z.z, z.w};
        float g = p.guidance;
        if constexpr (sizeof...(RowGuidance) == 1) g = (guidance_rows[i / p.HW], ...);     // the latent row of this pixel
        const float c[4] = {ec.x, ec.y, ec.z, ec.w};
        const float u[4] = {eu.x, eu.y, eu.z, eu.w};
        float mk = 1.f;
        float zi[4] = {0, 0, 0, 0}, nz[4] = {0, 0, 0, 0}, vn[4] = {0, 0, 0, 0};
        if (p.var_noise) {                                 // stochastic DDIM (eta > 0): sigma * noise, added before the blend
            const float4 n = reinterpret_cast<const float4*>(p.var_noise)[i];
            vn[0] = p.sigma * n.x; vn[1] = p.sigma * n.y; vn[2] = p.sigma * n.z; vn[3] = p.sigma * n.w;
        }
        if (p.mask) {
            mk = p.mask[i];
            const float4 a = reinterpret_cast<const float4*>(p.z_img)[i];
            const float4 n = reinterpret_cast<const float4*>(p.noise)[i];
            zi[0] = a.x; zi[1] = a.y; zi[2] = a.z; zi[3] = a.w;
            nz[0] = n.x; nz[1] = n.y; nz[2] = n.z; nz[3] = n.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float eps = u[e] + g * (c[e] - u[e]);
            const float x0 = (zz[e] - s1_t * eps) / sa_t;
            float zn = sa_p * x0 + s1_p * eps + vn[e];
            if (p.mask) {
                const float proper = sa_n * zi[e] + s1_n * nz[e];
                zn = (1.f - mk) * proper + mk * zn;
            }
            zz[e] = zn;
        }
        reinterpret_cast<float4*>(p.z)[i] = make_float4(zz[0], zz[1], zz[2], zz[3]);
        if (p.x_next) {
            const uint4 o = make_uint4(El<F16>::pack2(zz[0], zz[1]), El<F16>::pack2(zz[2], zz[3]), 0u, 0u);
            reinterpret_cast<uint4*>(p.x_next)[i] = o;
            reinterpret_cast<uint4*>(p.x_next)[i + total] = o;
        }
    }
}

// the next UNet input of one pixel: 16-bit(in_scale z), channels padded 4 -> 8 (one expression for the step kernels and the session's
// input launch, so that the two agree bit for bit)
template <bool F16>
__device__ __forceinline__ uint4 session_input_pack(float in_scale, const float (&zz)[4]) {
    return make_uint4(El<F16>::pack2(in_scale * zz[0], in_scale * zz[1]), El<F16>::pack2(in_scale * zz[2], in_scale * zz[3]), 0u, 0u);
}

// sampler_step: the same fused launch for every sampler whose update is affine in the latent, the guided epsilon, a short history
// and noise (DPM-Solver++ 1 / 2M, Euler, Euler-ancestral, PNDM/PLMS -- imd_sampler_params):
//   m  = m_x z + m_e eps;   z' = z_x z + z_m m + sum_k z_h[k] H[k] + z_n noise;   blend;   H[store] = m;   x_next = 16-bit(in_scale z')
// The coefficients come from the parameter block or from 13 floats of device memory (a captured step replays with other
// coefficients AND another history slot written, nothing in the graph changes).  History slot k is the float4 array
// p.hist + k * B * HW; a slot with coefficient 0 is not read (the start-up steps of a multistep sampler cost no extra traffic), and
// the slot being overwritten is read by the same thread first.
// Algorithmic traffic per latent element: 3 fp32 reads + 1 fp32 write + 2 x 4 B of next-input writes, + 1 read per history term,
// + 1 write with a store, + 1 read with noise, + 3 reads with the blend.
template <bool F16>
__global__ __launch_bounds__(256) void sampler_step_kernel(const SamplerParams p) {
    const long total = (long)p.B * p.HW;                   // one thread per pixel (4 channels = 16 B)
    float m_x = p.m_x, m_e = p.m_e, z_x = p.z_x, z_m = p.z_m, z_n = p.z_n, b_img = p.b_img, b_noise = p.b_noise, in_scale = p.in_scale;
    float zh[4] = {p.z_h[0], p.z_h[1], p.z_h[2], p.z_h[3]};
    int store = p.store;
    if (p.coefs) {
        m_x = p.coefs[0]; m_e = p.coefs[1]; z_x = p.coefs[2]; z_m = p.coefs[3];
        zh[0] = p.coefs[4]; zh[1] = p.coefs[5]; zh[2] = p.coefs[6]; zh[3] = p.coefs[7];
        z_n = p.coefs[8]; b_img = p.coefs[9]; b_noise = p.coefs[10]; in_scale = p.coefs[11];
        store = (int)p.coefs[12];
    }
    if (store >= p.K) store = -1;                          // (device coefficients are not seen by the launcher: never past the buffer)
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const float4 z = reinterpret_cast<const float4*>(p.z)[i];
        const float4 ec = reinterpret_cast<const float4*>(p.eps)[i];
        const float4 eu = reinterpret_cast<const float4*>(p.eps)[i + total];
        float zz[4] = {z.x, z.y, z.z, z.w};
        const float g = p.guidance_rows ? p.guidance_rows[i / p.HW] : p.guidance;     // the latent row of this pixel
        const float c[4] = {ec.x, ec.y, ec.z, ec.w};
        const float u[4] = {eu.x, eu.y, eu.z, eu.w};
        float hs[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < p.K && zh[k] != 0.f) h = reinterpret_cast<const float4*>(p.hist)[(long)k * total + i];
            hs[k][0] = h.x; hs[k][1] = h.y; hs[k][2] = h.z; hs[k][3] = h.w;
        }
        float mk = 1.f;
        float zi[4] = {0, 0, 0, 0}, nz[4] = {0, 0, 0, 0}, vn[4] = {0, 0, 0, 0};
        if (p.noise) {
            const float4 n = reinterpret_cast<const float4*>(p.noise)[i];
            vn[0] = z_n * n.x; vn[1] = z_n * n.y; vn[2] = z_n * n.z; vn[3] = z_n * n.w;
        }
        if (p.mask) {
            mk = p.mask[i];
            const float4 a = reinterpret_cast<const float4*>(p.z_img)[i];
            const float4 n = reinterpret_cast<const float4*>(p.blend_noise)[i];
            zi[0] = a.x; zi[1] = a.y; zi[2] = a.z; zi[3] = a.w;
            nz[0] = n.x; nz[1] = n.y; nz[2] = n.z; nz[3] = n.w;
        }
        float mm[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float eps = u[e] + g * (c[e] - u[e]);
            mm[e] = m_x * zz[e] + m_e * eps;
            float zn = z_x * zz[e] + z_m * mm[e];
#pragma unroll
            for (int k = 0; k < 4; ++k) zn += zh[k] * hs[k][e];
            zn += vn[e];
            if (p.mask) {
                const float proper = b_img * zi[e] + b_noise * nz[e];
                zn = (1.f - mk) * proper + mk * zn;
            }
            zz[e] = zn;
        }
        reinterpret_cast<float4*>(p.z)[i] = make_float4(zz[0], zz[1], zz[2], zz[3]);
        if (store >= 0) reinterpret_cast<float4*>(p.hist)[(long)store * total + i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
        if (p.x_next) {
            const uint4 o = session_input_pack<F16>(in_scale, zz);
            reinterpret_cast<uint4*>(p.x_next)[i] = o;
            reinterpret_cast<uint4*>(p.x_next)[i + total] = o;
        }
    }
}

// sampler_step_rows: sampler_step with the coefficient block PER LATENT ROW (a denoising session: every row is a request at its own
// position of its own schedule).  Row b reads 16 floats of device memory, coef_rows + 16 b, as four float4: [0..12] the block above,
// [13] active.  An inactive row is skipped whole -- no load and no store of z, eps, the history or x_next -- so a free slot keeps its
// bytes.  The per-pixel arithmetic is sampler_step_kernel's, statement for statement (same expression trees, same contraction): with
// every row equal and active the two launches are bit-identical.  The row of a pixel is i / HW, so a block that spans several rows
// (HW < 256) reads several blocks; at the real geometries (HW >= 64) the four loads are wave-uniform and hit one cache line.
//
// sampler_step_rows_at (a COMPACTING session, whose forward runs p.B <= slots batch rows) is the same kernel with ONE trailing SlotMap
// argument -- the instantiation with the empty pack keeps the two-argument signature, hence the kernarg layout and instruction stream it
// had before the variant existed (the ddim_cfg_step_kernel idiom).  Two address spaces are then apart: `i` / `total` index what the
// forward produced and consumes (eps, x_next, the coefficient block, the guidance scale: batch ROWS), `si` / `stotal` what belongs to
// the request (z, the history with plane k at hist + k slots HW, noise, the blend operands: SLOTS).  Row r is the request living in
// slot row_slot[r]; a row whose slot is outside [0, slots) is idle and skipped like an inactive one BEFORE anything is addressed
// through it, so whatever the device map holds the kernel stays inside its buffers; slots no row names keep their bytes.  (Two rows
// naming one slot would race: the session's plan gives every running slot exactly one row.)  The map load is one dword per pixel,
// wave-uniform at HW >= 64 like the coefficients.
struct SlotMap {
    const int* row_slot;                                   // DEVICE [B]: the slot of every batch row
    int slots;
};

template <bool F16, typename... Map>
__global__ __launch_bounds__(256) void sampler_step_rows_kernel(const SamplerParams p, const float* __restrict__ coef_rows, const Map... map) {
    static_assert(sizeof...(Map) <= 1, "row == slot (no map) or one SlotMap");
    const long total = (long)p.B * p.HW;                   // one thread per pixel (4 channels = 16 B)
    long stotal = total;
    if constexpr (sizeof...(Map) == 1) stotal = (((long)map.slots * p.HW), ...);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long b = i / p.HW;                           // the latent row of this pixel
        long si = i;                                       // ... and the pixel in its slot
        if constexpr (sizeof...(Map) == 1) {
            const int slot = (map.row_slot[b], ...);
            if (slot < 0 || slot >= (map.slots, ...)) continue;          // idle row
            si = (long)slot * p.HW + (i - b * p.HW);
        }
        const float4* row = reinterpret_cast<const float4*>(coef_rows) + b * (IMD_SAMPLER_ROW_FLOATS / 4);
        const float4 r3 = row[3];
        if (r3.y == 0.f) continue;                         // inactive: neither read nor written
        const float4 r0 = row[0], r1 = row[1], r2 = row[2];
        const float m_x = r0.x, m_e = r0.y, z_x = r0.z, z_m = r0.w;
        const float zh[4] = {r1.x, r1.y, r1.z, r1.w};
        const float z_n = r2.x, b_img = r2.y, b_noise = r2.z, in_scale = r2.w;
        int store = (int)r3.x;
        if (store >= p.K) store = -1;                      // (device coefficients are not seen by the launcher: never past the buffer)
        const float4 z = reinterpret_cast<const float4*>(p.z)[si];
        const float4 ec = reinterpret_cast<const float4*>(p.eps)[i];
        const float4 eu = reinterpret_cast<const float4*>(p.eps)[i + total];
        float zz[4] = {z.x, z.y, z.z, z.w};
        const float g = p.guidance_rows ? p.guidance_rows[b] : p.guidance;
        const float c[4] = {ec.x, ec.y, ec.z, ec.w};
        const float u[4] = {eu.x, eu.y, eu.z, eu.w};
        float hs[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < p.K && zh[k] != 0.f) h = reinterpret_cast<const float4*>(p.hist)[(long)k * stotal + si];
            hs[k][0] = h.x; hs[k][1] = h.y; hs[k][2] = h.z; hs[k][3] = h.w;
        }
        float mk = 1.f;
        float zi[4] = {0, 0, 0, 0}, nz[4] = {0, 0, 0, 0}, vn[4] = {0, 0, 0, 0};
        if (p.noise) {
            const float4 n = reinterpret_cast<const float4*>(p.noise)[si];
            vn[0] = z_n * n.x; vn[1] = z_n * n.y; vn[2] = z_n * n.z; vn[3] = z_n * n.w;
        }
        if (p.mask) {
            mk = p.mask[si];
            const float4 a = reinterpret_cast<const float4*>(p.z_img)[si];
            const float4 n = reinterpret_cast<const float4*>(p.blend_noise)[si];
            zi[0] = a.x; zi[1] = a.y; zi[2] = a.z; zi[3] = a.w;
            nz[0] = n.x; nz[1] = n.y; nz[2] = n.z; nz[3] = n.w;
        }
        float mm[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float eps = u[e] + g * (c[e] - u[e]);
            mm[e] = m_x * zz[e] + m_e * eps;
            float zn = z_x * zz[e] + z_m * mm[e];
#pragma unroll
            for (int k = 0; k < 4; ++k) zn += zh[k] * hs[k][e];
            zn += vn[e];
            if (p.mask) {
                const float proper = b_img * zi[e] + b_noise * nz[e];
                zn = (1.f - mk) * proper + mk * zn;
            }
            zz[e] = zn;
        }
        reinterpret_cast<float4*>(p.z)[si] = make_float4(zz[0], zz[1], zz[2], zz[3]);
        if (store >= 0) reinterpret_cast<float4*>(p.hist)[(long)store * stotal + si] = make_float4(mm[0], mm[1], mm[2], mm[3]);
        if (p.x_next) {
            const uint4 o = session_input_pack<F16>(in_scale, zz);
            reinterpret_cast<uint4*>(p.x_next)[i] = o;
            reinterpret_cast<uint4*>(p.x_next)[i + total] = o;
        }
    }
}

// session_input_rows: x_in[r] = x_in[B + r] = 16-bit(in_scale[r] z[row_slot[r]]), channels 4..7 zero -- the UNet input of a request
// written from its fp32 latent with the step's own pack expression (admission, and the re-layout of every row at a repack: it reads
// z and writes x_in, never what it wrote).  Rows with a slot outside [0, slots) are skipped.
template <bool F16>
__global__ __launch_bounds__(256) void session_input_rows_kernel(const float* __restrict__ z, const int* __restrict__ row_slot,
                                                                 const float* __restrict__ in_scale_rows, bf16_t* __restrict__ x_in,
                                                                 int B, int slots, int HW) {
    const long total = (long)B * HW;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long r = i / HW;
        const int slot = row_slot[r];
        if (slot < 0 || slot >= slots) continue;
        const float4 v = reinterpret_cast<const float4*>(z)[(long)slot * HW + (i - r * HW)];
        const float zz[4] = {v.x, v.y, v.z, v.w};
        const uint4 o = session_input_pack<F16>(in_scale_rows[r], zz);
        reinterpret_cast<uint4*>(x_in)[i] = o;
        reinterpret_cast<uint4*>(x_in)[i + total] = o;
    }
}

// diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin]
__global__ void timestep_embedding_kernel(const float* t, float* out, int B, int dim) {
    const int half = dim / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * half) return;
    const int b = i / half, j = i - b * half;
    const float freq = expf(-9.210340371976184f * (float)j / (float)half);   // ln(10000)
    const float arg = t[b] * freq;
    out[(size_t)b * dim + j] = cosf(arg);
    out[(size_t)b * dim + half + j] = sinf(arg);
}

// out[r, c] = a[r, c] + b_scale * b[r, c]   (strided rows; 8 channels per thread)
template <bool F16>
__global__ __launch_bounds__(256) void add_kernel(const bf16_t* a, int a_ld, const bf16_t* b, int b_ld, bf16_t* out, int out_ld,
                                                   long rows, int C, float b_scale) {
    const int vpr = C / 8;
    const long total = rows * vpr;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long r = i / vpr;
        const int c = (int)(i - r * vpr) * 8;
        float fa[8], fb[8];
        unpack8<F16>(*reinterpret_cast<const uint4*>(a + r * a_ld + c), fa);
        unpack8<F16>(*reinterpret_cast<const uint4*>(b + r * b_ld + c), fb);
#pragma unroll
        for (int e = 0; e < 8; ++e) fa[e] += b_scale * fb[e];
        *reinterpret_cast<uint4*>(out + r * out_ld + c) = pack8<F16>(fa);
    }
}

__global__ __launch_bounds__(256) void copy2d_kernel(const bf16_t* a, int a_ld, bf16_t* out, int out_ld, long rows, int C) {
    const int vpr = C / 8;
    const long total = rows * vpr;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long r = i / vpr;
        const int c = (int)(i - r * vpr) * 8;
        *reinterpret_cast<uint4*>(out + r * out_ld + c) = *reinterpret_cast<const uint4*>(a + r * a_ld + c);
    }
}

// out[r, 0:Ca] = a[r], out[r, Ca:Ca+Cb] = b[r] (+ b_add[r]): the skip concat of an up block (+ the ControlNet residual) in ONE launch
template <bool F16>
__global__ __launch_bounds__(256) void concat2_kernel(const bf16_t* a, int Ca, const bf16_t* b, int Cb, const bf16_t* b_add, bf16_t* out, long rows, long b_rows) {
    const int va = Ca / 8, vpr = (Ca + Cb) / 8;
    const long total = rows * vpr;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long r = i / vpr;
        const int v = (int)(i - r * vpr);
        uint4 val;
        if (v < va) val = *reinterpret_cast<const uint4*>(a + r * Ca + v * 8);
        else {
            const long off = r * Cb + (v - va) * 8;
            val = *reinterpret_cast<const uint4*>(b + (r % b_rows) * Cb + (v - va) * 8);     // (b_rows < rows: b repeats, e.g. one copy for both CFG halves)
            if (b_add) {
                float x[8], y[8];
                unpack8<F16>(val, x);
                unpack8<F16>(*reinterpret_cast<const uint4*>(b_add + off), y);
                val = make_uint4(El<F16>::pack2(x[0] + y[0], x[1] + y[1]), El<F16>::pack2(x[2] + y[2], x[3] + y[3]),
                                 El<F16>::pack2(x[4] + y[4], x[5] + y[5]), El<F16>::pack2(x[6] + y[6], x[7] + y[7]));
            }
        }
        *reinterpret_cast<uint4*>(out + r * (long)(Ca + Cb) + v * 8) = val;
    }
}

// out[r] = table[ids[r]] + pos[r % T]      (8 channels per thread; ids outside [0, vocab) read row 0)
template <bool F16>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const bf16_t* table, int vocab, const bf16_t* pos, int T, const int64_t* ids,
                                                           bf16_t* out, long rows, int C) {
    const int vpr = C / 8;
    const long total = rows * vpr;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long r = i / vpr;
        const int c = (int)(i - r * vpr) * 8;
        long id = ids[r];
        if (id < 0 || id >= vocab) id = 0;
        float a[8], b[8];
        unpack8<F16>(*reinterpret_cast<const uint4*>(table + id * C + c), a);
        unpack8<F16>(*reinterpret_cast<const uint4*>(pos + (r % T) * C + c), b);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += b[e];
        *reinterpret_cast<uint4*>(out + r * C + c) = pack8<F16>(a);
    }
}

// out[b][0] = cls + pos[0]; out[b][1 + p] = patches[b][p] + pos[1 + p]
template <bool F16>
__global__ __launch_bounds__(256) void vit_assemble_kernel(const bf16_t* patches, const bf16_t* cls, const bf16_t* pos, bf16_t* out, int B, int P, int C) {
    const int vpr = C / 8;
    const long total = (long)B * (P + 1) * vpr;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long r = i / vpr;
        const int c = (int)(i - r * vpr) * 8;
        const int b = (int)(r / (P + 1)), t = (int)(r - (long)b * (P + 1));
        float a[8], q[8];
        unpack8<F16>(t == 0 ? *reinterpret_cast<const uint4*>(cls + c) : *reinterpret_cast<const uint4*>(patches + ((long)b * P + t - 1) * C + c), a);
        unpack8<F16>(*reinterpret_cast<const uint4*>(pos + (long)t * C + c), q);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += q[e];
        *reinterpret_cast<uint4*>(out + r * C + c) = pack8<F16>(a);
    }
}

struct LincombArgs { const float* x[8]; float c[8]; int n; };
__global__ __launch_bounds__(256) void lincomb_kernel(const LincombArgs a, float* out, long n4, long numel) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256L) {
        const long e = i * 4;
        if (e + 4 <= numel) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < a.n) {
                    const float4 v = *reinterpret_cast<const float4*>(a.x[j] + e);
                    acc.x = fmaf(a.c[j], v.x, acc.x); acc.y = fmaf(a.c[j], v.y, acc.y); acc.z = fmaf(a.c[j], v.z, acc.z); acc.w = fmaf(a.c[j], v.w, acc.w);
                }
            *reinterpret_cast<float4*>(out + e) = acc;
        } else {
            for (long k = e; k < numel; ++k) {
                float acc = 0.f;
                for (int j = 0; j < a.n; ++j) acc = fmaf(a.c[j], a.x[j][k], acc);
                out[k] = acc;
            }
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(256) void f32_to_16_kernel(const float* a, bf16_t* out, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) out[i] = El<F16>::fromf(a[i]);
}

inline unsigned grid_for(long work_items) {
    long blocks = (work_items + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

}  // namespace

namespace {
// guidance_rows: none (the scalar step) or one device [B] fp32 array
template <typename... RowGuidance>
int launch_ddim_cfg_step(const DdimParams& p, hipStream_t s, const char* what, const RowGuidance*... guidance_rows) {
    if (p.B <= 0 || p.HW <= 0) return imd_set_error("%s: empty latent", what);
    if (p.mask && (!p.z_img || !p.noise)) return imd_set_error("%s: inpaint mask given without image latents / noise", what);
    if (p.var_noise && p.coefs) return imd_set_error("%s: the stochastic step (var_noise) takes host coefficients, not the device table", what);
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL((ddim_cfg_step_kernel<true, RowGuidance...>), dim3(grid_for((long)p.B * p.HW)), dim3(256), 0, s, p, guidance_rows...);
    else if (p.dtype == IMD_DTYPE_BF16) hipLaunchKernelGGL((ddim_cfg_step_kernel<false, RowGuidance...>), dim3(grid_for((long)p.B * p.HW)), dim3(256), 0, s, p, guidance_rows...);
    else return imd_set_error("%s: unknown dtype %d", what, p.dtype);
    return imd_check_launch(what);
}
}  // namespace

int imd_launch_ddim_cfg_step(const DdimParams& p, hipStream_t s) { return launch_ddim_cfg_step(p, s, "ddim_cfg_step"); }

int imd_launch_ddim_cfg_step_rows(const DdimParams& p, const float* guidance, hipStream_t s) {
    if (!guidance) return imd_set_error("ddim_cfg_step_rows: null guidance array");
    return launch_ddim_cfg_step(p, s, "ddim_cfg_step_rows", guidance);
}

namespace {
// what imd_sampler_step and imd_sampler_step_rows refuse alike (`rows`: the coefficients, store slot included, live in device memory)
int sampler_step_refusal(const SamplerParams& p, const char* what, bool rows) {
    auto misaligned = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
    if (p.B <= 0 || p.HW <= 0) return imd_set_error("%s: empty latent", what);
    if (p.K < 0 || p.K > IMD_SAMPLER_MAX_HISTORY) return imd_set_error("%s: K (%d) must be 0..%d history slots", what, p.K, IMD_SAMPLER_MAX_HISTORY);
    if (p.K > 0 && !p.hist) return imd_set_error("%s: K = %d history slots without a history buffer", what, p.K);
    if (!rows && !p.coefs && (p.store < -1 || p.store >= p.K)) return imd_set_error("%s: store slot %d outside -1..%d", what, p.store, p.K - 1);
    if (p.mask && (!p.z_img || !p.blend_noise)) return imd_set_error("%s: inpaint mask given without image latents / blend noise", what);
    if (misaligned(p.z, 16) || misaligned(p.eps, 16) || misaligned(p.x_next, 16) || misaligned(p.hist, 16) || misaligned(p.noise, 16) ||
        misaligned(p.z_img, 16) || misaligned(p.blend_noise, 16))
        return imd_set_error("%s: z, eps, x_next, hist, noise, z_img and blend_noise must be 16-byte aligned", what);
    if (misaligned(p.mask, 4) || misaligned(p.guidance_rows, 4) || (!rows && misaligned(p.coefs, 4)))
        return imd_set_error("%s: mask, guidance_rows and coefs must be 4-byte aligned", what);
    if (p.dtype != IMD_DTYPE_F16 && p.dtype != IMD_DTYPE_BF16) return imd_set_error("%s: unknown dtype %d", what, p.dtype);
    return 0;
}
}  // namespace

int imd_launch_sampler_step(const SamplerParams& p, hipStream_t s) {
    if (sampler_step_refusal(p, "sampler_step", false)) return 1;
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(sampler_step_kernel<true>, dim3(grid_for((long)p.B * p.HW)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(sampler_step_kernel<false>, dim3(grid_for((long)p.B * p.HW)), dim3(256), 0, s, p);
    return imd_check_launch("sampler_step");
}

int imd_launch_sampler_step_rows(const SamplerParams& p, const float* coef_rows, hipStream_t s) {
    if (!coef_rows) return imd_set_error("sampler_step_rows: null coef_rows");
    if (reinterpret_cast<uintptr_t>(coef_rows) & 15) return imd_set_error("sampler_step_rows: coef_rows must be 16-byte aligned (four float4 per latent row)");
    if (sampler_step_refusal(p, "sampler_step_rows", true)) return 1;
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(sampler_step_rows_kernel<true>, dim3(grid_for((long)p.B * p.HW)), dim3(256), 0, s, p, coef_rows);
    else hipLaunchKernelGGL(sampler_step_rows_kernel<false>, dim3(grid_for((long)p.B * p.HW)), dim3(256), 0, s, p, coef_rows);
    return imd_check_launch("sampler_step_rows");
}

int imd_launch_sampler_step_rows_at(const SamplerParams& p, const float* coef_rows, const int* row_slot, int slots, hipStream_t s) {
    if (!coef_rows) return imd_set_error("sampler_step_rows_at: null coef_rows");
    if (reinterpret_cast<uintptr_t>(coef_rows) & 15) return imd_set_error("sampler_step_rows_at: coef_rows must be 16-byte aligned (four float4 per batch row)");
    if (!row_slot) return imd_set_error("sampler_step_rows_at: null row_slot");
    if (reinterpret_cast<uintptr_t>(row_slot) & 3) return imd_set_error("sampler_step_rows_at: row_slot must be 4-byte aligned");
    if (slots < 1) return imd_set_error("sampler_step_rows_at: slots (%d) must be >= 1", slots);
    if (sampler_step_refusal(p, "sampler_step_rows_at", true)) return 1;
    if (p.B > slots) return imd_set_error("sampler_step_rows_at: B (%d batch rows) exceeds slots (%d)", p.B, slots);
    const SlotMap map = {row_slot, slots};
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL((sampler_step_rows_kernel<true, SlotMap>), dim3(grid_for((long)p.B * p.HW)), dim3(256), 0, s, p, coef_rows, map);
    else hipLaunchKernelGGL((sampler_step_rows_kernel<false, SlotMap>), dim3(grid_for((long)p.B * p.HW)), dim3(256), 0, s, p, coef_rows, map);
    return imd_check_launch("sampler_step_rows_at");
}

int imd_launch_session_input_rows(const float* z, const int* row_slot, const float* in_scale_rows, bf16_t* x_in, int B, int slots, int HW,
                                  int dtype, hipStream_t s) {
    if (!z || !row_slot || !in_scale_rows || !x_in) return imd_set_error("session_input_rows: null pointer");
    if (B <= 0 || HW <= 0) return imd_set_error("session_input_rows: empty input");
    if (slots < 1) return imd_set_error("session_input_rows: slots (%d) must be >= 1", slots);
    if (B > slots) return imd_set_error("session_input_rows: B (%d batch rows) exceeds slots (%d)", B, slots);
    if ((reinterpret_cast<uintptr_t>(z) & 15) || (reinterpret_cast<uintptr_t>(x_in) & 15))
        return imd_set_error("session_input_rows: z and x_in must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(row_slot) & 3) || (reinterpret_cast<uintptr_t>(in_scale_rows) & 3))
        return imd_set_error("session_input_rows: row_slot and in_scale_rows must be 4-byte aligned");
    if (dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(session_input_rows_kernel<true>, dim3(grid_for((long)B * HW)), dim3(256), 0, s, z, row_slot, in_scale_rows, x_in, B, slots, HW);
    else if (dtype == IMD_DTYPE_BF16) hipLaunchKernelGGL(session_input_rows_kernel<false>, dim3(grid_for((long)B * HW)), dim3(256), 0, s, z, row_slot, in_scale_rows, x_in, B, slots, HW);
    else return imd_set_error("session_input_rows: unknown dtype %d", dtype);
    return imd_check_launch("session_input_rows");
}

int imd_launch_timestep_embedding(const float* t, float* out, int B, int dim, hipStream_t s) {
    if (B <= 0 || dim <= 0 || (dim & 1)) return imd_set_error("timestep_embedding: bad shape B=%d dim=%d", B, dim);
    const int n = B * dim / 2;
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t, out, B, dim);
    return imd_check_launch("timestep_embedding");
}

int imd_launch_add(const bf16_t* a, int a_ld, const bf16_t* b, int b_ld, bf16_t* out, int out_ld, long rows, int C, float b_scale, int dtype, hipStream_t s) {
    if (rows <= 0 || C <= 0) return imd_set_error("add: empty tensor");
    if (C % 8 || a_ld % 8 || b_ld % 8 || out_ld % 8) return imd_set_error("add: C and row strides must be multiples of 8");
    if (dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(add_kernel<true>, dim3(grid_for(rows * (C / 8))), dim3(256), 0, s, a, a_ld, b, b_ld, out, out_ld, rows, C, b_scale);
    else if (dtype == IMD_DTYPE_BF16) hipLaunchKernelGGL(add_kernel<false>, dim3(grid_for(rows * (C / 8))), dim3(256), 0, s, a, a_ld, b, b_ld, out, out_ld, rows, C, b_scale);
    else return imd_set_error("add: unknown dtype %d", dtype);
    return imd_check_launch("add");
}

int imd_launch_embed_tokens(const bf16_t* table, int vocab, const bf16_t* pos, int T, const int64_t* ids, bf16_t* out, long rows, int C, int dtype, hipStream_t s) {
    if (rows <= 0 || C <= 0 || vocab <= 0 || T <= 0) return imd_set_error("embed_tokens: empty problem");
    if (C % 8) return imd_set_error("embed_tokens: C (%d) must be a multiple of 8", C);
    if (dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(embed_tokens_kernel<true>, dim3(grid_for(rows * (C / 8))), dim3(256), 0, s, table, vocab, pos, T, ids, out, rows, C);
    else if (dtype == IMD_DTYPE_BF16) hipLaunchKernelGGL(embed_tokens_kernel<false>, dim3(grid_for(rows * (C / 8))), dim3(256), 0, s, table, vocab, pos, T, ids, out, rows, C);
    else return imd_set_error("embed_tokens: unknown dtype %d", dtype);
    return imd_check_launch("embed_tokens");
}

int imd_launch_vit_assemble(const bf16_t* patches, const bf16_t* cls, const bf16_t* pos, bf16_t* out, int B, int P, int C, int dtype, hipStream_t s) {
    if (B <= 0 || P <= 0 || C <= 0) return imd_set_error("vit_assemble: empty problem");
    if (C % 8) return imd_set_error("vit_assemble: C (%d) must be a multiple of 8", C);
    const long work = (long)B * (P + 1) * (C / 8);
    if (dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(vit_assemble_kernel<true>, dim3(grid_for(work)), dim3(256), 0, s, patches, cls, pos, out, B, P, C);
    else if (dtype == IMD_DTYPE_BF16) hipLaunchKernelGGL(vit_assemble_kernel<false>, dim3(grid_for(work)), dim3(256), 0, s, patches, cls, pos, out, B, P, C);
    else return imd_set_error("vit_assemble: unknown dtype %d", dtype);
    return imd_check_launch("vit_assemble");
}

int imd_launch_lincomb(const float* const* xs, const float* coefs, int n, float* out, long numel, hipStream_t s) {
    if (n < 1 || n > 8) return imd_set_error("lincomb: 1..8 inputs (got %d)", n);
    if (numel <= 0) return imd_set_error("lincomb: empty tensor");
    LincombArgs a;
    for (int j = 0; j < 8; ++j) { a.x[j] = j < n ? xs[j] : nullptr; a.c[j] = j < n ? coefs[j] : 0.f; }
    a.n = n;
    for (int j = 0; j < n; ++j)
        if (a.x[j] == nullptr || (reinterpret_cast<uintptr_t>(a.x[j]) & 15)) return imd_set_error("lincomb: input %d is null or not 16-byte aligned", j);
    if (reinterpret_cast<uintptr_t>(out) & 15) return imd_set_error("lincomb: output is not 16-byte aligned");
    const long n4 = (numel + 3) / 4;
    hipLaunchKernelGGL(lincomb_kernel, dim3(grid_for(n4)), dim3(256), 0, s, a, out, n4, numel);
    return imd_check_launch("lincomb");
}

int imd_launch_copy2d(const bf16_t* a, int a_ld, bf16_t* out, int out_ld, long rows, int C, hipStream_t s) {
    if (rows <= 0 || C <= 0) return imd_set_error("copy2d: empty tensor");
    if (C % 8 || a_ld % 8 || out_ld % 8) return imd_set_error("copy2d: C and row strides must be multiples of 8");
    hipLaunchKernelGGL(copy2d_kernel, dim3(grid_for(rows * (C / 8))), dim3(256), 0, s, a, a_ld, out, out_ld, rows, C);
    return imd_check_launch("copy2d");
}

int imd_launch_concat2(const bf16_t* a, int Ca, const bf16_t* b, int Cb, const bf16_t* b_add, bf16_t* out, long rows, long b_rows, int dtype, hipStream_t s) {
    if (rows <= 0 || Ca <= 0 || Cb <= 0) return imd_set_error("concat2: empty tensor");
    if (b_rows <= 0) b_rows = rows;
    if (rows % b_rows) return imd_set_error("concat2: b_rows (%ld) must divide rows (%ld)", b_rows, rows);
    if (Ca % 8 || Cb % 8) return imd_set_error("concat2: channel counts must be multiples of 8 (got %d + %d)", Ca, Cb);
    const long work = rows * ((Ca + Cb) / 8);
    if (dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(concat2_kernel<true>, dim3(grid_for(work)), dim3(256), 0, s, a, Ca, b, Cb, b_add, out, rows, b_rows);
    else if (dtype == IMD_DTYPE_BF16) hipLaunchKernelGGL(concat2_kernel<false>, dim3(grid_for(work)), dim3(256), 0, s, a, Ca, b, Cb, b_add, out, rows, b_rows);
    else return imd_set_error("concat2: unknown dtype %d", dtype);
    return imd_check_launch("concat2");
}

int imd_launch_f32_to_16(const float* a, bf16_t* out, long n, int dtype, hipStream_t s) {
    if (n <= 0) return imd_set_error("f32_to_16: empty tensor");
    if (dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(f32_to_16_kernel<true>, dim3(grid_for(n)), dim3(256), 0, s, a, out, n);
    else if (dtype == IMD_DTYPE_BF16) hipLaunchKernelGGL(f32_to_16_kernel<false>, dim3(grid_for(n)), dim3(256), 0, s, a, out, n);
    else return imd_set_error("f32_to_16: unknown dtype %d", dtype);
    return imd_check_launch("f32_to_16");
}
