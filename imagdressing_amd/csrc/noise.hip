// noise_rows: counter-based standard-normal noise that belongs to a REQUEST (gfx950) -- imd_noise_params.  The four channels of a pixel
// are a pure function of (seed, image, draw, pixel):
//   (x0, x1, x2, x3) = Philox4x32-10(counter = (pixel, image, draw, 0), key = (seed_lo, seed_hi))        Salmon et al., SC'11
//   u_j = ((x_j >> 9) + 0.5) 2^-23                      exact in fp32, in [2^-24, 1 - 2^-24]: never 0, never 1
//   r0 = sqrt(-2 ln u0),  r1 = sqrt(-2 ln u2)           Box-Muller, two pairs per Philox call
//   out = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3, r1 sin 2 pi u3)
// |out| <= sqrt(2 ln 2^24) = 5.768: the tails beyond are cut, a mass of about 1e-8 per value.  ln, sqrt and sincospi are the accurate
// library functions (no __ intrinsics); sincospi(2 u) takes an argument that is exact in fp32, so no rounding of 2 pi u enters.
// Nothing else enters the value: not `rows`, not the row position, not the grid, not the other rows -- a session row and a solo call
// with the same key therefore hold the same bytes.
//
// Launch: grid (min(ceil(HW / 256), NOISE_MAX_BLOCKS_X), rows), 256 threads; blockIdx.y is the row, so the eight key words are uniform
// over the workgroup (scalar loads, once per thread and not per pixel) and an inactive row's workgroups leave before any access to
// `out`.  A thread owns the pixels tid, tid + stride, ...; each is ONE 16-byte vector store, consecutive lanes 16 bytes apart (1 KiB per
// wave and instruction).  Per pixel: 40 32x32 multiplies (10 rounds x 2 products x {hi, lo}; the two halves of a product are separate
// integer instructions, and Philox's full-width products leave no 24-bit shortcut), then two logs, two square roots and two sincospi.
// At 512 x 640 and 1024 x 1280 latents the launch costs what a launch costs (tools/device_noise_bench.py): neither bounds it.
#include <math.h>

#include "common.h"
#include "imd_kernels.h"

namespace {

constexpr int NOISE_THREADS = 256;
constexpr int NOISE_MAX_BLOCKS_X = 1024;                   // pixels past 256 * 1024 per row are reached by the grid-stride loop
constexpr int NOISE_MAX_ROWS = 65535;                      // gridDim.y

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(PHILOX_M0, c.x), l0 = PHILOX_M0 * c.x;
        const uint32_t h1 = __umulhi(PHILOX_M1, c.z), l1 = PHILOX_M1 * c.z;
        c = make_uint4(h1 ^ c.y ^ k0, l1, h0 ^ c.w ^ k1, l0);
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return c;
}

__device__ __forceinline__ float noise_uniform(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 0x1p-23f; }

__device__ __forceinline__ float4 noise_normal4(const uint4 x) {
    const float r0 = sqrtf(-2.f * logf(noise_uniform(x.x))), r1 = sqrtf(-2.f * logf(noise_uniform(x.z)));
    float s0, c0, s1, c1;
    sincospif(2.f * noise_uniform(x.y), &s0, &c0);
    sincospif(2.f * noise_uniform(x.w), &s1, &c1);
    return make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
}

template <int KIND>
__global__ __launch_bounds__(NOISE_THREADS) void noise_rows_kernel(const imd_noise_params p) {
    const int row = blockIdx.y;
    const uint32_t* __restrict__ key = p.key_rows + (size_t)row * IMD_NOISE_ROW_WORDS;
    if (key[4] == 0u) return;                              // (uniform over the workgroup) an inactive row: not read, not written
    const uint32_t k0 = key[0], k1 = key[1], image = key[2], draw = key[3];
    const int HW = p.HW;
    const int stride = (int)gridDim.x * NOISE_THREADS;     // <= 256 * 1024
    uint4* __restrict__ out = reinterpret_cast<uint4*>(p.out) + (size_t)row * HW;
    for (long long j = (long long)blockIdx.x * NOISE_THREADS + threadIdx.x; j < HW; j += stride) {
        const uint4 x = philox4x32_10(make_uint4((uint32_t)j, image, draw, 0u), k0, k1);
        if constexpr (KIND == IMD_NOISE_BITS) {
            out[j] = x;
        } else {
            const float4 n = noise_normal4(x);
            out[j] = make_uint4(__float_as_uint(n.x), __float_as_uint(n.y), __float_as_uint(n.z), __float_as_uint(n.w));
        }
    }
}

}  // namespace

int imd_launch_noise_rows(const imd_noise_params& p, hipStream_t s) {
    auto misaligned = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
    if (!p.out) return imd_set_error("noise_rows: null out");
    if (!p.key_rows) return imd_set_error("noise_rows: null key_rows");
    if (misaligned(p.out, 16)) return imd_set_error("noise_rows: out must be 16-byte aligned");
    if (misaligned(p.key_rows, 16)) return imd_set_error("noise_rows: key_rows must be 16-byte aligned");
    if (p.rows < 1 || p.HW < 1) return imd_set_error("noise_rows: empty output (rows = %d, HW = %d)", p.rows, p.HW);
    if (p.rows > NOISE_MAX_ROWS) return imd_set_error("noise_rows: rows (%d) must be at most %d", p.rows, NOISE_MAX_ROWS);
    if (p.kind != IMD_NOISE_NORMAL && p.kind != IMD_NOISE_BITS)
        return imd_set_error("noise_rows: unknown kind %d (IMD_NOISE_NORMAL = 0, IMD_NOISE_BITS = 1)", p.kind);
    const int bx = (p.HW - 1) / NOISE_THREADS + 1;
    const dim3 grid((unsigned)(bx < NOISE_MAX_BLOCKS_X ? bx : NOISE_MAX_BLOCKS_X), (unsigned)p.rows);
    if (p.kind == IMD_NOISE_BITS) hipLaunchKernelGGL(noise_rows_kernel<IMD_NOISE_BITS>, grid, dim3(NOISE_THREADS), 0, s, p);
    else hipLaunchKernelGGL(noise_rows_kernel<IMD_NOISE_NORMAL>, grid, dim3(NOISE_THREADS), 0, s, p);
    return imd_check_launch("noise_rows");
}
