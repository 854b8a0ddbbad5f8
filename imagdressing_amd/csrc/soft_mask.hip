// soft_mask: gray mask levels as per-pixel repaint depth (gfx950) -- imd_image_mask_release_params, imd_soft_mask_rows_params.
// Differential Diffusion (Levin & Fried, 2023): the gray level of a mask pixel decides for how many of the LAST steps of a run of n
// schedule positions the pixel is free to be repainted; before that it is reset to the re-noised original, as an unmasked pixel is.
// Every step still blends with a 0 / 1 mask, so no step kernel changes: two small launches in front of them.
//
// 1. image_mask_release_kernel, once per mask: the uint8 "L" window [H0][W0] -> uint16 release[h w].  Latent pixel (y, x) owns the bin of
//    torch's adaptive_avg_pool2d: rows [floor(y H0 / h), ceil((y + 1) H0 / h)), columns likewise.  S = the integer sum of its bytes,
//    D = 255 cnt:   release = n - ceil(S n / D) = n - (S n + D - 1) / D      in 64-bit integers, exact.
//    Mapping: ONE WAVE per latent pixel, four waves per workgroup.  The bin is numbered row-major (j = row * bw + col) and lane l reads
//    the bytes j = l, l + 64, ...: consecutive lanes on consecutive bytes of a bin row, so the 8 x 8 bin of a VAE-sized mask is one
//    byte per lane and a wide bin reads 64-byte runs.  The division j / bw is a 32-bit one per byte; the launch runs once per request
//    and no speed is claimed for it.  The lanes' 64-bit partial sums meet in an xor butterfly; lane 0 divides and stores 2 bytes.
// 2. soft_mask_rows_kernel, once per step: mask[r][p] = step_rows[r] >= release[r][p] ? 1.0f : 0.0f for every row whose step_rows
//    entry is not negative; a negative entry leaves the row unread and unwritten (a hard-mask request beside a soft one keeps its
//    mask).  Grid (pixels, rows): blockIdx.y is the row, so its step is uniform over the workgroup (one scalar load) and an inactive
//    row's workgroups leave before any access.  A thread owns FOUR pixels: one 8-byte load of four release values, one 16-byte store of
//    four floats, consecutive lanes 16 bytes apart in the output (1 KiB per wave and store instruction) -- the store is two thirds of the
//    launch's bytes.  Row r starts at element r HW, which is a multiple of 4 only when HW is (or r is kind): the first
//    (-r HW) mod 4 pixels of the row and the last (HW - head) mod 4 are written one by one by the first threads of the row's first
//    workgroup, at most six scalar stores per row; everything between is aligned for both vector widths because both buffers start on
//    16 bytes (release: 8) and share the element index.
#include "common.h"
#include "imd_kernels.h"

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_MAX_BLOCKS_X = 1024;                      // vectors past 256 * 1024 per row are reached by the grid-stride loop
constexpr int SM_MAX_ROWS = 65535;                         // gridDim.y
constexpr int MR_WAVES = SM_THREADS / 64;                  // latent pixels per workgroup

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(SM_THREADS) void image_mask_release_kernel(const imd_image_mask_release_params p) {
    const int lane = threadIdx.x & 63;
    const long long pix = (long long)blockIdx.x * MR_WAVES + (threadIdx.x >> 6);          // uniform over the wave
    if (pix >= (long long)p.h * p.w) return;
    const long long y = pix / p.w, x = pix - y * p.w;
    const long long y0 = y * p.H0 / p.h, y1 = ((y + 1) * p.H0 + p.h - 1) / p.h;
    const long long x0 = x * p.W0 / p.w, x1 = ((x + 1) * p.W0 + p.w - 1) / p.w;
    const uint32_t bw = (uint32_t)(x1 - x0), cnt = (uint32_t)(y1 - y0) * bw;              // cnt <= H0 W0 < 2^31 (checked by the launcher)
    const uint8_t* __restrict__ src = p.src + y0 * p.src_row_stride + x0;
    unsigned long long sum = 0;
    for (uint32_t j = lane; j < cnt; j += 64) {
        const uint32_t r = j / bw, c = j - r * bw;
        sum += src[(long long)r * p.src_row_stride + c];
    }
    sum = wave_sum_u64(sum);
    if (lane == 0) {
        const unsigned long long D = 255ull * cnt, n = (unsigned long long)p.n;
        p.out[pix] = (uint16_t)(n - (sum * n + D - 1) / D);                               // S <= D: the quotient is in [0, n]
    }
}

__global__ __launch_bounds__(SM_THREADS) void soft_mask_rows_kernel(const imd_soft_mask_rows_params p) {
    const int row = blockIdx.y;
    const int step = p.step_rows[row];
    if (step < 0) return;                                  // (uniform over the workgroup) a hard row: not read, not written
    const uint32_t k = (uint32_t)step;
    const int HW = p.HW;
    const size_t base = (size_t)row * HW;
    const int head = min((int)((4 - (base & 3)) & 3), HW);
    const int vecs = (HW - head) >> 2;
    const uint16_t* __restrict__ rel = p.release + base;
    float* __restrict__ m = p.mask + base;
    const uint2* __restrict__ rel4 = reinterpret_cast<const uint2*>(rel + head);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(m + head);
    const int stride = (int)gridDim.x * SM_THREADS;        // <= 256 * 1024
    for (long long v = (long long)blockIdx.x * SM_THREADS + threadIdx.x; v < vecs; v += stride) {
        const uint2 r = rel4[v];
        m4[v] = make_float4(k >= (r.x & 0xFFFFu) ? 1.f : 0.f, k >= (r.x >> 16) ? 1.f : 0.f,
                            k >= (r.y & 0xFFFFu) ? 1.f : 0.f, k >= (r.y >> 16) ? 1.f : 0.f);
    }
    if (blockIdx.x == 0) {                                 // the ragged ends of the row, at most 3 + 3 pixels
        const int t = threadIdx.x, tail0 = head + vecs * 4;
        const int i = t < head ? t : tail0 + (t - head);
        if (i < HW && (t < head || i >= tail0)) m[i] = k >= (uint32_t)rel[i] ? 1.f : 0.f;
    }
}

bool misaligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

}  // namespace

int imd_launch_image_mask_release(const imd_image_mask_release_params& p, hipStream_t s) {
    const char* n = "image_mask_release";
    if (!p.src) return imd_set_error("%s: null src", n);
    if (!p.out) return imd_set_error("%s: null out", n);
    if (p.h < 1 || p.w < 1) return imd_set_error("%s: empty latent (h = %d, w = %d)", n, p.h, p.w);
    if (p.H0 < 1 || p.W0 < 1) return imd_set_error("%s: empty mask window (H0 = %d, W0 = %d)", n, p.H0, p.W0);
    if (p.src_row_stride < p.W0) return imd_set_error("%s: src_row_stride (%lld) is below W0 (%d)", n, (long long)p.src_row_stride, p.W0);
    if (p.n < 1 || p.n > 65535) return imd_set_error("%s: n (%d) must be in [1, 65535]", n, p.n);
    if (misaligned(p.out, 2)) return imd_set_error("%s: out must be 2-byte aligned", n);
    if ((long long)p.H0 * p.W0 >= 0x80000000ll) return imd_set_error("%s: mask window too large (%d x %d: 2^31 bytes or more)", n, p.H0, p.W0);
    if ((long long)p.h * p.w >= 0x40000000ll) return imd_set_error("%s: latent too large (%d x %d: 2^30 pixels or more)", n, p.h, p.w);
    const long long pixels = (long long)p.h * p.w;
    hipLaunchKernelGGL(image_mask_release_kernel, dim3((unsigned)((pixels + MR_WAVES - 1) / MR_WAVES)), dim3(SM_THREADS), 0, s, p);
    return imd_check_launch(n);
}

int imd_launch_soft_mask_rows(const imd_soft_mask_rows_params& p, hipStream_t s) {
    const char* n = "soft_mask_rows";
    if (!p.release) return imd_set_error("%s: null release", n);
    if (!p.step_rows) return imd_set_error("%s: null step_rows", n);
    if (!p.mask) return imd_set_error("%s: null mask", n);
    if (misaligned(p.release, 8)) return imd_set_error("%s: release must be 8-byte aligned", n);
    if (misaligned(p.step_rows, 4)) return imd_set_error("%s: step_rows must be 4-byte aligned", n);
    if (misaligned(p.mask, 16)) return imd_set_error("%s: mask must be 16-byte aligned", n);
    if (p.B < 1 || p.HW < 1) return imd_set_error("%s: empty mask (B = %d, HW = %d)", n, p.B, p.HW);
    if (p.B > SM_MAX_ROWS) return imd_set_error("%s: B (%d) must be at most %d", n, p.B, SM_MAX_ROWS);
    const int bx = (p.HW / 4) / SM_THREADS + 1;            // (at least one workgroup per row: it also writes the ragged ends)
    const dim3 grid((unsigned)(bx < SM_MAX_BLOCKS_X ? bx : SM_MAX_BLOCKS_X), (unsigned)p.B);
    hipLaunchKernelGGL(soft_mask_rows_kernel, grid, dim3(SM_THREADS), 0, s, p);
    return imd_check_launch(n);
}
