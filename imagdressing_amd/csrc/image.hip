// Image input / output on the device (gfx950): what the pipelines otherwise do on one host thread around the sampling loop.
//
// image_resample: Pillow's 8-bit antialiased resampler (libImaging/Resample.c: ImagingResampleHorizontal_8bpc / ...Vertical_8bpc) --
// pure integer arithmetic once the coefficient tables exist (imagdressing_amd/image.py builds them in float64 as Pillow does), so the
// result is bit-exact: per axis  out = clip8((2^21 + sum_j in[xmin + j] * k[j]) >> 22)  with an int32 accumulator, horizontal first,
// the vertical pass over the UINT8 result of the horizontal one.  The output stage (crop window, binarise, /255, affine map, layout)
// is fused into the last pass.  Both axes: one launch, a workgroup owns a TILE_W x TILE_H tile of the crop window, resamples the
// source rows its tile needs horizontally into LDS (uint8) and runs the vertical pass from there; when those rows exceed the LDS
// tile (very strong reductions: hundreds of taps), two launches with the uint8 intermediate in global memory.
// These launches are bound by their count and latency (a 768 x 1024 x 3 source is 2.4 MB), not by bandwidth: one thread per pixel,
// byte loads, no staging tricks.
//
// image_pack_u8: decoder output [B, H, W, 4 | 8] 16-bit -> uint8 RGB, rint(clamp(x / 2 + 0.5, 0, 1) * 255) in fp32, so that one
// byte per channel value crosses to the host instead of four.
//
// image_overlay: the inpainting result composited into the person image, Pillow's Image.composite per byte (one rounding):
// out = orig outside the box, ((t >> 8) + t) >> 8 with t = orig (255 - m) + gen m + 128 inside.  The one bandwidth-bound kernel of this
// file: a lane owns 16 consecutive bytes of `out` (5 1/3 pixels, at most 6 mask bytes); lanes whose bytes lie in one row and wholly
// inside or wholly outside the box columns move them as one 16-byte access each (orig, gen -- at whatever byte offset the box gives
// it -- and out), every other lane (row ends, box edges, the tail of the batch) goes byte by byte.
//
// image_inpaint_condition: make_inpaint_condition of the inpainting script on uint8 inputs -> the ControlNet's 16-bit NHWC8 image.
#include "common.h"
#include "imd_kernels.h"

// the output stage promises separately rounded operations (the host path it reproduces has no fused multiply-add)
#pragma clang fp contract(off)

namespace {

constexpr int TW = IMD_IMG_TILE_W, TH = IMD_IMG_TILE_H, PRECISION_BITS = 22;
static_assert(TW * TH == 256, "one thread per output pixel of a tile");

struct AxisTable {
    const int32_t* xmin;
    const int32_t* count;
    const int32_t* k;
    int kmax, n_in;
};

struct OutStage {
    void* out;
    int kind, dtype, binarize, C;
    int out_h, out_w;      // the crop window
    float a[3], b[3];
};

IMD_DEVINL int clip8(int acc) {
    const int v = acc >> PRECISION_BITS;          // arithmetic shift, as Pillow's clip8
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// entry i of a table, clamped so that no tap leaves [0, n_in) whatever the table holds (a valid table is never changed by this)
IMD_DEVINL void taps_of(const AxisTable& t, int i, int& x0, int& n) {
    n = min(max(t.count[i], 0), min(t.kmax, t.n_in));
    x0 = min(max(t.xmin[i], 0), t.n_in - n);
}

template <bool F16>
IMD_DEVINL void emit(const OutStage& o, int b, int y, int x, const int* v) {
    const long pix = ((long)b * o.out_h + y) * o.out_w + x;
    int u[3];
    float f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        u[c] = c < o.C ? v[c] : 0;
        if (o.binarize) u[c] = __fdiv_rn((float)u[c], 255.0f) >= 0.5f ? 255 : 0;
        float m = __fdiv_rn((float)u[c], 255.0f) * o.a[c];
        asm volatile("" : "+v"(m));                    // the product is rounded on its own: nothing may fuse it into the add
        f[c] = m + o.b[c];
    }
    if (o.kind == IMD_IMG_U8) {
        uint8_t* out = reinterpret_cast<uint8_t*>(o.out) + pix * o.C;
        for (int c = 0; c < o.C; ++c) out[c] = (uint8_t)u[c];
    } else if (o.kind == IMD_IMG_F32_NCHW) {
        float* out = reinterpret_cast<float*>(o.out);
        const long plane = (long)o.out_h * o.out_w;
        for (int c = 0; c < o.C; ++c) out[((long)b * o.C + c) * plane + (long)y * o.out_w + x] = f[c];
    } else {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        w.x = El<F16>::pack2(f[0], o.C > 1 ? f[1] : 0.f);
        if (o.C > 2) w.y = El<F16>::pack2(f[2], 0.f);
        reinterpret_cast<uint4*>(o.out)[pix] = w;
    }
}

// One pass over the window [off_y, off_y + out_h) x [off_x, off_x + out_w) of this pass's output: AXIS 0 resamples along x, 1 along y,
// 2 copies (both axes skipped: the output stage alone).  One thread per pixel.
template <int AXIS, bool F16>
__global__ __launch_bounds__(256) void resample_pass_kernel(const uint8_t* __restrict__ src, long src_row, long src_img, AxisTable t,
                                                            int B, int off_y, int off_x, OutStage o) {
    const long total = (long)B * o.out_h * o.out_w;
    const int C = o.C;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const int x = (int)(i % o.out_w), y = (int)((i / o.out_w) % o.out_h), b = (int)(i / ((long)o.out_w * o.out_h));
        const uint8_t* img = src + (long)b * src_img;
        int acc[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
        int v[3] = {0, 0, 0};
        if (AXIS == 0) {
            int x0, n;
            taps_of(t, x + off_x, x0, n);
            const uint8_t* row = img + (long)(y + off_y) * src_row + (long)x0 * C;
            const int32_t* k = t.k + (long)(x + off_x) * t.kmax;
            for (int j = 0; j < n; ++j) {
                const int kj = k[j];
                for (int c = 0; c < C; ++c) acc[c] += (int)row[j * C + c] * kj;
            }
            for (int c = 0; c < C; ++c) v[c] = clip8(acc[c]);
        } else if (AXIS == 1) {
            int y0, n;
            taps_of(t, y + off_y, y0, n);
            const uint8_t* col = img + (long)y0 * src_row + (long)(x + off_x) * C;
            const int32_t* k = t.k + (long)(y + off_y) * t.kmax;
            for (int j = 0; j < n; ++j) {
                const int kj = k[j];
                for (int c = 0; c < C; ++c) acc[c] += (int)col[(long)j * src_row + c] * kj;
            }
            for (int c = 0; c < C; ++c) v[c] = clip8(acc[c]);
        } else {
            const uint8_t* px = img + (long)(y + off_y) * src_row + (long)(x + off_x) * C;
            for (int c = 0; c < C; ++c) v[c] = px[c];
        }
        emit<F16>(o, b, y, x, v);
    }
}

// Both axes in one launch.  grid = (tiles in x, tiles in y, B) over the crop window; LDS: [rows the tile needs][TW][C] uint8.
template <int C, bool F16>
__global__ __launch_bounds__(256) void resample_fused_kernel(const uint8_t* __restrict__ src, long src_row, long src_img, AxisTable th,
                                                             AxisTable tv, int top, int left, OutStage o) {
    __shared__ uint8_t lds[IMD_IMG_LDS_BYTES];
    constexpr int CAP = IMD_IMG_LDS_BYTES / (TW * C);          // rows of h the tile can hold
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, b = blockIdx.z;
    const int ny = min(TH, o.out_h - ty0), nx = min(TW, o.out_w - tx0);
    // source rows [r0, r1) that the tile's output rows read
    int r0 = tv.n_in, r1 = 0;
    for (int y = 0; y < ny; ++y) {
        int y0, n;
        taps_of(tv, top + ty0 + y, y0, n);
        r0 = min(r0, y0);
        r1 = max(r1, y0 + n);
    }
    const int nrows = min(max(r1 - r0, 0), CAP);               // (the host launches this form only when r1 - r0 <= CAP)
    const uint8_t* img = src + (long)b * src_img;
    for (int i = threadIdx.x; i < nrows * TW; i += 256) {
        const int r = i / TW, x = i % TW;
        if (x >= nx) continue;
        int x0, n;
        taps_of(th, left + tx0 + x, x0, n);
        const uint8_t* row = img + (long)(r0 + r) * src_row + (long)x0 * C;
        const int32_t* k = th.k + (long)(left + tx0 + x) * th.kmax;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
        for (int j = 0; j < n; ++j) {
            const int kj = k[j];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)row[j * C + c] * kj;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) lds[(r * TW + x) * C + c] = (uint8_t)clip8(acc[c]);
    }
    __syncthreads();
    const int y = threadIdx.x / TW, x = threadIdx.x % TW;
    if (y >= ny || x >= nx) return;
    int y0, n;
    taps_of(tv, top + ty0 + y, y0, n);
    const int l0 = min(max(y0 - r0, 0), nrows);
    n = min(n, nrows - l0);
    const int32_t* k = tv.k + (long)(top + ty0 + y) * tv.kmax;
    int v[3] = {0, 0, 0};
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < n; ++j) {
        const int kj = k[j];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += (int)lds[((l0 + j) * TW + x) * C + c] * kj;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = clip8(acc[c]);
    emit<F16>(o, b, ty0 + y, tx0 + x, v);
}

template <bool F16>
__global__ __launch_bounds__(256) void pack_u8_kernel(const bf16_t* __restrict__ src, uint8_t* __restrict__ out, long pixels, int ld) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < pixels; i += (long)gridDim.x * 256L) {
        const uint2 w = *reinterpret_cast<const uint2*>(src + i * ld);        // channels 0..3 (3 is padding)
        const float x[3] = {El<F16>::lo(w.x), El<F16>::hi(w.x), El<F16>::lo(w.y)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = x[c] * 0.5f + 0.5f;                                     // x / 2 is exact: fused or not, one rounding
            t = fminf(fmaxf(t, 0.f), 1.f);
            out[i * 3 + c] = (uint8_t)(int)rintf(t * 255.0f);
        }
    }
}

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

struct OverlayGeom {
    int B, Bo, H0, W0, x1, y1, cw, ch;
};

IMD_DEVINL uint32_t composite8(uint32_t o, uint32_t g, uint32_t m) {
    const uint32_t t = o * (255u - m) + g * m + 128u;
    return ((t >> 8) + t) >> 8;
}

// 16 bytes at any byte address (the compiler picks the widest access the target allows for an alignment of 1)
IMD_DEVINL u32x4_t load16(const uint8_t* p) {
    u32x4_t v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

IMD_DEVINL void store16(uint8_t* p, u32x4_t v) { __builtin_memcpy(p, &v, 16); }

__global__ __launch_bounds__(256) void overlay_kernel(const uint8_t* __restrict__ orig, const uint8_t* __restrict__ mask,
                                                      const uint8_t* __restrict__ gen, uint8_t* __restrict__ out, OverlayGeom q) {
    const int rowb = q.W0 * 3;                                   // bytes of a row
    const long img = (long)q.H0 * rowb, total = (long)q.B * img; // bytes of an image (< 2^31: the launcher checks) and of the batch
    const long pixels = (long)q.H0 * q.W0, grow = (long)q.cw * 3;
    const int bx0 = q.x1 * 3, bx1 = (q.x1 + q.cw) * 3;           // the box's byte columns
    for (long i = blockIdx.x * 256L + threadIdx.x; i * 16 < total; i += (long)gridDim.x * 256L) {
        const long g0 = i * 16;
        const int b = (int)(g0 / img), r0 = (int)(g0 - (long)b * img);
        const int y = r0 / rowb, xb = r0 - y * rowb;
        const bool whole = g0 + 16 <= total && xb + 16 <= rowb;  // 16 bytes of one row of one image
        const bool row_in = y >= q.y1 && y < q.y1 + q.ch;
        const uint8_t* src = orig + (q.Bo == 1 ? (long)r0 : g0);
        if (whole && (!row_in || xb + 16 <= bx0 || xb >= bx1)) {
            store16(out + g0, load16(src));
        } else if (whole && xb >= bx0 && xb + 16 <= bx1) {
            const u32x4_t o = load16(src);
            const u32x4_t g = load16(gen + ((long)b * q.ch + (y - q.y1)) * grow + (xb - bx0));
            const int px = xb / 3, c0 = xb - px * 3, npx = (xb + 15) / 3 - px + 1;          // 6 pixels (5 or 6 when c0 == 0)
            const uint8_t* mrow = mask + (q.Bo == 1 ? 0L : b * pixels) + (long)y * q.W0 + px;
            uint64_t mm = 0;
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (j < npx) mm |= (uint64_t)mrow[j] << (8 * j);
            u32x4_t w;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t sh = 8 * (k & 3);
                const uint32_t m = (uint32_t)(mm >> (8 * ((c0 + k) / 3))) & 255u;
                const uint32_t v = composite8((o[k >> 2] >> sh) & 255u, (g[k >> 2] >> sh) & 255u, m);
                w[k >> 2] = (k & 3) ? (w[k >> 2] | (v << sh)) : v;
            }
            store16(out + g0, w);
        } else {
            for (int k = 0; k < 16 && g0 + k < total; ++k) {
                const long gk = g0 + k;
                const int bb = (int)(gk / img), r = (int)(gk - (long)bb * img);
                const int yy = r / rowb, xx = r - yy * rowb;
                uint32_t v = orig[q.Bo == 1 ? (long)r : gk];
                if (yy >= q.y1 && yy < q.y1 + q.ch && xx >= bx0 && xx < bx1) {
                    const uint32_t m = mask[(q.Bo == 1 ? 0L : bb * pixels) + (long)yy * q.W0 + xx / 3];
                    v = composite8(v, gen[((long)bb * q.ch + (yy - q.y1)) * grow + (xx - bx0)], m);
                }
                out[gk] = (uint8_t)v;
            }
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(256) void inpaint_condition_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ mask,
                                                                uint4* __restrict__ out, long pixels) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < pixels; i += (long)gridDim.x * 256L) {
        const bool masked = __fdiv_rn((float)mask[i], 255.0f) > 0.5f;
        float f[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = masked ? -1.0f : __fdiv_rn((float)image[i * 3 + c], 255.0f);
        out[i] = make_uint4(El<F16>::pack2(f[0], f[1]), El<F16>::pack2(f[2], 0.f), 0u, 0u);
    }
}

int grid_1d(long n) {
    const long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

bool axis_given(const int32_t* xmin, const int32_t* count, const int32_t* k) { return xmin && count && k; }
bool axis_absent(const int32_t* xmin, const int32_t* count, const int32_t* k) { return !xmin && !count && !k; }

// every refusal of imd_image_resample; *form: launches the call makes (1 | 2)
int plan(const ImageResampleParams& p, int* form) {
    if (!p.src || !p.out) return imd_set_error("image_resample: null pointer (src / out)");
    if (p.C != 1 && p.C != 3) return imd_set_error("image_resample: C (%d) must be 1 or 3", p.C);
    if (p.B <= 0 || p.Hin <= 0 || p.Win <= 0 || p.Hres <= 0 || p.Wres <= 0)
        return imd_set_error("image_resample: empty image (B %d, %d x %d -> %d x %d)", p.B, p.Hin, p.Win, p.Hres, p.Wres);
    if (p.src_row_stride < (int64_t)p.Win * p.C || p.src_img_stride < 0)
        return imd_set_error("image_resample: row stride %lld below the %d bytes of a row", (long long)p.src_row_stride, p.Win * p.C);
    const bool h = axis_given(p.h_xmin, p.h_count, p.h_k), v = axis_given(p.v_xmin, p.v_count, p.v_k);
    if (!h && !axis_absent(p.h_xmin, p.h_count, p.h_k)) return imd_set_error("image_resample: incomplete horizontal table (xmin, count and k go together)");
    if (!v && !axis_absent(p.v_xmin, p.v_count, p.v_k)) return imd_set_error("image_resample: incomplete vertical table (xmin, count and k go together)");
    if (!h && p.Wres != p.Win) return imd_set_error("image_resample: horizontal axis skipped but the width changes (%d -> %d)", p.Win, p.Wres);
    if (!v && p.Hres != p.Hin) return imd_set_error("image_resample: vertical axis skipped but the height changes (%d -> %d)", p.Hin, p.Hres);
    if (h && (p.h_kmax <= 0 || p.h_taps <= 0 || p.h_taps > p.h_kmax))
        return imd_set_error("image_resample: horizontal count (%d) exceeds kmax (%d)", p.h_taps, p.h_kmax);
    if (v && (p.v_kmax <= 0 || p.v_taps <= 0 || p.v_taps > p.v_kmax))
        return imd_set_error("image_resample: vertical count (%d) exceeds kmax (%d)", p.v_taps, p.v_kmax);
    if (p.top < 0 || p.left < 0 || p.crop_h <= 0 || p.crop_w <= 0 || p.top > p.Hres - p.crop_h || p.left > p.Wres - p.crop_w)
        return imd_set_error("image_resample: crop (top %d, left %d, %d x %d) outside the resized image (%d x %d)", p.top, p.left, p.crop_h,
                             p.crop_w, p.Hres, p.Wres);
    if (p.kind != IMD_IMG_U8 && p.kind != IMD_IMG_F32_NCHW && p.kind != IMD_IMG_16_NHWC8)
        return imd_set_error("image_resample: unknown output kind %d", p.kind);
    if (p.kind == IMD_IMG_16_NHWC8 && p.dtype != IMD_DTYPE_F16 && p.dtype != IMD_DTYPE_BF16)
        return imd_set_error("image_resample: unknown dtype %d", p.dtype);
    if (p.kind == IMD_IMG_16_NHWC8 && ((uintptr_t)p.out & 15)) return imd_set_error("image_resample: a 16-bit NHWC8 output must be 16-byte aligned");
    if (p.kind == IMD_IMG_F32_NCHW && ((uintptr_t)p.out & 3)) return imd_set_error("image_resample: an fp32 output must be 4-byte aligned");
    *form = 1;
    if (h && v) {
        const bool fits = p.v_tile_rows > 0 && (long)p.v_tile_rows * TW * p.C <= IMD_IMG_LDS_BYTES;
        if ((p.flags & IMD_IMG_FORCE_TWO_PASS) || !fits) {
            *form = 2;
            if (!p.tmp) return imd_set_error("image_resample: two launches (v_tile_rows %d) need the uint8 intermediate tmp", p.v_tile_rows);
        }
    }
    return 0;
}

OutStage out_stage(const ImageResampleParams& p) {
    OutStage o;
    o.out = p.out; o.kind = p.kind; o.dtype = p.dtype; o.binarize = p.binarize; o.C = p.C;
    o.out_h = p.crop_h; o.out_w = p.crop_w;
    for (int c = 0; c < 3; ++c) { o.a[c] = p.a[c]; o.b[c] = p.b[c]; }
    return o;
}

template <int AXIS>
void launch_pass(const uint8_t* src, long src_row, long src_img, const AxisTable& t, int B, int off_y, int off_x, const OutStage& o, hipStream_t s) {
    const int grid = grid_1d((long)B * o.out_h * o.out_w);
    if (o.kind == IMD_IMG_16_NHWC8 && o.dtype == IMD_DTYPE_F16)
        hipLaunchKernelGGL((resample_pass_kernel<AXIS, true>), dim3(grid), dim3(256), 0, s, src, src_row, src_img, t, B, off_y, off_x, o);
    else
        hipLaunchKernelGGL((resample_pass_kernel<AXIS, false>), dim3(grid), dim3(256), 0, s, src, src_row, src_img, t, B, off_y, off_x, o);
}

template <int C>
void launch_fused(const ImageResampleParams& p, const AxisTable& th, const AxisTable& tv, const OutStage& o, hipStream_t s) {
    const dim3 grid((p.crop_w + TW - 1) / TW, (p.crop_h + TH - 1) / TH, p.B);
    if (o.kind == IMD_IMG_16_NHWC8 && o.dtype == IMD_DTYPE_F16)
        hipLaunchKernelGGL((resample_fused_kernel<C, true>), grid, dim3(256), 0, s, p.src, (long)p.src_row_stride, (long)p.src_img_stride, th, tv, p.top, p.left, o);
    else
        hipLaunchKernelGGL((resample_fused_kernel<C, false>), grid, dim3(256), 0, s, p.src, (long)p.src_row_stride, (long)p.src_img_stride, th, tv, p.top, p.left, o);
}

}  // namespace

int imd_image_resample_form_of(const ImageResampleParams& p) {
    int form = 0;
    return plan(p, &form) == 0 ? form : 0;
}

int imd_launch_image_resample(const ImageResampleParams& p, hipStream_t s) {
    int form = 0;
    if (plan(p, &form)) return 1;
    if ((p.crop_h + TH - 1) / TH > 65535 || p.B > 65535) return imd_set_error("image_resample: %d images of %d rows exceed the grid", p.B, p.crop_h);
    const bool h = p.h_xmin != nullptr, v = p.v_xmin != nullptr;
    const AxisTable th = {p.h_xmin, p.h_count, p.h_k, p.h_kmax, p.Win}, tv = {p.v_xmin, p.v_count, p.v_k, p.v_kmax, p.Hin};
    const OutStage o = out_stage(p);
    const long row = (long)p.src_row_stride, img = (long)p.src_img_stride;
    if (h && v && form == 1) {
        if (p.C == 3) launch_fused<3>(p, th, tv, o, s);
        else launch_fused<1>(p, th, tv, o, s);
    } else if (h && v) {
        // horizontal pass of every source row over the crop's columns -> tmp [B, Hin, crop_w, C]; then the vertical pass with the output stage
        OutStage mid = o;
        mid.out = p.tmp; mid.kind = IMD_IMG_U8; mid.binarize = 0; mid.out_h = p.Hin; mid.out_w = p.crop_w;
        launch_pass<0>(p.src, row, img, th, p.B, 0, p.left, mid, s);
        if (imd_check_launch("image_resample (horizontal pass)")) return 1;
        const long trow = (long)p.crop_w * p.C;
        launch_pass<1>(p.tmp, trow, trow * p.Hin, tv, p.B, p.top, 0, o, s);
    } else if (h) {
        launch_pass<0>(p.src, row, img, th, p.B, p.top, p.left, o, s);
    } else if (v) {
        launch_pass<1>(p.src, row, img, tv, p.B, p.top, p.left, o, s);
    } else {
        launch_pass<2>(p.src, row, img, th, p.B, p.top, p.left, o, s);
    }
    return imd_check_launch("image_resample");
}

int imd_launch_image_pack_u8(const ImagePackParams& p, hipStream_t s) {
    if (!p.src || !p.out) return imd_set_error("image_pack_u8: null pointer (src / out)");
    if (p.B <= 0 || p.H <= 0 || p.W <= 0) return imd_set_error("image_pack_u8: empty image (B %d, %d x %d)", p.B, p.H, p.W);
    if (p.ld != 4 && p.ld != 8) return imd_set_error("image_pack_u8: ld (%d) must be 4 or 8", p.ld);
    if ((uintptr_t)p.src & 7) return imd_set_error("image_pack_u8: src must be 8-byte aligned");
    const long pixels = (long)p.B * p.H * p.W;
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(pack_u8_kernel<true>, dim3(grid_1d(pixels)), dim3(256), 0, s, p.src, p.out, pixels, p.ld);
    else if (p.dtype == IMD_DTYPE_BF16) hipLaunchKernelGGL(pack_u8_kernel<false>, dim3(grid_1d(pixels)), dim3(256), 0, s, p.src, p.out, pixels, p.ld);
    else return imd_set_error("image_pack_u8: unknown dtype %d", p.dtype);
    return imd_check_launch("image_pack_u8");
}

int imd_launch_image_overlay(const ImageOverlayParams& p, hipStream_t s) {
    if (!p.orig || !p.mask || !p.gen || !p.out) return imd_set_error("image_overlay: null pointer (orig / mask / gen / out)");
    if (p.B <= 0 || p.H0 <= 0 || p.W0 <= 0) return imd_set_error("image_overlay: empty image (B %d, %d x %d)", p.B, p.H0, p.W0);
    if (p.Bo != 1 && p.Bo != p.B) return imd_set_error("image_overlay: Bo (%d) must be 1 (shared) or B (%d)", p.Bo, p.B);
    if (p.cw < 1 || p.ch < 1) return imd_set_error("image_overlay: empty box (%d x %d)", p.ch, p.cw);
    if (p.x1 < 0 || p.y1 < 0 || p.cw > p.W0 || p.ch > p.H0 || p.x1 > p.W0 - p.cw || p.y1 > p.H0 - p.ch)
        return imd_set_error("image_overlay: box (x1 %d, y1 %d, %d x %d) outside the image (%d x %d)", p.x1, p.y1, p.ch, p.cw, p.H0, p.W0);
    if ((long)p.H0 * p.W0 * 3 > 0x7fffffffL) return imd_set_error("image_overlay: an image of %d x %d exceeds 2^31 bytes", p.H0, p.W0);
    const OverlayGeom q = {p.B, p.Bo, p.H0, p.W0, p.x1, p.y1, p.cw, p.ch};
    const long lanes = ((long)p.B * p.H0 * p.W0 * 3 + 15) / 16;
    hipLaunchKernelGGL(overlay_kernel, dim3(grid_1d(lanes)), dim3(256), 0, s, p.orig, p.mask, p.gen, p.out, q);
    return imd_check_launch("image_overlay");
}

int imd_launch_image_inpaint_condition(const ImageInpaintConditionParams& p, hipStream_t s) {
    if (!p.image || !p.mask || !p.out) return imd_set_error("image_inpaint_condition: null pointer (image / mask / out)");
    if (p.B <= 0 || p.H <= 0 || p.W <= 0) return imd_set_error("image_inpaint_condition: empty image (B %d, %d x %d)", p.B, p.H, p.W);
    if ((uintptr_t)p.out & 15) return imd_set_error("image_inpaint_condition: the NHWC8 output must be 16-byte aligned");
    const long pixels = (long)p.B * p.H * p.W;
    uint4* out = reinterpret_cast<uint4*>(p.out);
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(inpaint_condition_kernel<true>, dim3(grid_1d(pixels)), dim3(256), 0, s, p.image, p.mask, out, pixels);
    else if (p.dtype == IMD_DTYPE_BF16) hipLaunchKernelGGL(inpaint_condition_kernel<false>, dim3(grid_1d(pixels)), dim3(256), 0, s, p.image, p.mask, out, pixels);
    else return imd_set_error("image_inpaint_condition: unknown dtype %d", p.dtype);
    return imd_check_launch("image_inpaint_condition");
}
