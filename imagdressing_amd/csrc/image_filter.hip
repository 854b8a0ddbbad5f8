// Mask growing and feathering on the device (gfx950): Pillow's ImageFilter.MaxFilter(2k + 1) and ImageFilter.GaussianBlur on uint8
// "L" images, byte for byte (imd_image_mask_filter; the formula is in include/imagdressing_hip.h, the numpy restatement in
// imagdressing_amd/image.py: blur_reference / dilate_reference).  Integer only: the box (r, ww, fw) comes from the caller.
//
// Both filters are separable and every pass works on the uint8 result of the one before, so an axis is processed with its lines
// resident in LDS: a workgroup owns a strip of S whole lines (rows, or columns), loads it once, runs the passes of that axis between
// barriers (two uint8 buffers of IMD_IMG_MASK_LINE_MAX bytes, ping-pong) and stores it once.  A strip is read whole before it is
// written, and strips are disjoint, so every launch after the first works in place on `out`.  The window maximum commutes between the
// axes, which leaves three launches for both steps: columns (maximum), rows (maximum, three box passes), columns (three box passes).
// Inside a pass a thread owns a segment of one line: it sums its first window once (over the clamped range, with the replicated
// edge samples counted by multiplicity, so r >= n costs no more than n) and then slides it -- the cost of a pass does not grow with
// the radius beyond that first window.
// A line longer than the LDS buffer takes one launch per pass, global to global through `tmp`, one thread per pixel.
#include "common.h"
#include "imd_kernels.h"

namespace {

constexpr int CAP = IMD_IMG_MASK_LINE_MAX;
static_assert(2 * CAP <= IMD_IMG_LDS_BYTES, "two line buffers within the LDS budget of image.hip");

struct Box {
    uint32_t r, ww, fw;
};

struct Plane {
    long row, img;      // strides in bytes
};

// sum_{j = -r..r} in[c(x + j)], c = clamp to [0, n - 1]; `at(i)` reads sample i of the line
template <class At>
IMD_DEVINL uint32_t window_sum(At at, int n, long x, long r) {
    const long lo = x - r > 0 ? x - r : 0, hi = x + r < n - 1 ? x + r : n - 1;
    uint32_t s = 0;
    for (long t = lo; t <= hi; ++t) s += at((int)t);
    if (r > x) s += (uint32_t)(r - x) * at(0);
    if (x + r > n - 1) s += (uint32_t)(x + r - (n - 1)) * at(n - 1);
    return s;
}

template <class At>
IMD_DEVINL uint32_t clamped(At at, int n, long i) {
    return at((int)(i < 0 ? 0 : (i > n - 1 ? n - 1 : i)));
}

IMD_DEVINL uint32_t box_out(const Box& q, uint32_t sum, uint32_t edges) { return (q.ww * sum + q.fw * edges + (1u << 23)) >> 24; }

struct Bounds {
    int x0, y0, x1, y1;
};

// One axis of the filter with the lines in LDS.  AXIS 0: lines are rows, 1: columns.  grid = (strips, B); a strip is S lines.
// Sample i of line l of the strip lies at LDS byte l * n + i (rows) or i * S + l (columns) -- in both cases the order in which the
// strip is loaded, consecutive lanes reading consecutive bytes of a row.
template <int AXIS>
__global__ __launch_bounds__(256) void mask_filter_lds_kernel(const uint8_t* __restrict__ src, Plane ps, uint8_t* __restrict__ dst, Plane pd,
                                                              int H, int W, int S, int k, int nblur, Box q, int32_t* __restrict__ bounds) {
    __shared__ uint8_t lds[2 * CAP];
    __shared__ int bb[4];
    const int n = AXIS ? H : W, nlines = AXIS ? W : H;
    const int l0 = blockIdx.x * S, nl = min(S, nlines - l0), b = blockIdx.y;
    const int total = AXIS ? n * S : nl * n;                     // LDS bytes of the strip (<= CAP: the launcher sizes S)
    const uint8_t* in = src + (long)b * ps.img;
    for (int i = threadIdx.x; i < total; i += 256) {
        int y, x;
        if (AXIS) { y = i / S; x = i % S; if (x >= nl) continue; x += l0; }
        else { y = l0 + i / n; x = i % n; }
        lds[i] = in[(long)y * ps.row + x];
    }
    if (threadIdx.x < 4) bb[threadIdx.x] = threadIdx.x == 0 ? W : (threadIdx.x == 1 ? H : -1);
    __syncthreads();
    // a thread owns samples [i0, i1) of line l
    const int l = threadIdx.x % S, g = threadIdx.x / S, nseg = 256 / S;
    const int seg = (n + nseg - 1) / nseg;
    const int i0 = g * seg, i1 = min(n, i0 + seg);
    const bool active = l < nl && g < nseg && i0 < n;
    const int base = AXIS ? l : l * n, step = AXIS ? S : 1;
    int cur = 0;
    const int npass = (k > 0 ? 1 : 0) + nblur;
    for (int pass = 0; pass < npass; ++pass) {
        const uint8_t* a = lds + cur * CAP + base;
        uint8_t* o = lds + (cur ^ 1) * CAP + base;
        auto at = [&](int i) -> uint32_t { return a[i * step]; };
        if (active && k > 0 && pass == 0) {
            for (int i = i0; i < i1; ++i) {
                const int lo = max(0, i - min(k, n)), hi = min(n - 1, i + min(k, n));
                uint32_t m = 0;
                for (int t = lo; t <= hi; ++t) m = max(m, at(t));
                o[i * step] = (uint8_t)m;
            }
        } else if (active) {
            const long r = q.r;
            uint32_t sum = window_sum(at, n, i0, r);
            for (int i = i0; i < i1; ++i) {
                const uint32_t right = clamped(at, n, i + r + 1);
                o[i * step] = (uint8_t)box_out(q, sum, clamped(at, n, i - r - 1) + right);
                sum += right - clamped(at, n, i - r);
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    const uint8_t* res = lds + cur * CAP;
    uint8_t* out = dst + (long)b * pd.img;
    Bounds m = {W, H, -1, -1};
    for (int i = threadIdx.x; i < total; i += 256) {
        int y, x;
        if (AXIS) { y = i / S; x = i % S; if (x >= nl) continue; x += l0; }
        else { y = l0 + i / n; x = i % n; }
        const uint8_t v = res[i];
        out[(long)y * pd.row + x] = v;
        if (v) { m.x0 = min(m.x0, x); m.y0 = min(m.y0, y); m.x1 = max(m.x1, x); m.y1 = max(m.y1, y); }
    }
    if (bounds) {
        if (m.x1 >= 0) { atomicMin(&bb[0], m.x0); atomicMin(&bb[1], m.y0); atomicMax(&bb[2], m.x1); atomicMax(&bb[3], m.y1); }
        __syncthreads();
        if (threadIdx.x == 0 && bb[2] >= 0) {
            int32_t* d = bounds + 4L * b;
            atomicMin(&d[0], bb[0]); atomicMin(&d[1], bb[1]); atomicMax(&d[2], bb[2]); atomicMax(&d[3], bb[3]);
        }
    }
}

// One pass, global to global (src != dst), one thread per pixel.  OP 0: copy, 1: window maximum, 2: box pass.  AXIS as above.
template <int AXIS, int OP>
__global__ __launch_bounds__(256) void mask_filter_pass_kernel(const uint8_t* __restrict__ src, Plane ps, uint8_t* __restrict__ dst, Plane pd,
                                                               int B, int H, int W, int k, Box q, int32_t* __restrict__ bounds) {
    const long pixels = (long)H * W, total = (long)B * pixels;
    const int n = AXIS ? H : W;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const int b = (int)(i / pixels);
        const long rem = i - (long)b * pixels;
        const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
        const uint8_t* line = src + (long)b * ps.img + (AXIS ? (long)x : (long)y * ps.row);
        const long step = AXIS ? ps.row : 1;
        auto at = [&](int t) -> uint32_t { return line[(long)t * step]; };
        const int c = AXIS ? y : x;
        uint32_t v;
        if (OP == 0) {
            v = at(c);
        } else if (OP == 1) {
            const int lo = max(0, c - min(k, n)), hi = min(n - 1, c + min(k, n));
            v = 0;
            for (int t = lo; t <= hi; ++t) v = max(v, at(t));
        } else {
            const long r = q.r;
            v = box_out(q, window_sum(at, n, c, r), clamped(at, n, c - r - 1) + clamped(at, n, c + r + 1));
        }
        dst[(long)b * pd.img + (long)y * pd.row + x] = (uint8_t)v;
        if (bounds && v) {
            int32_t* d = bounds + 4L * b;
            atomicMin(&d[0], x); atomicMin(&d[1], y); atomicMax(&d[2], x); atomicMax(&d[3], y);
        }
    }
}

__global__ void mask_bounds_init_kernel(int32_t* __restrict__ bounds, int B, int H, int W) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 4 * B) bounds[i] = (i & 3) == 0 ? W : ((i & 3) == 1 ? H : -1);
}

struct Plan {
    bool global;        // one launch per pass through tmp
    int launches;
};

// every refusal of imd_image_mask_filter
int plan(const ImageMaskFilterParams& p, Plan* out) {
    if (!p.src || !p.out) return imd_set_error("image_mask_filter: null pointer (src / out)");
    if (p.B <= 0 || p.H <= 0 || p.W <= 0) return imd_set_error("image_mask_filter: empty image (B %d, %d x %d)", p.B, p.H, p.W);
    if ((long)p.H * p.W > 0x7fffffffL) return imd_set_error("image_mask_filter: an image of %d x %d exceeds 2^31 bytes", p.H, p.W);
    if (p.src_row_stride < p.W || p.out_row_stride < p.W)
        return imd_set_error("image_mask_filter: row stride (src %lld, out %lld) below the %d bytes of a row", (long long)p.src_row_stride,
                             (long long)p.out_row_stride, p.W);
    if (p.B > 1 && (p.src_img_stride < (int64_t)(p.H - 1) * p.src_row_stride + p.W || p.out_img_stride < (int64_t)(p.H - 1) * p.out_row_stride + p.W))
        return imd_set_error("image_mask_filter: image stride (src %lld, out %lld) below the bytes of an image", (long long)p.src_img_stride,
                             (long long)p.out_img_stride);
    if (p.k < 0) return imd_set_error("image_mask_filter: k (%d) must not be negative", p.k);
    if (p.blur) {
        if (p.passes != 3) return imd_set_error("image_mask_filter: passes (%d) must be 3, Pillow's GaussianBlur", p.passes);
        const uint64_t total = (2ull * p.r + 1) * p.ww + 2ull * p.fw;
        if (total != (1ull << 24) && total != (1ull << 24) - 1)
            return imd_set_error("image_mask_filter: box (r %u, ww %u, fw %u) is inconsistent: (2r + 1) ww + 2 fw = %llu, not 2^24 or 2^24 - 1",
                                 p.r, p.ww, p.fw, (unsigned long long)total);
    }
    if (p.B > 65535) return imd_set_error("image_mask_filter: %d images exceed the grid", p.B);
    const int steps = (p.k > 0 ? 1 : 0) + (p.blur ? 1 : 0);
    out->global = (p.flags & IMD_IMG_MASK_FORCE_GLOBAL) || p.H > CAP || p.W > CAP;
    if (out->global) {
        if (!p.tmp) return imd_set_error("image_mask_filter: one launch per pass (%d x %d, flags %d) needs the uint8 plane tmp", p.H, p.W, p.flags);
        if (p.tmp == p.src || p.tmp == p.out) return imd_set_error("image_mask_filter: tmp must be a plane of its own");
        out->launches = steps ? (p.k > 0 ? 2 : 0) + (p.blur ? 6 : 0) : 1;
    } else {
        out->launches = steps == 2 ? 3 : (steps == 1 ? 2 : 1);
    }
    if (p.bounds) out->launches += 1;
    return 0;
}

// lines of a strip: rows aim at segments of ~16 samples per thread, columns at 64 bytes of a row per load; both within the buffer
int strip_lines(int axis, int n) {
    const int fit = CAP / n;
    const int want = axis ? 64 : 256 / ((n + 15) / 16 < 256 ? (n + 15) / 16 : 256);
    const int s = want < fit ? want : fit;
    return s < 1 ? 1 : (s > 256 ? 256 : s);
}

void launch_lds(int axis, const uint8_t* src, Plane ps, uint8_t* dst, Plane pd, const ImageMaskFilterParams& p, int k, int nblur,
                int32_t* bounds, hipStream_t s) {
    const Box q = {p.r, p.ww, p.fw};
    const int n = axis ? p.H : p.W, nlines = axis ? p.W : p.H;
    const int S = strip_lines(axis, n);
    const dim3 grid((nlines + S - 1) / S, p.B);
    if (axis) hipLaunchKernelGGL(mask_filter_lds_kernel<1>, grid, dim3(256), 0, s, src, ps, dst, pd, p.H, p.W, S, k, nblur, q, bounds);
    else hipLaunchKernelGGL(mask_filter_lds_kernel<0>, grid, dim3(256), 0, s, src, ps, dst, pd, p.H, p.W, S, k, nblur, q, bounds);
}

template <int AXIS, int OP>
void launch_pass(const uint8_t* src, Plane ps, uint8_t* dst, Plane pd, const ImageMaskFilterParams& p, int32_t* bounds, hipStream_t s) {
    const Box q = {p.r, p.ww, p.fw};
    const long g = ((long)p.B * p.H * p.W + 255) / 256;
    hipLaunchKernelGGL((mask_filter_pass_kernel<AXIS, OP>), dim3((int)(g > 65535 ? 65535 : g)), dim3(256), 0, s, src, ps, dst, pd, p.B, p.H, p.W,
                       p.k, q, bounds);
}

}  // namespace

int imd_image_mask_filter_form_of(const ImageMaskFilterParams& p) {
    Plan pl;
    return plan(p, &pl) == 0 ? pl.launches : 0;
}

int imd_launch_image_mask_filter(const ImageMaskFilterParams& p, hipStream_t s) {
    Plan pl;
    if (plan(p, &pl)) return 1;
    const Plane ps = {(long)p.src_row_stride, (long)p.src_img_stride}, po = {(long)p.out_row_stride, (long)p.out_img_stride};
    if (p.bounds) {
        hipLaunchKernelGGL(mask_bounds_init_kernel, dim3((4 * p.B + 255) / 256), dim3(256), 0, s, p.bounds, p.B, p.H, p.W);
        if (imd_check_launch("image_mask_filter (bounds)")) return 1;
    }
    const bool mx = p.k > 0, bl = p.blur != 0;
    if (!pl.global) {
        // the last launch writes the bounds; every launch after the first works in place on out
        if (mx && bl) {
            launch_lds(1, p.src, ps, p.out, po, p, p.k, 0, nullptr, s);
            launch_lds(0, p.out, po, p.out, po, p, p.k, 3, nullptr, s);
            launch_lds(1, p.out, po, p.out, po, p, 0, 3, p.bounds, s);
        } else if (mx) {
            launch_lds(1, p.src, ps, p.out, po, p, p.k, 0, nullptr, s);
            launch_lds(0, p.out, po, p.out, po, p, p.k, 0, p.bounds, s);
        } else if (bl) {
            launch_lds(0, p.src, ps, p.out, po, p, 0, 3, nullptr, s);
            launch_lds(1, p.out, po, p.out, po, p, 0, 3, p.bounds, s);
        } else {
            launch_lds(0, p.src, ps, p.out, po, p, 0, 0, p.bounds, s);
        }
        return imd_check_launch("image_mask_filter");
    }
    // one launch per pass, alternating tmp and out: the number of passes is even (2, 6 or 8), so the last one lands in out
    const Plane pt = {(long)p.W, (long)p.H * p.W};
    if (!mx && !bl) {
        if (p.src == p.out) launch_pass<0, 0>(p.src, ps, p.tmp, pt, p, p.bounds, s);          // (nothing to move: the bounds alone)
        else launch_pass<0, 0>(p.src, ps, p.out, po, p, p.bounds, s);
        return imd_check_launch("image_mask_filter");
    }
    const int npass = (mx ? 2 : 0) + (bl ? 6 : 0);
    const uint8_t* cur = p.src;
    Plane pc = ps;
    for (int i = 0; i < npass; ++i) {
        const bool to_tmp = (i & 1) == 0;
        uint8_t* dst = to_tmp ? p.tmp : p.out;
        const Plane pd = to_tmp ? pt : po;
        int32_t* bnd = i == npass - 1 ? p.bounds : nullptr;
        const int j = mx ? i - 2 : i;                              // index among the box passes
        if (mx && i == 0) launch_pass<0, 1>(cur, pc, dst, pd, p, bnd, s);
        else if (mx && i == 1) launch_pass<1, 1>(cur, pc, dst, pd, p, bnd, s);
        else if (j < 3) launch_pass<0, 2>(cur, pc, dst, pd, p, bnd, s);
        else launch_pass<1, 2>(cur, pc, dst, pd, p, bnd, s);
        if (imd_check_launch("image_mask_filter (pass)")) return 1;
        cur = dst;
        pc = pd;
    }
    return 0;
}
