// residual_scale_rows: every batch row of up to 16 tensors gets its own scale, in place, in ONE launch (gfx950) -- imd_scale_rows_params.
// The ControlNet's conditioning scale is `out_scale` of its 13 zero-conv launches: a property of a launch, not of a row.  A batch whose
// requests differ in that scale (or in the step window in which it applies) runs the zero convs with out_scale = 1 and this launch
// between the ControlNet and the UNet.  Segment k is a contiguous 16-bit [rows, row_elems[k]] tensor; for every row r and segment k
//   scale_rows[r] == 1.0f :  the row is neither read nor written (its bytes, NaN payloads included, stay)
//   otherwise             :  out = RNE16(float(x) * scale_rows[r])      widen (exact), ONE fp32 multiply, round to nearest even
// which is, bit for bit, (x.float() * torch.tensor(s, dtype=torch.float32)).to(dtype) on the CPU.  0 and negative scales are scales.
//
// Work decomposition.  The unit is a CHUNK: SR_CHUNK_VECS = 1024 consecutive 16-byte vectors (16 KiB) of ONE row of ONE segment, the
// last chunk of a row ragged.  Segment k has rows * ceil(vecs_k / 1024) chunks (vecs_k = row_elems[k] / 8); the launcher puts the running
// sum of those counts (chunk_end[k], from the 16-byte-vector counts of the block) into the kernel arguments, so chunk c belongs to the
// segment whose [chunk_end[k - 1], chunk_end[k]) holds it -- a search over at most 16 wave-uniform entries, done with scalar compares
// and selects (no dynamic indexing of the arguments).  Inside its segment chunk c - chunk_end[k - 1] is (row, offset) = divmod by the
// chunks per row.  The segments of one forward differ 50x in size (5120 x 320 down to 80 x 1280 elements per row at a 64 x 80 latent):
// numbering the chunks through all segments gives every workgroup the same 16 KiB of work, where a grid dimension per segment of equal
// extent would leave most of the grid idle.  The grid is min(chunks, SR_MAX_BLOCKS) workgroups of 256 threads which stride over the
// chunk numbers.  Per chunk the segment descriptor and the row's scale are uniform over the workgroup (blockIdx and kernel arguments
// only): scalar loads, once per chunk and not per element; a row at 1.0 costs that one scalar load and nothing else.  A thread then
// owns the vectors tid, tid + 256, tid + 512, tid + 768 of the chunk: four independent 16-byte loads in flight, consecutive lanes 16
// bytes apart (1 KiB per wave and instruction), then four 16-byte stores to the same addresses.
// No LDS, no atomics, no barrier, nothing data-dependent beyond the s == 1 skip; every thread reads a vector before it overwrites it
// and no other thread touches it.
#include "common.h"
#include "imd_kernels.h"

namespace {

constexpr int SR_THREADS = 256;
constexpr int SR_UNROLL = 4;
constexpr int SR_CHUNK_VECS = SR_THREADS * SR_UNROLL;      // 1024 16-byte vectors = 16 KiB
constexpr int SR_MAX_BLOCKS = 2048;                        // 8 workgroups per CU on 256 CUs; chunks past that by the stride loop
constexpr int SR_SEGS = IMD_SCALE_ROWS_MAX_SEGMENTS;

struct ScaleRowsArgs {                                     // by value in the kernel arguments (SGPRs); entries at or past `segments` repeat the last
    uint4* data[SR_SEGS];
    uint32_t vecs[SR_SEGS];                                // 16-byte vectors per row
    uint32_t cpr[SR_SEGS];                                 // chunks per row
    uint32_t chunk_end[SR_SEGS];                           // running sum of rows * cpr
    uint32_t chunks;                                       // == chunk_end[segments - 1]
};

template <bool F16>
__global__ __launch_bounds__(SR_THREADS) void residual_scale_rows_kernel(const ScaleRowsArgs a, const float* __restrict__ scale_rows) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
        // (segment, row, offset) of chunk c: all uniform over the workgroup
        uint32_t begin = 0, vecs = a.vecs[0], cpr = a.cpr[0];
        uint4* base = a.data[0];
#pragma unroll
        for (int j = 0; j < SR_SEGS - 1; ++j) {
            if (c >= a.chunk_end[j]) {                     // c < chunks == chunk_end[j] for every j >= segments - 1: never taken there
                begin = a.chunk_end[j];
                vecs = a.vecs[j + 1];
                cpr = a.cpr[j + 1];
                base = a.data[j + 1];
            }
        }
        const uint32_t local = c - begin;
        const uint32_t row = local / cpr, off = local - row * cpr;
        const float s = scale_rows[row];
        if (s == 1.0f) continue;                           // not read, not written
        uint4* const p = base + (size_t)row * vecs;
        const uint32_t v0 = off * SR_CHUNK_VECS + tid;
        uint4 x[SR_UNROLL];
#pragma unroll
        for (int u = 0; u < SR_UNROLL; ++u)
            if (v0 + u * SR_THREADS < vecs) x[u] = p[v0 + u * SR_THREADS];
#pragma unroll
        for (int u = 0; u < SR_UNROLL; ++u) {
            if (v0 + u * SR_THREADS < vecs) {
                float f[8];
                unpack8<F16>(x[u], f);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] *= s;
                p[v0 + u * SR_THREADS] = pack8<F16>(f);
            }
        }
    }
}

}  // namespace

int imd_launch_residual_scale_rows(const imd_scale_rows_params& p, hipStream_t s) {
    // (capi.cpp has checked the block: dtype, 1 <= segments <= 16, rows >= 1, row_elems positive multiples of 8, pointers and alignment)
    const char* n = "residual_scale_rows";
    ScaleRowsArgs a;
    unsigned long long total = 0;
    for (int k = 0; k < p.segments; ++k) {
        a.data[k] = reinterpret_cast<uint4*>(p.data[k]);
        a.vecs[k] = (uint32_t)(p.row_elems[k] / 8);
        a.cpr[k] = (a.vecs[k] + SR_CHUNK_VECS - 1) / SR_CHUNK_VECS;
        total += (unsigned long long)p.rows * a.cpr[k];
        if (total >= 0x80000000ull) return imd_set_error("%s: operand too large (2^31 chunks of 16 KiB or more)", n);
        a.chunk_end[k] = (uint32_t)total;
    }
    for (int k = p.segments; k < SR_SEGS; ++k) {
        a.data[k] = a.data[p.segments - 1];
        a.vecs[k] = a.vecs[p.segments - 1];
        a.cpr[k] = a.cpr[p.segments - 1];
        a.chunk_end[k] = (uint32_t)total;
    }
    a.chunks = (uint32_t)total;
    const dim3 grid((unsigned)(total < (unsigned long long)SR_MAX_BLOCKS ? total : SR_MAX_BLOCKS));
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL(residual_scale_rows_kernel<true>, grid, dim3(SR_THREADS), 0, s, a, p.scale_rows);
    else hipLaunchKernelGGL(residual_scale_rows_kernel<false>, grid, dim3(SR_THREADS), 0, s, a, p.scale_rows);
    return imd_check_launch(n);
}
