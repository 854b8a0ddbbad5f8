// residual_mix_rows: the scaled sum of up to 4 sources on up to 16 tensors, every batch row with its own scale per source, in ONE launch
// (gfx950) -- imd_mix_rows_params.  Several ControlNets run with out_scale = 1, one after another; this launch then mixes their residuals
// for the UNet.  Segment j of source k is a contiguous 16-bit [rows, row_elems[j]] tensor; for every segment j and row r
//   acc = nothing
//   for k = 0 .. sources - 1:  s = scales[k * rows + r];  s == 0.0f: the row of source k is NOT read;  otherwise
//       term = float(x_k) * s  (widen, ONE fp32 multiply);  acc = term or acc + term  (ONE fp32 add -- no fused multiply-add)
//   dst = RNE16(acc), +0 where every source was skipped
// which is, bit for bit, the chain of x.float() * torch.tensor(s, dtype=torch.float32) and + on the CPU.  The whole kernel is compiled with
// floating-point contraction off: a v_fma / v_mac here would round the product and the sum once instead of twice.
//
// Work decomposition: that of residual_scale_rows.hip, for its reason (the segments of one forward differ 50x in size).  The unit is a
// CHUNK of MR_CHUNK_VECS = 1024 consecutive 16-byte vectors (16 KiB) of ONE row of ONE segment, the last chunk of a row ragged, numbered
// through all segments; the launcher puts the running sums of the chunk counts into the kernel arguments and the segment of chunk c is
// found with 15 scalar compares over them (the number of sums that c has reached).  The slot's entries -- K source bases, the destination
// base, the vector and chunk counts -- are then scalar loads from the kernel-argument segment at that index: the argument block is
// read where it lies, nothing is copied to scratch (ScratchSize 0) and the SGPRs hold one slot, not sixteen.  The grid is
// min(chunks, MR_MAX_BLOCKS) workgroups of 256 threads striding over the chunk numbers.  Per chunk the segment, the row and the K scales
// of the row depend on blockIdx and kernel arguments only: scalar loads, and `s == 0` is a uniform branch around the four loads of that
// source.  A thread owns the vectors tid, tid + 256, tid + 512, tid + 768 of the chunk in every contributing source.  Its loads are
// unconditional inside that branch -- a vector past the ragged end of the row reads the row's last vector instead and drops it -- so
// that 4 x (contributing sources) independent 16-byte loads are in flight before the arithmetic and the four guarded 16-byte stores; a
// branch around every load would make the compiler wait for each before the next.  The chunk ends with vmcnt(0): with the stores out,
// the compiler has no register of a pending store to protect and issues the next chunk's loads without a wait between the sources.
// dst[j] may be src[k][j]: every thread has read all its vectors of the chunk before it stores the first, no other thread stores to
// them, and the only vector a thread reads that is not its own is the dropped one.  No LDS, no atomics, no barrier.
#include "common.h"
#include "imd_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_UNROLL = 4;
constexpr int MR_CHUNK_VECS = MR_THREADS * MR_UNROLL;      // 1024 16-byte vectors = 16 KiB
constexpr int MR_MAX_BLOCKS = 2048;                        // 8 workgroups per CU on 256 CUs; chunks past that by the stride loop
constexpr int MR_SEGS = IMD_MIX_ROWS_MAX_SEGMENTS;
constexpr int MR_SRCS = IMD_MIX_ROWS_MAX_SOURCES;

template <int K>
struct MixRowsArgs {                                       // by value in the kernel arguments; entries at or past `segments` repeat the last
    const uint4* src[K][MR_SEGS];
    uint4* dst[MR_SEGS];
    uint32_t vecs[MR_SEGS];                                // 16-byte vectors per row
    uint32_t cpr[MR_SEGS];                                 // chunks per row
    uint32_t chunk_end[MR_SEGS];                           // running sum of rows * cpr
    uint32_t chunks;                                       // == chunk_end[segments - 1]
    uint32_t rows;
};

template <bool F16, int K>
__global__ __launch_bounds__(MR_THREADS) void residual_mix_rows_kernel(const MixRowsArgs<K> a, const float* __restrict__ scales) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
        // (segment, row, offset) of chunk c: all uniform over the workgroup
        uint32_t j = 0;
#pragma unroll
        for (int i = 0; i < MR_SEGS - 1; ++i) j += c >= a.chunk_end[i] ? 1u : 0u;      // c < chunks == chunk_end[i] for every i >= segments - 1
        const uint32_t begin = j ? a.chunk_end[j - 1] : 0u, vecs = a.vecs[j], cpr = a.cpr[j];
        uint4* const out = a.dst[j];
        const uint4* in[K];
#pragma unroll
        for (int k = 0; k < K; ++k) in[k] = a.src[k][j];
        const uint32_t local = c - begin;
        const uint32_t row = local / cpr, off = local - row * cpr;
        const size_t row_base = (size_t)row * vecs;
        const uint32_t v0 = off * MR_CHUNK_VECS + tid;
        float s[K];
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = scales[(size_t)k * a.rows + row];
        uint4 x[K][MR_UNROLL];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (s[k] != 0.0f) {                            // uniform: a gated source costs its scalar load and nothing else
#pragma unroll
                for (int u = 0; u < MR_UNROLL; ++u) {          // past the row's end: the row's last vector, read and dropped
                    const uint32_t v = v0 + u * MR_THREADS;
                    x[k][u] = in[k][row_base + (v < vecs ? v : vecs - 1)];
                }
            }
        }
        float acc[MR_UNROLL][8];
        bool have = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (s[k] != 0.0f) {
#pragma unroll
                for (int u = 0; u < MR_UNROLL; ++u) {
                    if (v0 + u * MR_THREADS < vecs) {
                        float f[8];
                        unpack8<F16>(x[k][u], f);
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float term = f[e] * s[k];
                            acc[u][e] = have ? acc[u][e] + term : term;
                        }
                    }
                }
                have = true;
            }
        }
#pragma unroll
        for (int u = 0; u < MR_UNROLL; ++u) {
            if (v0 + u * MR_THREADS < vecs)
                out[row_base + v0 + u * MR_THREADS] = have ? pack8<F16>(acc[u]) : make_uint4(0u, 0u, 0u, 0u);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): the stores are out, the next chunk's loads do not queue behind them
    }
}

template <int K>
int launch(const imd_mix_rows_params& p, hipStream_t s, const char* n) {
    MixRowsArgs<K> a;
    unsigned long long total = 0;
    for (int j = 0; j < MR_SEGS; ++j) {
        const int q = j < p.segments ? j : p.segments - 1;
        for (int k = 0; k < K; ++k) a.src[k][j] = reinterpret_cast<const uint4*>(p.src[k][q]);
        a.dst[j] = reinterpret_cast<uint4*>(p.dst[q]);
        a.vecs[j] = (uint32_t)(p.row_elems[q] / 8);
        a.cpr[j] = (a.vecs[j] + MR_CHUNK_VECS - 1) / MR_CHUNK_VECS;
        if (j < p.segments) {
            total += (unsigned long long)p.rows * a.cpr[j];
            if (total >= 0x80000000ull) return imd_set_error("%s: operand too large (2^31 chunks of 16 KiB or more)", n);
        }
        a.chunk_end[j] = (uint32_t)total;
    }
    a.chunks = (uint32_t)total;
    a.rows = (uint32_t)p.rows;
    const dim3 grid((unsigned)(total < (unsigned long long)MR_MAX_BLOCKS ? total : MR_MAX_BLOCKS));
    if (p.dtype == IMD_DTYPE_F16) hipLaunchKernelGGL((residual_mix_rows_kernel<true, K>), grid, dim3(MR_THREADS), 0, s, a, p.scales);
    else hipLaunchKernelGGL((residual_mix_rows_kernel<false, K>), grid, dim3(MR_THREADS), 0, s, a, p.scales);
    return imd_check_launch(n);
}

}  // namespace

int imd_launch_residual_mix_rows(const imd_mix_rows_params& p, hipStream_t s) {
    // (capi.cpp has checked the block: dtype, sources, segments, rows, row_elems, pointers, alignment and overlap)
    const char* n = "residual_mix_rows";
    static_assert(MR_SRCS == 4, "one instantiation per source count");
    switch (p.sources) {
        case 1: return launch<1>(p, s, n);
        case 2: return launch<2>(p, s, n);
        case 3: return launch<3>(p, s, n);
        default: return launch<4>(p, s, n);
    }
}
