// Blocks shared by the attention kernels (attention.hip, attention_d40.hip, attention_d40_fp8.hip, attention_d512.hip), each with its explanation
// once.  Rule: a helper is used at a site only if the file's device assembly stays what it was; DESIGN 2.1d lists what stayed inline.
#pragma once
#include "common.h"
#include "lds_dma.h"
#include "imd_kernels.h"

namespace {

// 16-byte raw buffer load through a descriptor over one (batch, head)'s K rows / V^T rows: a byte offset past the descriptor's size reads as
// zero, so tails and "this thread has no vector" cases need no branch -- they pass OOB.
typedef __attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t v4u;
__device__ __forceinline__ uint4 buf_load16(const __amdgpu_buffer_rsrc_t& rs, uint32_t byte_off) {
    const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, 0);
    return make_uint4(v[0], v[1], v[2], v[3]);
}
constexpr uint32_t OOB = 0xffffffffu;

// Packed 3-input maximum (v_pk_maximum3_f16): on non-negative 16-bit float patterns (fp16 OR bf16) it is the maximum of the patterns as integers,
// with inf / NaN patterns propagating.  Two spellings that do not merge: the scheduler sees an asm statement and a builtin differently, and each
// kernel's code depends on the one it was tuned with (the builtin in attention.hip: 6,307 lines of its assembly differ; the asm in attention_d40.hip: 28,309).
__device__ __forceinline__ uint32_t pk_max3_f16(uint32_t a, uint32_t b, uint32_t c) {      // attention.hip
    uint32_t d;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max3(uint32_t a, uint32_t b, uint32_t c) {          // attention_d40.hip
    const h2_t x = __builtin_bit_cast(h2_t, a), y = __builtin_bit_cast(h2_t, b), z = __builtin_bit_cast(h2_t, c);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_maximum(__builtin_elementwise_maximum(x, y), z));
}

// LDS layout of a register-staged K / V^T buffer (16-bit operands): [V^T rows][K rows] of a 64-key tile, rows padded by 16 bytes to an odd number
// of 16-byte slots (conflict-free b128 fragment reads).  V^T rows kept: the D real rows plus (when D < DPV) the all-ones row D that yields the
// softmax denominator.  The remaining pad rows of the last 32-row MFMA block are NOT stored: their fragment reads run into the K rows that follow
// (finite garbage in, accumulator rows nobody reads out) -- 26 KB instead of 32 KB per workgroup for d = 40, i.e. 6 resident workgroups per CU
// instead of 5.  phantom_rows_fit is that condition; every layout with unstored V^T rows asserts it (the LDS-DMA and fp8 layouts too).
constexpr bool phantom_rows_fit(int dpv, int vrows, int vstr, int kbytes) { return (dpv - vrows) * vstr <= kbytes; }
struct AttnTile { static constexpr int KT = 64, VSTR = KT * 2 + 16; };      // keys per staged tile / unit; bytes per V^T LDS row (9 x 16 B)
template <int D> struct AttnCfg : AttnTile {
    static constexpr int DPK = (D + 15) / 16 * 16, DPV = (D + 31) / 32 * 32;
    static constexpr int NKT = DPK / 16, NDT = DPV / 32;
    static constexpr int KSTR = DPK * 2 + 16;      // bytes per K LDS row (d = 40: 112 B = 7 x 16 B)
    static constexpr int VROWS = DPV > D ? D + 1 : DPV, VBYTES = VROWS * VSTR, BUF = VBYTES + KT * KSTR;
    static_assert(phantom_rows_fit(DPV, VROWS, VSTR, KT * KSTR), "phantom V^T rows must stay inside the K rows");
    static constexpr int KVECS = (KT * (DPK / 8) + 255) / 256, VVECS = (D * (KT / 8) + 255) / 256;      // 16-byte vectors per thread and tile
};

// Pad slot D.  When D is no multiple of the MFMA's contraction / row block, slot D does two jobs (the d = 40 kernels, the generic kernel at 40 / 80):
//   * QK^T: K's pad column D holds 1 and Q's pad slot D holds -m_ref, so S comes out as q.k - m_ref.  A Q fragment is 8 consecutive head-dim values,
//     fragment t of half-wave hi covering 16 t + 8 hi .. + 7: slot D is element 0 (D % 8 == 0: the low half of word .x) of fragment QPAD_T in the lanes with hi == QPAD_HI;
//   * P.V: V^T row D is all ones, so accumulator row D is the softmax denominator.  Register r of a 32x32 accumulator block is row
//     8 (r >> 2) + 4 hi + (r & 3): row D is register L_REG of block L_DT in the lanes with hi == L_HI.
// In the fp8 kernel (1-byte elements, one 64-slot contraction, lane half hi = slots 32 hi .. + 31) the Q slots D, D + 1 are the low 16 bits of dword
// QPAD8_W in the lanes with hi == QPAD8_HI; its accumulator layout is the same.
template <int D> struct AttnPad {
    static_assert((D % 8) == 0, "pad slot must start a 16-bit pair");
    static constexpr int QPAD_T = D / 16, QPAD_HI = (D % 16) / 8;
    static constexpr int L_DT = D / 32, L_REG = ((D % 32) & 3) + 4 * ((D % 32) >> 3), L_HI = ((D % 32) >> 2) & 1;
    static constexpr int QPAD8_HI = (D % 64) / 32, QPAD8_W = (D % 32) / 4;
};

// XCD-aware work list.  Hardware block L runs on XCD L % 8 (private 4 MiB L2 each).  Every XCD gets a contiguous slice of the work list, so that all
// q-tiles of one (batch, head) -- which re-read the same K / V^T -- hit the same L2 instead of pulling it through all eight.  List order: q-tile
// fastest, then BATCH, then head: an XCD's slice then holds whole heads across all batch rows, i.e. the same mix of two-phase (garment) and one-phase
// rows as every other XCD.  Two steps, because the kernels do not all follow one helper: attn_work_index, position of this workgroup
// in that list, and attn_work_split, index -> (q-tile, head, batch); attn_work_item is both.  ORDER says whether the plain dispatch order can be had
// instead: never, by the tuning knob imd_attn_params.flags & 1 (tested where the kernels always tested it: behind the arithmetic), or always.
// (gemm_common.h::xcd_remap is the same first step behind the GEMMs' flag test; the attention files do not include that header.)
enum : int { WORK_XCD = 0, WORK_KNOB = 1, WORK_PLAIN = 2 };
template <int ORDER>
__device__ __forceinline__ unsigned attn_work_index(const AttnParams& p) {
    const unsigned gx = gridDim.x, gy = gridDim.y, gz = gridDim.z, total = gx * gy * gz;
    const unsigned Lb = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const unsigned xcd = Lb & 7u, slot = Lb >> 3;
    const unsigned q8 = total >> 3, r8 = total & 7u;          // bijective also when total % 8 != 0
    unsigned w = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    if (ORDER == WORK_PLAIN || (ORDER == WORK_KNOB && (p.flags & 1))) w = Lb;
    return w;
}
__device__ __forceinline__ void attn_work_split(unsigned w, int& wx, int& h, int& b) {
    const unsigned gx = gridDim.x, gz = gridDim.z;
    wx = (int)(w % gx);
    b = (int)((w / gx) % gz);
    h = (int)(w / (gx * gz));
}
template <int ORDER>
__device__ __forceinline__ void attn_work_item(const AttnParams& p, int& wx, int& h, int& b) { attn_work_split(attn_work_index<ORDER>(p), wx, h, b); }

// The constant V^T row D of every LDS buffer, written once and never restaged.  `word` is the 32-bit pattern of the row (16-bit kernels: two ones; fp8: four 2^ev); buffer i's row starts at i * BUFB + ROW_OFF
// and is ROWB bytes long; NT = threads of the workgroup.
template <int NBUF, int BUFB, int ROW_OFF, int ROWB, int NT>
__device__ __forceinline__ void attn_const_row(char* smem, int tid, uint32_t word) {
    constexpr int PADV = ROWB / 16;
    for (int v = tid; v < NBUF * PADV; v += NT)
        *reinterpret_cast<uint4*>(smem + (v / PADV) * BUFB + ROW_OFF + (v % PADV) * 16) = make_uint4(word, word, word, word);
}

}  // namespace
