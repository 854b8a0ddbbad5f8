// LDS-DMA (buffer_load ... lds) helpers shared by the kernels that stream operand tiles straight from global memory into
// LDS without a VGPR round trip: the attention kernels (attention_d40.hip), the DMA GEMMs and convolutions (gemm_dma*.hip, conv_patch*.hip,
// conv_img.hip), the halo-patch family (through patch_common.h) and the row-resident family (through row_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// One LDS-DMA piece: 64 lanes x 16 bytes from `rsrc` at per-lane byte offset `voff` (out of range reads 0) to LDS bytes
// [lds_addr, lds_addr + 1024) -- lane-linear, so tiles cannot be padded; bank conflicts are avoided by choosing WHICH
// 16-byte piece of global memory a lane fetches (source-side swizzle).  Inline asm on purpose: through the builtin hipcc
// assumes the DMA may alias every later ds_read of the kernel's one LDS array and drains it (s_waitcnt vmcnt(0)) in front of
// the first fragment read -- the whole point is to keep it in flight.  Completion is waited for by hand (dma_wait*) before
// the barrier that publishes the tile.  M0 (the DMA's LDS base) is saved and restored inside the statement; the leading
// s_nop covers a descriptor / offset register written by a VALU just before (hipcc does not see hazards inside an asm string).
typedef int v4i_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void dma16(const v4i_t& rsrc, uint32_t lds_addr, uint32_t voff) {
    uint32_t keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(lds_addr), "s"(rsrc) : "memory");
}
// The same piece for steady-state loops whose descriptor and LDS address were produced by SALU instructions well ahead: without the
// five leading wait states (they cover a descriptor SGPR written by a VALU -- v_readfirstlane -- immediately before)
__device__ __forceinline__ void dma16_nonop(const v4i_t& rsrc, uint32_t lds_addr, uint32_t voff) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(lds_addr), "s"(rsrc) : "memory");
}
// The steady-state piece of the unrolled loops (halo-patch convolutions, the static attention loop): three instructions and one add.
//   * LDS address = `lds_base` + LDS_OFF with LDS_OFF an IMMEDIATE: the loops are unrolled over their patch buffers / ring slots, so the
//     buffer or slot of a piece is a compile-time constant and `lds_base` (the piece's address inside buffer / slot 0) is the one
//     loop-invariant SGPR per piece.  The s_add_u32 writes M0 directly -- no save / restore of M0 (hipcc does not keep a value in M0
//     across a statement), no s_mov, no address add outside the statement; it also writes SCC, hence the clobber.
//   * `s_nop 0`: the one wait state between an SALU write of M0 and the LDS-DMA that reads it; hipcc pads nothing inside an asm string.
//     No leading nops as in dma16: descriptor and base are loop-invariant SGPRs, written long before.
//   * `voff` is a RUNNING per-lane source offset: the statement reads it, then `step` (to the piece's position in the next tap / chunk /
//     unit) is added -- one VALU add per piece instead of offset arithmetic and an out-of-range select per use.  A piece that must read
//     zeros (halo pixel outside the image, row past N) starts at 2^31: with operands < 2 GiB (the launchers check) and the few hundred
//     steps of a loop, each far below 2^31 in sum, it stays >= the descriptor's byte count under the 32-bit adds, and the DMA writes
//     zeros for out-of-range offsets.  Pieces staged past the last tap / chunk read in-range bytes that nobody multiplies.
template <int LDS_OFF>
__device__ __forceinline__ void dma16_run(const v4i_t& rsrc, uint32_t lds_base, uint32_t& voff, uint32_t step) {
    asm volatile("s_add_u32 m0, %1, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, 0 offen lds"
                 : : "v"(voff), "s"(lds_base), "s"(rsrc), "n"(LDS_OFF) : "memory", "scc");
    voff += step;
}
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// all but the N youngest pieces of this wave (N a compile-time constant)
template <int N> __device__ __forceinline__ void dma_wait_keep_n() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ v4i_t raw_rsrc(const void* base, uint32_t bytes) {      // stride 0, raw addressing, wave-uniform by construction
    const uint64_t a = (uint64_t)base;
    v4i_t r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    r[1] = __builtin_amdgcn_readfirstlane((int)((uint32_t)(a >> 32) & 0xffffu));
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000;
    return r;
}

}  // namespace
