// Building blocks of the halo-patch 3x3 convolution family (conv_patch.hip, conv_ups_phase.hip, conv_patch2.hip, conv_patch3.hip): a
// workgroup owns a TH x TW block of output pixels of one image x BN output channels, stages the (TH+2) x (TW+2) input patch of a
// channel chunk in LDS once and lets the taps read their MFMA operand fragments from it at constant row offsets, while the weight
// tile of a tap streams through a ring in LDS.  What is specific to a member -- its tile, its schedule (main loop and waits), what
// its epilogue adds -- is told at the head of its file; the blocks every member repeats live here, each with its explanation.  The
// staging piece itself is lds_dma.h::dma16_run, the GroupNorm-statistics epilogue gemm_common.h::gn_stats_fold_store; row swizzle,
// accumulators -> LDS tile and the launch body are the tiled GEMMs' (tile_common.h).
//
// RULE: these helpers only move text.  A kernel uses one only if it compiles to the same instructions as
// with the block written out (compare the device assembly); where it does not, the kernel keeps the block inline and says so in one
// line.  hipcc's output follows a helper's shape: what is here is the shape that kept every user's assembly.
#pragma once
#include <type_traits>

#include "tile_common.h"

namespace {

// MFMA column (lane & 31) -> pixel of the wave's 2 x 16 pixel block (two image rows of the tile).  ds_read_b128 is serviced in the
// 16-lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31}; with the identity mapping the second image row (patch rows + TW + 2 = 18)
// lands two lanes of a group on one 16-byte bank slot (2-way conflict on every activation fragment).  This permutation gives each
// group 16 patch rows that are distinct mod 16: conflict-free at the 80-byte row stride of the register-staged form (5 r mod 16
// distinct) and, as 8 + 8 consecutive patch rows, at the unpadded swizzled rows of the LDS-DMA forms (PD below).  Every
// member has 16-pixel-wide tiles, so the one table serves them all.
__device__ constexpr unsigned char kColPix[32] = {0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 15, 4, 5, 6, 7,
                                                  30, 31, 16, 17, 22, 23, 24, 25, 26, 27, 28, 29, 18, 19, 20, 21};

// ---- tile decode: workgroup -> (image b, pixel tile ty / tx, channel tile tile_n) ----
// The map the kernel works on may be ragged (96 x 72 latents: W = 72, 36, 18): the last tile row / column hangs over the edge; its
// patch pixels outside the image read as zero like any halo pixel and its output pixels are not stored.  NMUL channel-tile slots per
// BN channels (the four phases of conv_ups_phase.hip); tile_id numbers the (pixel tile, channel tile) pairs for the split-K counters.
struct HaloTile { int tiles_x, tiles_y, n_tiles, tile_n, tile_id, tx, ty, b; };
template <int TH_, int TW_, int BN_, int NMUL = 1>
__device__ __forceinline__ HaloTile halo_tile(const ConvGemmParams& p, int H, int W) {
    HaloTile t;
    t.tiles_x = (W + TW_ - 1) / TW_; t.tiles_y = (H + TH_ - 1) / TH_;
    t.n_tiles = NMUL * ((p.N + BN_ - 1) / BN_);
    int bid;
    xcd_tile_order(p.flags, (int)(gridDim.x / t.n_tiles), t.n_tiles, bid, t.tile_n);      // bid = pixel-tile index
    t.tile_id = bid * t.n_tiles + t.tile_n;
    t.tx = bid % t.tiles_x; bid /= t.tiles_x;
    t.ty = bid % t.tiles_y;
    t.b = bid / t.tiles_y;
    return t;
}

// ---- K slices over channel chunks of CKD_ channels: slice `split` (blockIdx.y) owns chunks [c_begin, c_end); an empty range past
// the end is possible.  (Takes p and computes the chunk count itself: with the count as an argument an s_add got its operands swapped.) ----
struct KSlice { int c_begin, c_end; };
template <int CKD_>
__device__ __forceinline__ KSlice k_slice(const ConvGemmParams& p, int split) {
    const int nchunks = p.Cin / CKD_;
    const int per = (nchunks + p.split_k - 1) / p.split_k;
    KSlice k;
    k.c_begin = split * per;
    k.c_end = min(nchunks, k.c_begin + per);
    return k;
}

// ---- patch staging: stored pixel behind logical pixel (iy, ix) of image b.  The kernels tile the LOGICAL input map (= the output map)
// and apply the zero halo there; with the fused nearest-2x upsample the stored map is half as large and the source pixel is the logical
// one >> 1.  (Only this much is shared: with the halo test and the out-of-range marker in the helper too, in either of two shapes,
// conv_patch.hip and conv_patch3.hip compiled differently.) ----
__device__ __forceinline__ int halo_src_pixel(const ConvGemmParams& p, int b, int iy, int ix) {
    const int sy = p.ups ? (iy >> 1) : iy, sx = p.ups ? (ix >> 1) : ix;
    return (b * p.Hin + sy) * p.Win + sx;
}

// ---- the 8 x 16 pixel x 128 channel tile of conv_patch.hip and conv_ups_phase.hip ----
constexpr int TH = 8, TW = 16;                 // output pixels per workgroup: 8 rows x 16 columns
constexpr int PW = TW + 2, PH = TH + 2;        // halo patch
constexpr int NPIX = PH * PW;                  // 180 patch pixels
constexpr int CK = 32;                         // channels per chunk
constexpr int BN = 128;
constexpr int CLD = BN + 4;
constexpr int EROWS = 64;
constexpr int EPI_LDS = EROWS * CLD * 4;       // 33,792
// LDS-DMA geometry at CKD channels per chunk.  Both operands are written lane-linear, i.e. as unpadded rows of RB bytes: the halo
// patch of a chunk (180 pixel rows) and the weight tile of a tap (128 rows), in one-KB pieces.  Fragment reads stay conflict-free
// through the SOURCE-side swizzle of tile_common.h::lds_row_swz -- piece c of row r sits at position c ^ swz(r) -- for any 8 + 8
// consecutive rows of the patch as for aligned row groups of the weight tile.
//   CKD = 32: 64-byte rows, 12 patch pieces, 8 weight pieces, three-slot weight ring, 48 KB.
//   CKD = 64 (tile config 29): 128-byte rows -- the L2 hands a CU whole 128-byte lines (tools/probes/staging_probe.hip: 62 GB/s per CU
//   in 64-byte segments, 113 in 128-byte ones) -- 23 patch pieces (six per wave with one empty), 16 weight pieces, two-slot ring, 80 KB.
template <int CKD> struct PD {
    static constexpr int RB = CKD * 2, LPR = RB / 16;                       // row bytes, 16-byte pieces per row
    static constexpr int APIECES = (NPIX * RB + 1023) / 1024;               // 12 | 23
    static constexpr int APW = (APIECES + 3) / 4;                           // patch pieces per wave: 3 | 6
    static constexpr int AB = APW * 4 * 1024;                               // 12,288 | 24,576
    static constexpr int WPW = BN * RB / 1024 / 4;                          // weight pieces per wave and tap: 2 | 4
    static constexpr int WB = WPW * 4 * 1024;                               // 8,192 | 16,384
    static constexpr int NWR = CKD == 32 ? 3 : 2;
    static constexpr int LDS = 2 * AB + NWR * WB;                           // 49,152 | 81,920
    static_assert(LDS >= EPI_LDS, "the epilogue tile must fit the main-loop LDS");
    static __device__ __forceinline__ int swz(int r) { return lds_row_swz<RB>(r); }
};

// ---- host side ----
// What every member asks of a problem: 3x3, stride 1, symmetric padding, a map of at least one tile, whole channel chunks, a row-major
// output without GEGLU.  The input map is the output map, or half of it with the fused nearest-2x upsample (Upsample2D: interpolate ->
// conv; a source-pixel map of the patch staging).
static bool halo_geometry(const ConvGemmParams& p, int th, int tw, int ck) {
    const bool geom = p.ups ? (p.Hout == 2 * p.Hin && p.Wout == 2 * p.Win) : (p.Hin == p.Hout && p.Win == p.Wout);
    return p.taps == 9 && p.stride == 1 && !p.pad_br_only && geom && p.Hout >= th && p.Wout >= tw && (p.Cin % ck) == 0 &&
           p.mode == OUT_ROWMAJOR && p.act != ACT_GEGLU;
}
// tiles per image (= statistic partials per image of an un-split launch), and workgroups per K slice
static int halo_tiles(int H, int W, int N, int th, int tw, int bn) { return ((H + th - 1) / th) * ((W + tw - 1) / tw) * ((N + bn - 1) / bn); }
static long halo_blocks(const ConvGemmParams& p, int th, int tw, int bn) {
    return (long)(p.M / (p.Hout * p.Wout)) * halo_tiles(p.Hout, p.Wout, p.N, th, tw, bn);
}
// whether the epilogue of an un-split launch can produce GroupNorm statistics (gn_stats_add: a group has >= 8 channels; the fold: one
// thread per group)
static bool halo_stats_ok(const ConvGemmParams& p) {
    return !(p.split_k > 1 || p.out_f32 || p.gn_stats_groups <= 0 || p.gn_stats_groups > 64 || p.N % p.gn_stats_groups || (p.N / p.gn_stats_groups) < 8);
}

}  // namespace
