// conv_ring.hpp -- what the three LDS-DMA ring convolutions of unet_kernels.hip share: k_conv_ring (3x3 / 1x1, stride 1),
// k_conv_ring_s2 (Downsample) and k_conv_ring_up (the four Upsample phases).  Per 16-channel unit a slab of input pixels and
// the weights of every tap go global -> LDS by LDS-DMA in pieces of 32 rows x 32 B = 1 KiB into a ring of NBUF unit buffers,
// one or two units ahead of the matrix instructions; the two 16-byte halves of a row are swapped when bit 3 of the row is set.
// Here: the geometry of each kernel family (RingGeom), which the kernel AND its host launcher instantiate, so that the LDS
// request cannot drift from the kernel's slab; the piece layout and the half-swap swizzle; the per-lane DMA geometry and the
// 16-byte DMA call.
//
// Deliberately NOT here, because lifting them moves the kernels off their code (compare the device assembly of the nine
// instantiations before and after when trying again; helpers were tried as always_inline and as plain inline functions):
//  * the tap sequence (mask A | read the next set | DMA ops | matrix instructions) and the unit around it (wait, barrier,
//    rotate), with read_frags / mask_a / mfma_step.  As one template taking the op issuer as a functor, k_conv_ring's 3x3
//    loop came out with other control flow around its DMA ops (7277 -> 7314 .. 11014 -> 11067 lines); k_conv_ring_up kept
//    its instructions but one s_nop moved behind the first matrix instruction of the last tap, and the 64-column
//    instantiation computed four A offsets differently; k_conv_ring_s2 got other wait counts.  An always_inline tap sequence
//    put the A masks behind the next set's reads.
//  * the weight-piece source (n0 + 32 t rows, tap * C, clamp), the accumulator zeroing and the epilogue tail
//    (tile_stats_begin .. tile_stats_flush): each of them as a shared function changed k_conv_ring or the 64-column
//    instantiations of the other two -- also where the function was only used by ANOTHER kernel of this file.
//  * the swizzle as a function: fine in k_conv_ring, another v_bitop3 in the set-up of the other two; hence the macro.
//  * ring_lane in k_conv_ring: the production build is the same, the CTDD_RES_STAMPS build numbers the scalar registers of its
//    time line differently; that kernel writes the three values out (with RING_HALF).
#pragma once
#include "common.hpp"

namespace ctdd {

// ---------------------------------------------------------------- geometry, for the kernel and for its launcher
constexpr int RING_BK = 16;                                      // channels of a unit: one 32-byte LDS row per pixel / weight row
constexpr int RING_ROWB = RING_BK * 2, RING_PIECE = 32 * RING_ROWB;   // a piece: 32 rows = 1 KiB = one DMA wave-instruction
// slab pieces of 32 rows >= BMP + 2 * (33 + 1) rows: a tile of BMP flattened pixels with a halo of W + 1 on either side, W <= 33
constexpr int ring_halo_pieces(int bmp) { return (bmp + 2 * 34 + 31) / 32; }

// NW waves of MT 32-row tiles each, BNT 32-column tiles, TAPS taps, a slab of SP pieces, a ring of NBUF unit buffers
template <int NW_, int MT_, int TAPS_, int BNT_, int NBUF_, int SP_>
struct RingGeom {
  static constexpr int NW = NW_, MT = MT_, TAPS = TAPS_, BNT = BNT_, NBUF = NBUF_, SP = SP_;
  static constexpr int WM = 32 * MT, BMP = NW * WM, BN = 32 * BNT;
  static constexpr int SLABB = SP * RING_PIECE, BUFB = SLABB + TAPS * BN * RING_ROWB;
  static constexpr int TOTAL = SP + TAPS * BNT, OPS = (TOTAL + NW - 1) / NW;   // pieces of a unit, DMA ops per wave and unit
  static constexpr int DEPTH = NBUF - 1;                         // units in flight ahead of the one computed
  static constexpr int LDS = NBUF * BUFB;                        // bytes of the ring
  static_assert(DEPTH == 1 || DEPTH == 2, "ring of two or three unit buffers");
  static_assert(OPS <= 2 * TAPS, "at most two DMA ops per tap");
};
// k_conv_ring<BNT, NBUF, NW>: nine taps; a 1x1 unit has BMP rows (no halo) and one tap
template <int BNT, int NBUF, int NW>
struct RingS1 : RingGeom<NW, 2, 9, BNT, NBUF, ring_halo_pieces(NW * 64)> {
  static constexpr int SP1 = NW * 2, OPS1 = (SP1 + BNT + NW - 1) / NW;
};
// k_conv_ring_s2<BNT, NBUF>: two parity planes of PP pieces: 4 * 127 + 6 * 16 + 1 = 605 input pixels <= 2 * 320 (W <= 16)
template <int BNT, int NBUF>
struct RingS2 : RingGeom<4, 1, 9, BNT, NBUF, 2 * 10> {
  static constexpr int PP = 10, PLR = PP * 32;
};
// k_conv_ring_up<BNT, NBUF>: k_conv_ring's slab on the low-resolution pixels, the four taps of one phase
template <int BNT, int NBUF>
struct RingUp : RingGeom<8, 2, 4, BNT, NBUF, ring_halo_pieces(512)> {};

static_assert(RingS1<3, 3, 8>::SP == 19 && RingUp<3, 3>::SP == 19 && RingS1<3, 2, 4>::SP == 11 && RingS2<3, 3>::SP == 20, "slab pieces");
static_assert(RingS1<3, 3, 8>::LDS == 141312 && RingS1<3, 3, 8>::OPS == 6 && RingS1<3, 3, 8>::OPS1 == 3, "k_conv_ring<3, 3, 8>");

// ---------------------------------------------------------------- layout and DMA
// byte offset of 16-byte half `half` (0 / 1) of LDS row `row` within the row (a macro: see above)
#define RING_HALF(row, half) (((half) ^ (((row) >> 3) & 1)) << 4)

// Lane l of a DMA op fills LDS bytes [16 l, 16 l + 16) of the piece = row l / 2, stored half l & 1: it reads the 16 bytes at
// swz16 of source row rl (wlane: that place in rows of Ktot bf16, the weight matrix).
struct RingLane {
  int rl;
  unsigned swz16, wlane;
};
__device__ inline RingLane ring_lane(int lane, int Ktot) {
  const int rl = lane >> 1;
  const unsigned swz16 = (unsigned)RING_HALF(rl, lane & 1);
  return {rl, swz16, (unsigned)rl * (unsigned)Ktot * 2u + swz16};
}
__device__ inline void ring_dma16(const unsigned char* src, unsigned char* dst) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (void __attribute__((address_space(3)))*)dst, 16, 0, 0);
}

}  // namespace ctdd
