// row_tile.hpp -- the row-tile K loops that k_resblock_mid (unet_resblock_kernels.hip) and k_conv_rows (unet_rows_kernels.hip)
// share, with their weight loads: a pixel tile is one output row of a zero-bordered LDS slab, a wave owns three 16-channel weight
// tiles (v_mfma_f32_16x16x32_bf16, weights as the A operand) and streams its weights global -> registers through a ring of two units
// (ctdd/unet_engine.py: pack_row_tile_weights).  rt_gemm_rows is the loop of the kernels with one wave per SIMD (two fragment sets),
// rt_gemm_rows_1buf that of the eight-wave splits of k_conv_rows and k_conv_rows_head (one set).
//
// Deliberately NOT here, because lifting them changes the register allocation of the kernels they are inlined into (compare the
// device assembly before and after when trying again): the 8-channel GroupNorm + Swish conversion, the group sums -> scale / shift
// derivation and the fp32 partials -> fp64 reduction of rb_groupnorm / rm_gn1_stats / rm_gn1_apply / cr_fill / k_conv_rows, and
// the 1x1 skip loops rm_gemm_skip / cr_gemm_skip (a band offset passed to k_resblock_mid, or band-offset pointers passed to
// k_conv_rows, each move one of the two kernels off its code).
#pragma once
#include <type_traits>

#include "common.hpp"

namespace ctdd {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2v = __attribute__((ext_vector_type(2))) __bf16;
using f32x2v = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int RT_UNIT = 9 * 512;                               // bf16 elements of one (32 channels, dx) unit of a 3x3 weight stream

__device__ inline unsigned rt_pack2(float a, float b) {
  f32x2v v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2v));
}
// the value again, as one the compiler knows nothing about: what is derived from it is computed where it is used instead of being
// kept in registers (the pixel indices of the row tiles) across the K loops
__device__ inline int rt_again(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// one unit of a 3x3 weight stream: [dy][tile] fragments of 1 KiB each (ctdd_unet.h)
__device__ __attribute__((always_inline)) inline void rt_wload9(u32x4 (&dst)[3][3], const unsigned short* __restrict__ wrow, int u) {
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int t = 0; t < 3; ++t) dst[dy][t] = *(const u32x4*)(wrow + (size_t)u * RT_UNIT + (dy * 3 + t) * 512);
}
// one 32-channel unit of a 1x1 weight stream: [tile] fragments
__device__ __attribute__((always_inline)) inline void rt_wload3(u32x4 (&dst)[3], const unsigned short* __restrict__ wrow, int u) {
#pragma unroll
  for (int t = 0; t < 3; ++t) dst[t] = *(const u32x4*)(wrow + (size_t)u * 1536 + t * 512);
}

// The K loop of a 3x3 segment of nunits / 3 32-channel blocks held in columns [0, 32 nunits / 3) of a zero-bordered slab of PITCH
// positions per padded row at RS bytes per position: pixel tile y = output row y (NPT of them), lane j = a padded column.  Units
// in the order (channel block, dx), weight ring wr holding units 0 and 1 (requested a phase ago).  fb: byte address of this
// lane's position of padded row 0 + its k quarter.  Unit u: F[r] = the fragment of padded row r at that column shift, read ONCE;
// output row y takes acc[t][y] += W[dy][t] F[y + dy].  The fragments of unit u + 1 are requested while unit u computes
// (F[y + 2] ahead of row y's matrix instructions, so at most NPT + 5 fragments are alive), the weights of unit u + 2 when unit u
// has consumed its slot.  The request past the last unit repeats the last unit's addresses.  FULL: all NPT rows, one straight
// line per unit (rows past the image read zeros and are never stored); otherwise rows y >= H are skipped wave-uniformly.
template <bool FULL, int RS, int PITCH, int NPT>
__device__ __attribute__((always_inline)) inline void rt_gemm_rows(f32x4 (&acc)[3][NPT], u32x4 (&wr)[2][3][3], const unsigned short* __restrict__ wrow,
                                                                  int nunits, const unsigned char* sm, int fb, int H) {
  int un = 0, dxn = 0, cbn = 0;                                 // the unit whose fragments are requested next
  auto xaddr = [&]() {                                         // (selects, not branches)
    const int o = fb + (dxn - 1) * RS + cbn * 64;
    const bool more = un + 1 < nunits, wrap = dxn == 2;
    un += more ? 1 : 0;
    cbn += more && wrap ? 1 : 0;
    dxn = more ? (wrap ? 0 : dxn + 1) : dxn;
    return o;
  };
  auto fload = [&](bf16x8& f, int o, int r) { f = *(const bf16x8*)(sm + o + r * (PITCH * RS)); };
  auto step = [&](u32x4 (&slot)[3][3], bf16x8 (&fc)[NPT + 2], bf16x8 (&fn)[NPT + 2], int u, auto guard) {
    constexpr bool GUARD = decltype(guard)::value;
    if (GUARD && u >= nunits) return;
    const int o = xaddr();
    fload(fn[0], o, 0);
    fload(fn[1], o, 1);
#pragma unroll
    for (int y = 0; y < NPT; ++y) {
      if (FULL || y < H) {
        fload(fn[y + 2], o, y + 2);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int t = 0; t < 3; ++t)
            acc[t][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, slot[dy][t]), fc[y + dy], acc[t][y], 0, 0, 0);
        // (pins the request for F[y + 2] to this row: left alone, the scheduler gathers a unit's requests at the end of the unit
        // before, where the first rows wait for them, and sinks both slots' weight loads to the end of the loop body, where the
        // next iteration drains them with vmcnt(0))
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (!GUARD || u + 2 < nunits) rt_wload9(slot, wrow, u + 2);
    __builtin_amdgcn_sched_barrier(0);
  };
  bf16x8 F[2][NPT + 2];
  {
    const int o = xaddr();
#pragma unroll
    for (int r = 0; r < NPT + 2; ++r)
      if (FULL || r < H + 2) fload(F[0][r], o, r);
  }
  // vmcnt(0): the ring's first two units have landed (they were requested a phase ago).  Entered with loads of unknown age in
  // flight, the loop's own waits are merged with that state and come out as vmcnt(8 .. 0) at the top of every iteration: the
  // ring drained once per two units.  Entered with nothing in flight they are the counted vmcnt(9 ..) of the ring.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  int u0 = 0;
  for (; u0 + 4 <= nunits; u0 += 2) {
    step(wr[0], F[0], F[1], u0, std::false_type{});
    step(wr[1], F[1], F[0], u0 + 1, std::false_type{});
  }
  for (; u0 < nunits; u0 += 2) {
    step(wr[0], F[0], F[1], u0, std::true_type{});
    step(wr[1], F[1], F[0], u0 + 1, std::true_type{});
  }
}

// The same K loop (FULL) on ONE set of NPT + 2 fragments, for a wave that has a partner on its SIMD to issue under its LDS waits
// and no registers for a second set: the fragment of padded row y is dead once output row y has taken its nine matrix
// instructions, and is requested again there for unit u + 1 (rows NPT and NPT + 1 behind the last output row), so every fragment
// is requested at least NPT - 2 output rows before its first use.  Per output pixel the order of units, dy and tiles is
// rt_gemm_rows': the same bits.
template <int RS, int PITCH, int NPT>
__device__ __attribute__((always_inline)) inline void rt_gemm_rows_1buf(f32x4 (&acc)[3][NPT], u32x4 (&wr)[2][3][3], const unsigned short* __restrict__ wrow,
                                                                       int nunits, const unsigned char* sm, int fb) {
  int un = 0, dxn = 0, cbn = 0;                                 // the unit whose fragments are requested next
  auto xaddr = [&]() {                                         // (selects, not branches)
    const int o = fb + (dxn - 1) * RS + cbn * 64;
    const bool more = un + 1 < nunits, wrap = dxn == 2;
    un += more ? 1 : 0;
    cbn += more && wrap ? 1 : 0;
    dxn = more ? (wrap ? 0 : dxn + 1) : dxn;
    return o;
  };
  auto fload = [&](bf16x8& f, int o, int r) { f = *(const bf16x8*)(sm + o + r * (PITCH * RS)); };
  bf16x8 F[NPT + 2];
  auto step = [&](u32x4 (&slot)[3][3], int u, auto guard) {
    constexpr bool GUARD = decltype(guard)::value;
    if (GUARD && u >= nunits) return;
    const int o = xaddr();
#pragma unroll
    for (int y = 0; y < NPT; ++y) {
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int t = 0; t < 3; ++t)
          acc[t][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, slot[dy][t]), F[y + dy], acc[t][y], 0, 0, 0);
      fload(F[y], o, y);
      if (y == NPT - 1) {
        fload(F[NPT], o, NPT);
        fload(F[NPT + 1], o, NPT + 1);
      }
      __builtin_amdgcn_sched_barrier(0);                        // (pins the requests to their rows, as in rt_gemm_rows)
    }
    if (!GUARD || u + 2 < nunits) rt_wload9(slot, wrow, u + 2);
    __builtin_amdgcn_sched_barrier(0);
  };
  {
    const int o = xaddr();
#pragma unroll
    for (int r = 0; r < NPT + 2; ++r) fload(F[r], o, r);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);                           // vmcnt(0), as in rt_gemm_rows
  int u0 = 0;
  for (; u0 + 4 <= nunits; u0 += 2) {
    step(wr[0], u0, std::false_type{});
    step(wr[1], u0 + 1, std::false_type{});
  }
  for (; u0 < nunits; u0 += 2) {
    step(wr[0], u0, std::true_type{});
    step(wr[1], u0 + 1, std::true_type{});
  }
}

}  // namespace ctdd
