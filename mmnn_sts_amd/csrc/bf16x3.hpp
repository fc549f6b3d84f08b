// Three-piece bf16 form of an fp32 value (conv3_bf16x3.hip): x = hi + mid + lo, each piece rounded to nearest from what the pieces before
// it left over (24 mantissa bits).  One helper for every producer of the pieces -- the weight packer (elementwise.hip) and the operand
// split passes (conv3_bf16x3.hip) -- so that the matrix kernels read exactly the pieces they used to form themselves.
//   Pre-split layouts, 16-byte entries of 8 consecutive channels (one LDS operand row / one MFMA register fragment):
//     operand planes   [piece][n][c / 8][voxel]                     (written per launch by conv3_split_*_kernel)
//     weight panels    [piece][tap][k / 8][row][8]  k = the reduction channel, row = the output channel of the launch (pack kinds 5, 6)
#pragma once
#include "common.hpp"

namespace mmnn {

#if defined(__HIPCC__)
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float r1 = x - (float)h;
  m = (__bf16)r1;
  l = (__bf16)(r1 - (float)m);
}
__device__ __forceinline__ uint32_t pack2(__bf16 lo, __bf16 hi) {
  return (uint32_t)__builtin_bit_cast(unsigned short, lo) | ((uint32_t)__builtin_bit_cast(unsigned short, hi) << 16);
}
// eight fp32 values -> their three 16-byte piece entries
__device__ __forceinline__ void split3x8(const float (&v)[8], uint4& hi, uint4& mid, uint4& lo) {
  __bf16 ph[8], pm[8], pl[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) split3(v[e], ph[e], pm[e], pl[e]);
  hi = make_uint4(pack2(ph[0], ph[1]), pack2(ph[2], ph[3]), pack2(ph[4], ph[5]), pack2(ph[6], ph[7]));
  mid = make_uint4(pack2(pm[0], pm[1]), pack2(pm[2], pm[3]), pack2(pm[4], pm[5]), pack2(pm[6], pm[7]));
  lo = make_uint4(pack2(pl[0], pl[1]), pack2(pl[2], pl[3]), pack2(pl[4], pl[5]), pack2(pl[6], pl[7]));
}
#endif

}  // namespace mmnn
