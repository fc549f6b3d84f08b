// Mask bits to mask bytes: what the contour rasteriser (rtstruct.hip) and the SEG frame unpacker (seg.hip) share.  Both build 16 mask
// bits per lane in a register and write them as 16 bytes to a 16-byte-aligned group of the output volume.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmnn {

// four bits -> four bytes of 0 / 1 (the four products occupy disjoint bit ranges: no carries)
__device__ __forceinline__ unsigned spread4(unsigned b) { return ((b & 0xFu) * 0x00204081u) & 0x01010101u; }

// Bit t of `bits` -> byte group[t] = 0 or `one` (1..255), for the bytes b0 <= t < b1 of the group (0 <= b0 < b1 <= 16); `group` is
// 16-byte aligned.  One 16-byte store for a whole group; a group cut by the start or the end of its row, span or volume goes byte by byte.
__device__ __forceinline__ void store_mask_bits(uint8_t* group, int b0, int b1, unsigned bits, unsigned one) {
  if (b1 - b0 == 16) {
    uint4 v;
    v.x = spread4(bits) * one; v.y = spread4(bits >> 4) * one; v.z = spread4(bits >> 8) * one; v.w = spread4(bits >> 12) * one;
    *reinterpret_cast<uint4*>(group) = v;
  } else {
    uint8_t* p = group + b0;
    bits >>= b0;
    for (int n = b1 - b0; n > 0; --n, ++p, bits >>= 1) *p = (uint8_t)((bits & 1u) * one);
  }
}

}  // namespace mmnn
