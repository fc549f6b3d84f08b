// Three-piece bf16 form of an fp32 value, and the building blocks of the kernels that multiply in it (conv3_bf16x3.hip): x = hi + mid + lo,
// each piece rounded to nearest from what the pieces before it left over (24 mantissa bits).  One helper for every producer of the pieces
// -- the weight packer (elementwise.hip) and the operand split passes (conv3_bf16x3.hip) -- so that the matrix kernels read exactly the
// pieces they used to form themselves.
//   Pre-split layouts, 16-byte entries of 8 consecutive channels (one LDS operand row / one MFMA register fragment):
//     operand planes   [piece][n][c / 8][voxel]                     (written per launch by conv3_split_*_kernel)
//     weight panels    [piece][tap][k / 8][row][8]  k = the reduction channel, row = the output channel of the launch (pack kinds 5, 6)
//   plane_entry / plane_piece_stride and panel_entry / panel_pos below ARE these layouts: every writer and reader indexes through them.
//   A kernel of the family is built from: split3x8 / store_pieces (producers), mfma_bf16x3 (the product), HaloTile (tile geometry, the
//   workgroup -> tile decomposition, the tile count) and HaloStage (global -> registers -> LDS staging of a chunk's halo tile); acc_row
//   and half_sum2 (common.hpp) for the epilogue.  It supplies its own tap loop, commit schedule and epilogue.
#pragma once
#include "common.hpp"

namespace mmnn {

#if defined(__HIPCC__)
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8_t as_bf16x8(uint4 v) { return __builtin_bit_cast(bf16x8_t, v); }

// ---- layouts (entry = 16 bytes) -------------------------------------------------------------------------------------------
// operand planes: entries per piece, and the entry of (sample n, channel group c8, voxel v) inside a piece
__host__ __device__ constexpr long plane_piece_stride(int N, int C8, int V) { return (long)N * C8 * V; }
__host__ __device__ constexpr long plane_entry(int n, int c8, int v, int C8, int V) { return ((long)n * C8 + c8) * V + v; }
// weight panels of K8 channel groups x R rows: the entry of (piece, tap, channel group k8, row), and the coordinates of entry i of a piece
__host__ __device__ constexpr long panel_entry(int piece, int tap, int k8, int row, int K8, int R) {
  return ((long)(piece * 27 + tap) * K8 + k8) * R + row;
}
__device__ __forceinline__ void panel_pos(long i, int K8, int R, int& tap, int& k8, int& row) {
  row = (int)(i % R);
  const long k = i / R;
  k8 = (int)(k % K8);
  tap = (int)(k / K8);
}

// ---- pieces ---------------------------------------------------------------------------------------------------------------
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
// split eight values and store their piece entries: `dst` = the entry's place in piece 0, `ps` = entries per piece
__device__ __forceinline__ void store_pieces(uint4* __restrict__ dst, long ps, const float (&v)[8]) {
  uint4 hi, mid, lo;
  split3x8(v, hi, mid, lo);
  dst[0] = hi; dst[ps] = mid; dst[2 * ps] = lo;
}

// acc += a * b for operands in pieces [hi, mid, lo]: six MFMAs, the lo.lo, mid.lo and lo.mid products are below fp32 resolution.
// Smallest products first: their sum is formed before it meets the large one.
__device__ __forceinline__ void mfma_bf16x3(f32x16_t& acc, const bf16x8_t (&a)[3], const bf16x8_t (&b)[3]) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}

// ---- halo tile ------------------------------------------------------------------------------------------------------------
// A workgroup of 256 threads works on TD x TH x 32 voxels = ROWS rows of 32 consecutive w (row t: d = t / TH, h = t % TH), one
// KC = 16-channel chunk at a time.  In LDS a chunk's halo tile is three bf16 planes [piece][channel half][halo voxel] of 16-byte entries
// (BUF entries); a kernel keeps two such buffers.
constexpr int BF16X3_KC = 16;
template <int TD_, int TH_, int TW_>
struct HaloTile {
  static constexpr int TD = TD_, TH = TH_, TW = TW_;
  static constexpr int HD = TD + 2, HH = TH + 2, HW = TW + 2, HV = HD * HH * HW, ROWS = TD * TH;
  static constexpr int ITEMS = (2 * HV + 255) / 256;                                       // staging items per thread and chunk
  static constexpr int BUF = 6 * HV;
  static constexpr size_t OPER_BYTES = (size_t)2 * BUF * 16;                               // two buffers
  static_assert(TW == 32, "rows of 32 voxels");
  static_assert(4 * ROWS * 16 * 64 * sizeof(float) <= OPER_BYTES, "four waves' partial tiles fit the operand buffers");

  // tiles of a launch (host), and workgroup b's tile: its first voxel and its sample
  static long count(int N, int D, int H, int W) { return (long)N * cdiv(D, TD) * cdiv(H, TH) * cdiv(W, TW); }
  int w0, h0, d0, n;
  __device__ __forceinline__ HaloTile(int b, int D, int H, int W) {
    const int twn = (W + TW - 1) / TW, thn = (H + TH - 1) / TH, tdn = (D + TD - 1) / TD;
    w0 = (b % twn) * TW; b /= twn;
    h0 = (b % thn) * TH; b /= thn;
    d0 = (b % tdn) * TD;
    n = b / tdn;
  }
  // voxel `col` of row t: its offset in the volume, and whether it is inside
  __device__ __forceinline__ bool row_pos(int t, int col, int D, int H, int W, int& o) const {
    const int d = d0 + t / TH, h = h0 + t % TH, w = w0 + col;
    o = (d * H + h) * W + w;
    return d < D && h < H && w < W;
  }
  // halo voxel that tap (td, th, tw) reads for voxel `col` of row t
  static __device__ __forceinline__ int tap_hv(int t, int col, int td, int th, int tw) {
    return ((t / TH + td) * HH + (t % TH + th)) * HW + (col + tw);
  }
  // LDS entry of (piece p, channel half g, halo voxel hv) inside a buffer
  static __device__ __forceinline__ int lds_entry(int p, int g, int hv) { return (p * 2 + g) * HV + hv; }
};

// Staging of a chunk's halo tile, global -> registers -> LDS, so that the loads of chunk ch + 1 fly under the MFMAs of chunk ch.  Item =
// (channel half g, halo voxel hv), g the slow index: a wave's 64 lanes copy 64 consecutive halo entries of one plane.  Thread tid holds
// items tid, tid + 256, ...; outside the volume an item is zero (padding AFTER the operand's prologue).  The registers in between (Regs)
// are the kernel's own array, not a member: as a member the forward's allocation came out 5 registers above its 482.
template <class T>
struct HaloStage {
  T tile;
  const uint4* __restrict__ xin;    // piece 0, the tile's sample
  long ps;                          // entries per piece
  int C8, V, tid, D, H, W;
  typedef uint4 Regs[T::ITEMS][3];  // [item][piece]
  __device__ __forceinline__ HaloStage(const T& tile, const uint4* planes, int N, int C8, int tid, int D, int H, int W)
      : tile(tile), xin(planes + plane_entry(tile.n, 0, 0, C8, D * H * W)), ps(plane_piece_stride(N, C8, D * H * W)), C8(C8), V(D * H * W), tid(tid), D(D), H(H), W(W) {}
  __device__ __forceinline__ bool item_pos(int it, int& g, int& hv, int& o) const {
    const int item = tid + it * 256;
    g = item >= T::HV;
    hv = item - g * T::HV;
    const int hd = hv / (T::HH * T::HW), hh = (hv / T::HW) % T::HH, hw = hv % T::HW;
    const int d = tile.d0 + hd - 1, h = tile.h0 + hh - 1, w = tile.w0 + hw - 1;
    o = (d * H + h) * W + w;
    return item < 2 * T::HV && (unsigned)d < (unsigned)D && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
  }
  __device__ __forceinline__ void issue(Regs& xr, int ch) const {
#pragma unroll
    for (int it = 0; it < T::ITEMS; ++it) {
      int g, hv, o;
      const bool ok = item_pos(it, g, hv, o);
      const uint4* src = xin + plane_entry(0, 2 * ch + g, o, C8, V);
#pragma unroll
      for (int p = 0; p < 3; ++p) xr[it][p] = ok ? src[p * ps] : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  __device__ __forceinline__ void commit_item(const Regs& xr, int it, uint4* buf) const {
    int g, hv, o;
    item_pos(it, g, hv, o);
    if (tid + it * 256 >= 2 * T::HV) return;
#pragma unroll
    for (int p = 0; p < 3; ++p) buf[T::lds_entry(p, g, hv)] = xr[it][p];
  }
  __device__ __forceinline__ void commit(const Regs& xr, uint4* buf) const {
#pragma unroll
    for (int it = 0; it < T::ITEMS; ++it) commit_item(xr, it, buf);
  }
};
#endif

}  // namespace mmnn
