// DICOM slice decode: the PixelData bytes of a sorted single-frame series -> the raw voxel volume the scan ingest takes (the contract
// is the comment above mmnn_decode_slices in include/mmnn_sts.h).  A streaming pass: every stored word is read once and every output
// element written once.
//
//   decode_slices_kernel  grid (x groups of 64 * VEC columns, row blocks), block (64, DC_WAVES): lanes along x, a wave = one row
//                         segment, a grid-stride loop over the y * z rows; element offsets are 64-bit.  With an integer output a lane
//                         owns 16 bytes of the row (one 16-byte load, one 16-byte store); with the float64 output it owns two voxels
//                         (one 16-byte store, a 2-, 4- or 8-byte load).  VEC = 1 (element loads and stores) when the row length or
//                         the alignment of either buffer does not allow that.  The slice's (slope, inter) pair is the same in every
//                         lane of a row: one uniform load per row.  No LDS, no atomics.
#include "../../include/mmnn_sts.h"
#include "common.hpp"

#include <type_traits>

namespace mmnn {

constexpr int DC_WAVES = 4;
constexpr int DC_TPB = 64 * DC_WAVES;

struct DcArgs {
  const void* pixels;
  const double* scale;                      // [Z][2] (slope, inter); float64 output only
  void* out;
  int X, Y, Z;
  int shift;                                // high_bit + 1 - bits_stored
  int spare;                                // 32 - bits_stored: the sign extension's shift pair
  unsigned mask;                            // 2^bits_stored - 1
  int is_signed;
};

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) DcVec { T e[VEC]; };

// the stored value of one word: the bits_stored bits below high_bit, sign-extended from its top bit for a signed series
__device__ __forceinline__ int dc_value(unsigned word, const DcArgs& a) {
  const unsigned u = (word >> a.shift) & a.mask;
  return a.is_signed ? (int)(u << a.spare) >> a.spare : (int)u;
}

// W: the stored word (uint8_t, uint16_t, uint32_t).  An integer output has the word's width, so its element is the low bits of the
// value whatever its signedness; F64 stores v * slope + inter of the row's slice, a rounded multiply and a rounded add, never an FMA.
template <typename W, int VEC, bool F64>
__global__ void __launch_bounds__(DC_TPB) decode_slices_kernel(const DcArgs a) {
  using O = std::conditional_t<F64, double, W>;
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * VEC;
  if (x0 >= a.X) return;                    // VEC > 1 only when X % VEC == 0: a group is inside or outside as a whole
  const int R = a.Y * a.Z;
  const W* src = static_cast<const W*>(a.pixels);
  O* dst = static_cast<O*>(a.out);
  for (int r = blockIdx.y * DC_WAVES + threadIdx.y; r < R; r += gridDim.y * DC_WAVES) {
    const long idx = (long)r * a.X + x0;
    const DcVec<W, VEC> in = *reinterpret_cast<const DcVec<W, VEC>*>(src + idx);
    DcVec<O, VEC> o;
    if constexpr (F64) {
      const int k = r / a.Y;
      const double slope = a.scale[2 * k], inter = a.scale[2 * k + 1];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const int s = dc_value((unsigned)in.e[v], a);
        const double d = a.is_signed ? (double)s : (double)(unsigned)s;
        o.e[v] = __dadd_rn(__dmul_rn(d, slope), inter);
      }
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) o.e[v] = (W)(unsigned)dc_value((unsigned)in.e[v], a);
    }
    *reinterpret_cast<DcVec<O, VEC>*>(dst + idx) = o;
  }
}

namespace {

template <typename W, bool F64>
void dc_launch(const DcArgs& a, hipStream_t stream) {
  constexpr int VEC = F64 ? 2 : 16 / (int)sizeof(W);
  const size_t osz = F64 ? sizeof(double) : sizeof(W);
  const bool vec = a.X % VEC == 0 && (uintptr_t)a.pixels % (sizeof(W) * VEC) == 0 && (uintptr_t)a.out % (osz * VEC) == 0;
  const int gx = cdiv(a.X, 64 * (vec ? VEC : 1));
  int gy = cdiv((long)a.Y * a.Z, DC_WAVES);
  const int cap = cdiv(2048, gx);
  if (gy > cap) gy = cap;
  if (vec) MMNN_LAUNCH((decode_slices_kernel<W, VEC, F64>), dim3(gx, gy), dim3(64, DC_WAVES), 0, stream, a);
  else MMNN_LAUNCH((decode_slices_kernel<W, 1, F64>), dim3(gx, gy), dim3(64, DC_WAVES), 0, stream, a);
}

template <bool F64>
void dc_dispatch(const DcArgs& a, int bits_allocated, hipStream_t stream) {
  if (bits_allocated == 8) dc_launch<uint8_t, F64>(a, stream);
  else if (bits_allocated == 16) dc_launch<uint16_t, F64>(a, stream);
  else dc_launch<uint32_t, F64>(a, stream);
}

// the NIfTI code of the integer type that holds words of `bits` bits of the given signedness
int dc_integer_code(int bits, int is_signed) {
  if (bits == 8) return is_signed ? 256 : 2;
  if (bits == 16) return is_signed ? 4 : 512;
  return is_signed ? 8 : 768;
}

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int mmnn_decode_slices(const mmnn_decode_slices_desc* d, const void* pixels, const double* slice_scale, void* out, void* stream_) {
  MMNN_REQUIRE(d, "decode_slices: null descriptor");
  MMNN_REQUIRE(d->x >= 1 && d->y >= 1 && d->z >= 1, "decode_slices: non-positive extent %d x %d x %d", d->x, d->y, d->z);
  MMNN_REQUIRE((double)d->x * d->y * d->z < 2147483648.0, "decode_slices: extent %d x %d x %d holds 2^31 voxels or more", d->x, d->y, d->z);
  MMNN_REQUIRE(d->bits_allocated == 8 || d->bits_allocated == 16 || d->bits_allocated == 32,
               "decode_slices: bits_allocated %d is none of 8, 16, 32", d->bits_allocated);
  MMNN_REQUIRE(d->bits_stored >= 1 && d->bits_stored <= d->bits_allocated, "decode_slices: bits_stored %d outside 1..%d", d->bits_stored,
               d->bits_allocated);
  MMNN_REQUIRE(d->high_bit >= d->bits_stored - 1 && d->high_bit <= d->bits_allocated - 1, "decode_slices: high_bit %d outside %d..%d",
               d->high_bit, d->bits_stored - 1, d->bits_allocated - 1);
  MMNN_REQUIRE(d->is_signed == 0 || d->is_signed == 1, "decode_slices: is_signed %d is neither 0 nor 1", d->is_signed);
  const int code = dc_integer_code(d->bits_allocated, d->is_signed);
  MMNN_REQUIRE(d->out_type == 64 || d->out_type == code, "decode_slices: out_type %d is neither 64 (float64) nor %d, the integer type of %d %s bits",
               d->out_type, code, d->bits_allocated, d->is_signed ? "signed" : "unsigned");
  MMNN_REQUIRE(pixels && out, "decode_slices: null argument");
  const bool f64 = d->out_type == 64;
  MMNN_REQUIRE(!f64 || slice_scale, "decode_slices: out_type 64 needs slice_scale");
  MMNN_REQUIRE(f64 || !slice_scale, "decode_slices: slice_scale must be null for an integer out_type");
  const size_t isz = (size_t)d->bits_allocated / 8, osz = f64 ? sizeof(double) : isz;
  MMNN_REQUIRE((uintptr_t)pixels % isz == 0, "decode_slices: pixels not aligned to its element size");
  MMNN_REQUIRE((uintptr_t)out % osz == 0, "decode_slices: out not aligned to its element size");
  MMNN_REQUIRE(!f64 || (uintptr_t)slice_scale % sizeof(double) == 0, "decode_slices: slice_scale not aligned to 8 bytes");
  const size_t n = (size_t)d->x * d->y * d->z;
  const uintptr_t p0 = (uintptr_t)pixels, p1 = p0 + n * isz, o0 = (uintptr_t)out, o1 = o0 + n * osz;
  MMNN_REQUIRE(p1 <= o0 || o1 <= p0, "decode_slices: pixels and out overlap");
  if (f64) {
    const uintptr_t s0 = (uintptr_t)slice_scale, s1 = s0 + (size_t)d->z * 2 * sizeof(double);
    MMNN_REQUIRE(s1 <= o0 || o1 <= s0, "decode_slices: slice_scale and out overlap");
  }
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  DcArgs a{};
  a.pixels = pixels; a.scale = slice_scale; a.out = out;
  a.X = d->x; a.Y = d->y; a.Z = d->z;
  a.shift = d->high_bit + 1 - d->bits_stored;
  a.spare = 32 - d->bits_stored;
  a.mask = d->bits_stored == 32 ? 0xFFFFFFFFu : (1u << d->bits_stored) - 1u;
  a.is_signed = d->is_signed;
  if (f64) dc_dispatch<true>(a, d->bits_allocated, stream);
  else dc_dispatch<false>(a, d->bits_allocated, stream);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
