// DICOM SEG frames -> a 0 / `one` byte mask (the contract is the comment above mmnn_unpack_frames in include/mmnn_sts.h).  A streaming
// pass bound by its stores: the mask is eight times the bit stream it is unpacked from.
//
//   unpack_frames_kernel  one lane = 16 consecutive bytes of `out`, aligned to 16 bytes of the ADDRESS (as csrc/rtstruct.hip aligns its
//                         groups): an output that starts `s` bytes past a 16-byte boundary shifts the groups left by s, so that only
//                         the first and the last group of the volume are cut and fall back to byte stores; every other lane issues
//                         one 16-byte store, and a wave writes 1 KiB without a gap.  The volume is flat: a group does not care where a
//                         row ends.  It does care where a slice ends, because the frames of two slices sit anywhere in the stream: a
//                         group is walked in runs that stay inside one slice (one run, unless x*y is no multiple of 16 or s != 0 and
//                         the group meets a slice's end; more than two only when x*y < 16).  For a run of n <= 16 voxels from in-slice
//                         pixel p the frames listed for the slice are OR-ed: frame f holds the run at stream bits f*x*y + p ..., which
//                         start in the middle of a byte whenever f*x*y + p is no multiple of 8.  The run is read as one or two aligned
//                         32-bit words of the stream and a funnel shift; the second word is loaded only when the run reaches into it,
//                         so no word is touched that holds no bit of a listed, valid frame's pixels.  (The aligned word around the
//                         stream's first or last byte may reach up to 3 bytes beyond `bits` inside the same 4-byte cell; those bits
//                         are shifted or masked away.)  A slice without frames costs its stores and two loads of slice_first.  The
//                         lanes of a wave share the slice almost always, so slice_first and refs are read at wave-uniform addresses.
//                         No LDS, no atomics.
#include "../../include/mmnn_sts.h"
#include "common.hpp"
#include "mask_bytes.hpp"

namespace mmnn {

constexpr int UF_TPB = 256;

struct UfArgs {
  const uint8_t* bits;
  const int* refs;                          // [n_refs] frame indices
  const int* slice_first;                   // [Z + 1]
  uint8_t* out;
  unsigned N;                               // X * Y * Z  (< 2^31)
  unsigned XY;                              // X * Y
  int n_frames, n_refs;
  unsigned lead;                            // out & 15
  unsigned one;                             // 1..255
};

// bits [b, b + n) of the stream, 1 <= n <= 16, in the low bits of the result (bit b lowest)
__device__ __forceinline__ unsigned uf_run(const uint8_t* bits, long b, int n) {
  const uintptr_t at = (uintptr_t)bits + (uintptr_t)(b >> 3);
  const unsigned* w = reinterpret_cast<const unsigned*>(at & ~(uintptr_t)3);
  const unsigned sh = (unsigned)(at & 3) * 8u + (unsigned)(b & 7);               // 0..31
  const unsigned lo = w[0];
  const unsigned hi = sh + (unsigned)n > 32u ? w[1] : 0u;
  return __funnelshift_r(lo, hi, sh) & ((1u << n) - 1u);
}

__global__ void __launch_bounds__(UF_TPB) unpack_frames_kernel(const UfArgs a) {
  const unsigned g = blockIdx.x * UF_TPB + threadIdx.x;
  const long o0 = (long)g * 16 - a.lead;                                         // the group's first byte as an offset into `out`
  if (o0 >= (long)a.N) return;
  const unsigned ob = o0 < 0 ? 0u : (unsigned)o0;
  const unsigned oe = o0 + 16 < (long)a.N ? (unsigned)(o0 + 16) : a.N;
  unsigned m = 0u;                                                               // bit t: voxel o0 + t is set
  unsigned o = ob;
  unsigned k = o / a.XY, p = o - k * a.XY;
  while (o < oe) {
    unsigned n = a.XY - p;
    if (n > oe - o) n = oe - o;
    const int c0 = a.slice_first[k], c1 = a.slice_first[k + 1];
    unsigned run = 0u;
    if (c0 >= 0 && c0 <= c1 && c1 <= a.n_refs) {
      for (int c = c0; c < c1; ++c) {
        const int f = a.refs[c];
        if (f >= 0 && f < a.n_frames) run |= uf_run(a.bits, (long)f * a.XY + p, (int)n);
      }
    }
    m |= run << (o - (unsigned)o0);          // (o >= o0, also when o0 is negative: the difference is 0..15)
    o += n;
    ++k;
    p = 0u;
  }
  store_mask_bits(a.out + o0, (int)((long)ob - o0), (int)((long)oe - o0), m, a.one);
}

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int mmnn_unpack_frames(const mmnn_unpack_frames_desc* d, const uint8_t* bits, const int32_t* refs, const int32_t* slice_first, uint8_t* out,
                       void* stream_) {
  MMNN_REQUIRE(d, "unpack_frames: null descriptor");
  MMNN_REQUIRE(d->x >= 1 && d->y >= 1 && d->z >= 1, "unpack_frames: non-positive extent %d x %d x %d", d->x, d->y, d->z);
  MMNN_REQUIRE((double)d->x * d->y * d->z < 2147483648.0, "unpack_frames: extent %d x %d x %d holds 2^31 voxels or more", d->x, d->y, d->z);
  MMNN_REQUIRE(d->n_frames >= 0, "unpack_frames: n_frames %d is negative", d->n_frames);
  MMNN_REQUIRE(d->n_refs >= 0, "unpack_frames: n_refs %d is negative", d->n_refs);
  MMNN_REQUIRE(d->one >= 1 && d->one <= 255, "unpack_frames: one = %d outside 1..255", d->one);
  MMNN_REQUIRE(slice_first && out, "unpack_frames: null argument");
  MMNN_REQUIRE(d->n_refs == 0 || (bits && refs), "unpack_frames: %d frame references and a null bits / refs pointer", d->n_refs);
  MMNN_REQUIRE((uintptr_t)refs % sizeof(int32_t) == 0 && (uintptr_t)slice_first % sizeof(int32_t) == 0,
               "unpack_frames: refs / slice_first not aligned to 4 bytes");
  const size_t n = (size_t)d->x * d->y * d->z, xy = (size_t)d->x * d->y;
  if (bits) {
    const size_t stream_bytes = ((size_t)d->n_frames * xy + 7) / 8;
    const uintptr_t b0 = (uintptr_t)bits, b1 = b0 + stream_bytes, o0 = (uintptr_t)out, o1 = o0 + n;
    MMNN_REQUIRE(b1 <= o0 || o1 <= b0, "unpack_frames: bits and out overlap");
  }
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  UfArgs a{};
  a.bits = bits; a.refs = refs; a.slice_first = slice_first; a.out = out;
  a.N = (unsigned)n; a.XY = (unsigned)xy;
  a.n_frames = d->n_frames; a.n_refs = d->n_refs;
  a.lead = (unsigned)((uintptr_t)out & 15);
  a.one = (unsigned)d->one;
  const long groups = ((long)n + a.lead + 15) / 16;
  MMNN_LAUNCH(unpack_frames_kernel, dim3((unsigned)cdiv(groups, UF_TPB)), dim3(UF_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
