// DICOM JPEG Lossless, first-order prediction (T.81 Annex H, process 14 selection value 1; transfer syntaxes 1.2.840.10008.1.2.4.70 and
// .57 with predictor 1): the entropy-coded data of a sorted single-frame series -> the bytes an uncompressed series would hold, which
// mmnn_decode_slices then takes unchanged (the contract is the comment above mmnn_jpegll_decode in include/mmnn_sts.h; what a raw byte
// and a bit position mean, the clamps and the chunk-to-chunk state are csrc/jpegll_core.hpp, which a host program runs under the
// sanitizers).  What it shares with csrc/dicom_rle.hip is stated once: the window fill in csrc/stream_window.hpp, the span clamp, the
// round of pointer doubling and the progress in csrc/stream_core.hpp, the host-side refusals in csrc/stream_args.hpp.
//
//   jpegll_symbols_kernel  grid z, block 1024: one workgroup per frame.  The data passes through LDS in windows of JLL_CHUNK + JLL_LOOK raw
//                          bytes, filled by aligned 16-byte loads (the ragged end of the payload by bytes).  Per window:
//                            1. every thread judges one raw byte (kept, stuffed zero, end of the data); block_exclusive_scan over the
//                               judgements compacts the kept bytes into the unstuffed array and finds the first end;
//                            2. every bit position gets its successor, as if a symbol started there, and pointer doubling from the
//                               window's known entry bit marks the positions where one does: at most 13 rounds of two LDS passes (the
//                               rounds stop once the entry's pointer has left the chunk);
//                            3. every thread takes 8 positions, decodes the symbols that start there, block_exclusive_scan numbers them,
//                               and the differences go to the workspace at their sample index.  Every difference is written once.
//                          A frame that its data does not fill has zero differences from there on and status 1.  Behind the last window
//                          the workgroup sums column 0 of its own differences downwards (the predictor of a row's first sample is the
//                          sample above it) and leaves each row's first sample in the workspace.
//   jpegll_rows_kernel     grid (y, min(z, 1024)), block 64: one wave per row sums the row's differences from its first sample on, 8 per
//                          lane and a shift-up ladder across the lanes, and writes the words: 16 bytes (8 bytes at 8 bits) per lane when
//                          the row starts are aligned, element stores otherwise.
// LDS of the first kernel: raw window 1040 B, unstuffed 1047 B, marks 8 KB, hops 16 KB, table and scan words: 27 KB of a CU's 160 KB.
// 16 waves, because every step is a chain of dependent LDS reads: the waves hide each other's latency.  One lane walking the chain of a
// window in place of the doubling rounds was measured and lost by 4.6 x (noise) to 36 x (masks); it is gone.
#include "../../include/mmnn_sts.h"
#include "common.hpp"
#include "reduce.hpp"
#include "jpegll_core.hpp"
#include "stream_args.hpp"
#include "stream_window.hpp"

namespace mmnn {

constexpr int JL_WAVES = 16;
constexpr int JL_TPB = 64 * JL_WAVES;
constexpr int JL_PER = JLL_BITS / JL_TPB;    // bit positions per thread
constexpr int JR_TPB = 64;                   // of the row kernel
constexpr int JR_PER = 8;
static_assert(JLL_CHUNK == MMNN_JPEGLL_CHUNK && JLL_CHUNK == JL_TPB && JL_PER == 8 && JLL_LOOK == 16, "window geometry");
static_assert(sizeof(mmnn_jpegll_frame) == 56, "frame record");

struct JpegllArgs {
  const uint8_t* payload;
  long payload_bytes;
  const mmnn_jpegll_frame* frames;           // [z]
  uint16_t* diff;                            // [z][y][x]
  uint16_t* first;                           // [z][y]: the first sample of every row
  int32_t* status;                           // [z]
  int x, y;
};

__global__ void __launch_bounds__(JL_TPB) jpegll_symbols_kernel(const JpegllArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[JLL_WINDOW];
  __shared__ __attribute__((aligned(16))) uint8_t u[JLL_UNSTUFFED + 1];
  __shared__ __attribute__((aligned(16))) uint8_t mark[JLL_BITS];
  __shared__ uint16_t hop[JLL_BITS];
  __shared__ uint32_t scan[JL_WAVES];
  __shared__ JllTable table;
  __shared__ JllChunk chunk;
  __shared__ ChainExit left;
  const int tid = threadIdx.x;
  const long k = blockIdx.x;
  const long plane = (long)a.x * a.y;
  uint16_t* diff = a.diff + k * plane;
  const mmnn_jpegll_frame* fr = a.frames + k;
  if (tid == 0) jll_build(table, fr->bits, fr->huffval);
  JllState st = jll_begin(stream_clamp(fr->offset, fr->length, a.payload_bytes), plane);   // the same in every thread
  const uint32_t half = 1u << (jll_precision(fr->precision) - 1);
  while (stream_more(st)) {
    window_fill<JLL_WINDOW, JL_TPB>(raw, a.payload, a.payload_bytes, st.base, tid);
    for (int i = tid; i < JLL_UNSTUFFED + 1; i += JL_TPB) u[i] = 0xFF;
#pragma unroll
    for (int i = 0; i < JL_PER / 4; ++i) reinterpret_cast<uint32_t*>(mark)[i * JL_TPB + tid] = 0u;
    __syncthreads();
    // 1. stuffed zeros out, the end of the data found: thread t judges raw byte t
    const long pa = jll_prev_at(st);
    const uint32_t f = jll_judge(raw, st, tid, tid == 0 && pa >= 0 ? a.payload[pa] : -1);
    uint32_t all;
    const uint32_t before = block_exclusive_scan<JL_WAVES>(f, scan, all);
    const bool live = before < JLL_END;      // no end in front of this byte
    if (live && f == JLL_KEEP) u[before & 0xFFFFu] = raw[tid];
    if (live && f == JLL_END) chunk = jll_chunk(true, (int)(before & 0xFFFFu));
    if (tid == 0 && all < JLL_END) chunk = jll_chunk(false, (int)(all & 0xFFFFu));
    __syncthreads();
    if (tid == 0 && !chunk.last) jll_look(raw, st, u, chunk);
    __syncthreads();
    const JllChunk c = chunk;
    const bool enters = jll_enters(st.entry, c);
    // 2. the chain: the text of chain_resolve<JLL_BITS, JL_TPB, JLL_ROUNDS> (csrc/stream_window.hpp, whose contract holds here), written
    // out: through the helper the compiler schedules this kernel differently and the smooth scan and the masks decode 1.3 to 1.5 %
    // slower.  Lanes along the positions (thread t has t, t + 1024, ...): neighbouring lanes read neighbouring entries.
#pragma unroll
    for (int i = 0; i < JL_PER; ++i) hop[i * JL_TPB + tid] = (uint16_t)jll_successor(table, u, i * JL_TPB + tid, c);
    if (tid == 0) {
      left = ChainExit{st.entry, 1};
      if (enters) mark[st.entry] = 1;
    }
    __syncthreads();
    for (int r = 0; r < JLL_ROUNDS && enters; ++r) {
      uint16_t on[JL_PER];
#pragma unroll
      for (int i = 0; i < JL_PER; ++i) on[i] = chain_hop<JLL_BITS>(hop, mark, i * JL_TPB + tid);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < JL_PER; ++i) hop[i * JL_TPB + tid] = on[i];
      __syncthreads();
      if (hop[st.entry] >= JLL_BITS) break;  // (the same word in every thread; the next write of hop lies behind the next barrier)
    }
    // 3. the symbols: thread t has the positions 8 t .. 8 t + 7, i.e. the bits of unstuffed byte t
    uint16_t d[JL_PER];
    uint32_t have = 0u, count = 0u;
    const uint64_t marks = *reinterpret_cast<const uint64_t*>(mark + tid * JL_PER);
    const int64_t endbits = jll_endbits(c);
#pragma unroll
    for (int i = 0; i < JL_PER; ++i) {
      d[i] = 0;
      if ((marks >> (8 * i)) & 0xFFu) {
        const int p = tid * JL_PER + i;
        const JllSym s = jll_classify(table, u, p, endbits);
        if (jll_leaves(s, p, c)) left = jll_exit(s, p, c);     // the chain's last member in the chunk: one writer
        if (!s.cut) {
          d[i] = s.diff;
          have |= 1u << i;
          ++count;
        }
      }
    }
    uint32_t total;
    uint32_t at = block_exclusive_scan<JL_WAVES>(count, scan, total);
    const uint32_t n = stream_take(st, total);
#pragma unroll
    for (int i = 0; i < JL_PER; ++i)
      if ((have >> i) & 1u) {
        if (at < n) diff[st.done + at] = d[i];
        ++at;
      }
    __syncthreads();                         // `left` is complete
    jll_advance(st, left, c, n);
    __syncthreads();                         // the next window overwrites raw, u, mark, hop, chunk and left
  }
  const bool failed = stream_short(st);
  if (failed)
    for (long o = st.done + tid; o < plane; o += JL_TPB) diff[o] = 0;
  if (tid == 0) a.status[k] = failed ? 1 : 0;
  __threadfence_block();
  __syncthreads();                           // the workgroup's own differences are visible to all of it
  // column 0 downwards: row r starts with 2^(P-1) + the sum of the first differences of rows 0 .. r, modulo 2^16
  uint16_t* first = a.first + k * a.y;
  uint32_t carry = half;
  for (long r0 = 0; r0 < a.y; r0 += JL_TPB) {
    const long r = r0 + tid;
    const uint32_t v = r < a.y ? diff[r * a.x] : 0u;
    uint32_t sum;
    const uint32_t ahead = block_exclusive_scan<JL_WAVES>(v, scan, sum);
    if (r < a.y) first[r] = (uint16_t)(carry + ahead + v);
    carry += sum;
  }
}

// One wave per row.  VEC: every row of `diff` and of `pixels` starts on a multiple of JR_PER elements from an aligned base and x is a
// multiple of JR_PER, so a lane's JR_PER elements are one load and one store.
template <typename W, bool VEC>
__global__ void __launch_bounds__(JR_TPB) jpegll_rows_kernel(const uint16_t* diff, const uint16_t* first, int x, int y, int z, W* pixels) {
  struct alignas(VEC ? sizeof(uint16_t) * JR_PER : sizeof(uint16_t)) In { uint16_t v[JR_PER]; };
  struct alignas(VEC ? sizeof(W) * JR_PER : sizeof(W)) Out { W v[JR_PER]; };
  __shared__ uint32_t scan[1];
  const long r = blockIdx.x;
  const int lane = threadIdx.x;
  for (long k = blockIdx.y; k < z; k += gridDim.y) {
    const long row = (k * y + r) * x;
    uint32_t carry = first[k * y + r];
    for (long c0 = 0; c0 < x; c0 += JR_TPB * JR_PER) {
      const long c = c0 + lane * JR_PER;
      uint32_t v[JR_PER];
      if (VEC) {
        In in{};
        if (c < x) in = *reinterpret_cast<const In*>(diff + row + c);
#pragma unroll
        for (int j = 0; j < JR_PER; ++j) v[j] = in.v[j];
      } else {
#pragma unroll
        for (int j = 0; j < JR_PER; ++j) v[j] = c + j < x ? diff[row + c + j] : 0u;
      }
      if (c == 0) v[0] = 0u;                 // (the row's first sample is `first`, not a sum along the row)
#pragma unroll
      for (int j = 1; j < JR_PER; ++j) v[j] += v[j - 1];
      uint32_t sum;
      const uint32_t ahead = carry + block_exclusive_scan<1>(v[JR_PER - 1], scan, sum);
      if (VEC) {
        if (c < x) {
          Out o;
#pragma unroll
          for (int j = 0; j < JR_PER; ++j) o.v[j] = (W)(ahead + v[j]);
          *reinterpret_cast<Out*>(pixels + row + c) = o;
        }
      } else {
#pragma unroll
        for (int j = 0; j < JR_PER; ++j)
          if (c + j < x) pixels[row + c + j] = (W)(ahead + v[j]);
      }
      carry += sum;
    }
  }
}

namespace {

struct JpegllWorkspace { size_t diff, first, bytes; };
JpegllWorkspace jpegll_carve(long plane, int y, int z) {
  Carver c;
  JpegllWorkspace w;
  w.diff = c.take((size_t)plane * z * sizeof(uint16_t));
  w.first = c.take((size_t)y * z * sizeof(uint16_t));
  w.bytes = c.cur;
  return w;
}

template <typename W>
void jpegll_rows(const uint16_t* diff, const uint16_t* first, int x, int y, int z, void* pixels, hipStream_t stream) {
  const bool vec = x % JR_PER == 0 && (uintptr_t)pixels % (sizeof(W) * JR_PER) == 0;
  const dim3 grid((unsigned)y, (unsigned)(z < 1024 ? z : 1024));
  if (vec) MMNN_LAUNCH((jpegll_rows_kernel<W, true>), grid, dim3(JR_TPB), 0, stream, diff, first, x, y, z, static_cast<W*>(pixels));
  else MMNN_LAUNCH((jpegll_rows_kernel<W, false>), grid, dim3(JR_TPB), 0, stream, diff, first, x, y, z, static_cast<W*>(pixels));
}

constexpr StreamCall JPEGLL_CALL{"jpegll_decode", "frames", 16, "neither 8 nor 16"};

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_jpegll_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t bits_allocated) {
  if (!stream_extent_ok(x, y, z) || !stream_depth_ok(JPEGLL_CALL, bits_allocated)) {
    set_error("jpegll_workspace_bytes: extent %d x %d x %d at %d bits", x, y, z, bits_allocated);
    return -1;
  }
  return (int64_t)jpegll_carve((long)x * y, y, z).bytes;
}

int mmnn_jpegll_decode(const mmnn_jpegll_desc* d, const void* payload, const mmnn_jpegll_frame* frames, void* pixels, int32_t* status,
                       void* workspace, void* stream_) {
  if (stream_check_args(JPEGLL_CALL, d, payload, frames, pixels, status, workspace)) return 1;
  const int B = d->bits_allocated / 8;
  const long plane = (long)d->x * d->y;
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const JpegllWorkspace w = jpegll_carve(plane, d->y, d->z);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  JpegllArgs a{};
  a.payload = static_cast<const uint8_t*>(payload);
  a.payload_bytes = d->payload_bytes;
  a.frames = frames;
  a.diff = reinterpret_cast<uint16_t*>(ws + w.diff);
  a.first = reinterpret_cast<uint16_t*>(ws + w.first);
  a.status = status;
  a.x = d->x;
  a.y = d->y;
  MMNN_LAUNCH(jpegll_symbols_kernel, dim3((unsigned)d->z), dim3(JL_TPB), 0, stream, a);
  if (B == 1) jpegll_rows<uint8_t>(a.diff, a.first, d->x, d->y, d->z, pixels, stream);
  else jpegll_rows<uint16_t>(a.diff, a.first, d->x, d->y, d->z, pixels, stream);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
