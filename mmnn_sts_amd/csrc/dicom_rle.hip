// DICOM RLE Lossless (PS3.5 Annex G) expansion: the PackBits segments of a sorted single-frame series -> the bytes an uncompressed
// series would hold, which mmnn_decode_slices then takes unchanged (the contract is the comment above mmnn_rle_expand in
// include/mmnn_sts.h; what a control byte means, the clamps and the chunk-to-chunk state are csrc/rle_core.hpp, which a host program
// runs under the sanitizers).  What it shares with csrc/dicom_jpegll.hip is stated once: the window fill and the doubling rounds with
// their barriers in csrc/stream_window.hpp, the span clamp and the progress in csrc/stream_core.hpp, the host-side refusals in
// csrc/stream_args.hpp.
//
//   rle_planes_kernel      grid (z * B), block 1024: one workgroup per (frame, byte plane), B = bits_allocated / 8.  The segment passes
//                          through LDS in windows of RLE_CHUNK + RLE_LOOK bytes, filled by aligned 16-byte loads (the ragged end of
//                          the payload by bytes).  Per window:
//                            1. every position gets its successor, as if it held a control byte, and pointer doubling from the
//                               window's known entry point marks the positions that do: at most 12 rounds of two LDS passes, fewer
//                               when the runs are long (the rounds stop once the entry's pointer has left the chunk);
//                            2. every thread takes 4 positions, sums the output lengths of the runs that start there, and
//                               block_exclusive_scan turns the sums into off[p], the output offset of the run at p;
//                            3. all lanes expand: a thread owns 16 output bytes that share one aligned 16-byte cell of the
//                               destination, finds the run of its first byte by binary search in off[] and reads on from run to run;
//                               a whole cell is one 16-byte store, the ragged cells at either end of the window's output are byte
//                               stores.  Every output byte is written once; no atomics.
//                          16 waves, because every step is a chain of dependent LDS reads: the waves hide each other's latency.
//                          A plane that its segment does not fill is zero from there on and its status word is 1.  With B = 1 the plane
//                          IS the frame and the kernel writes `pixels` and `status` itself.
//   rle_interleave_kernel  B > 1: the B planes of a word, which the first kernel left in the workspace (plane starts padded to 16
//                          bytes), meet here: a thread reads 16 / B bytes of each plane and stores 16 bytes of whole words; element
//                          loads and stores when a frame is no multiple of 16 bytes or `pixels` is not aligned to 16.  Thread block
//                          (0, 0) also folds the planes' status words into the frames'.
#include "../../include/mmnn_sts.h"
#include "common.hpp"
#include "reduce.hpp"
#include "rle_core.hpp"
#include "stream_args.hpp"
#include "stream_window.hpp"

namespace mmnn {

constexpr int RL_WAVES = 16;
constexpr int RL_TPB = 64 * RL_WAVES;
constexpr int RL_PER = RLE_CHUNK / RL_TPB;   // positions per thread
constexpr int IL_TPB = 256;                  // of the interleave
static_assert(RLE_CHUNK == MMNN_RLE_CHUNK && RL_PER == 4 && RLE_LOOK >= 129 && RLE_LOOK % 16 == 0, "window geometry");

struct RleArgs {
  const uint8_t* payload;
  long payload_bytes;
  const int64_t* segments;                   // [z * B][2]
  uint8_t* planes;                           // where plane fp starts: planes + fp * stride
  long stride;
  long plane;                                // x * y
  int32_t* pstatus;                          // [z * B]
};

__global__ void __launch_bounds__(RL_TPB) rle_planes_kernel(const RleArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t win[RLE_WINDOW];
  __shared__ __attribute__((aligned(16))) uint8_t mark[RLE_CHUNK];
  __shared__ __attribute__((aligned(16))) uint32_t off[RLE_CHUNK];
  __shared__ uint16_t hop[RLE_CHUNK];
  __shared__ uint32_t scan[RL_WAVES];
  __shared__ ChainExit left;
  const int tid = threadIdx.x;
  const long fp = blockIdx.x;
  uint8_t* dst = a.planes + fp * a.stride;
  RleState st = rle_begin(stream_clamp(a.segments[2 * fp], a.segments[2 * fp + 1], a.payload_bytes), a.plane);   // the same in every thread
  while (stream_more(st)) {
    window_fill<RLE_WINDOW, RL_TPB>(win, a.payload, a.payload_bytes, st.base, tid);
    reinterpret_cast<uint32_t*>(mark)[tid] = 0u;
    __syncthreads();
    const long end = rle_end(st);
    // 1. the chain; `left` has one writer in front of chain_resolve's barriers (thread 0) and one behind them (the chain's last member)
    if (tid == 0) left = ChainExit{st.entry, 1};
    chain_resolve<RLE_CHUNK, RL_TPB, RLE_ROUNDS>(hop, mark, st.entry, rle_enters(st.entry, end), tid,
                                                 [&](int p) { return rle_successor(win, p, end); });
    // the chain's last member in the chunk says where the next window is entered
#pragma unroll
    for (int i = 0; i < RL_PER; ++i) {
      const int p = i * RL_TPB + tid;
      if (mark[p] && rle_successor(win, p, end) == RLE_CHUNK) left = rle_exit(win, p, end);
    }
    // 2. the output offset of every run
    uint32_t len[RL_PER], sum = 0u;
#pragma unroll
    for (int i = 0; i < RL_PER; ++i) {
      len[i] = rle_length(win, mark, tid * RL_PER + i, end);
      sum += len[i];
    }
    uint32_t total;
    uint32_t at = block_exclusive_scan<RL_WAVES>(sum, scan, total);
    uint4 q;
    q.x = at; at += len[0];
    q.y = at; at += len[1];
    q.z = at; at += len[2];
    q.w = at;
    *reinterpret_cast<uint4*>(off + tid * RL_PER) = q;
    __syncthreads();
    // 3. the expansion
    const ChainExit w = left;
    const uint32_t n = stream_take(st, total);
    uint8_t* d = dst + st.done;
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(d) & 15);
    const uint32_t cells = (lead + n + 15u) / 16u;
    for (uint32_t g = tid; g < cells; g += RL_TPB) {
      const long lo = 16l * g - lead;        // the output byte at the cell's first address (in front of the output for a ragged cell 0)
      const uint32_t o0 = lo < 0 ? 0u : (uint32_t)lo;
      const uint32_t o1 = lo + 16 < (long)n ? (uint32_t)(lo + 16) : n;
      RleCursor c;
      rle_open(c, win, off, rle_locate(off, o0), end);
      if (o1 - o0 == 16u) {
        unsigned q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 16; ++i) q[i >> 2] |= (unsigned)rle_byte(c, win, off, o0 + i, end) << (8 * (i & 3));
        *reinterpret_cast<uint4*>(d + lo) = make_uint4(q[0], q[1], q[2], q[3]);
      } else {
        for (uint32_t o = o0; o < o1; ++o) d[o] = rle_byte(c, win, off, o, end);
      }
    }
    rle_advance(st, w, n);
    __syncthreads();                         // the next window overwrites win, mark, hop, off and left
  }
  const bool failed = stream_short(st);
  if (failed)
    for (long o = st.done + tid; o < st.plane; o += RL_TPB) dst[o] = 0;
  if (tid == 0) a.pstatus[fp] = failed ? 1 : 0;
}

// WORDS words of B bytes per thread: WORDS bytes of each plane in, WORDS * B bytes out.  Plane s holds byte B - 1 - s of the word.
template <int B, int WORDS>
__global__ void __launch_bounds__(IL_TPB) rle_interleave_kernel(const uint8_t* planes, long stride, long plane, int z, uint8_t* pixels,
                                                                const int32_t* pstatus, int32_t* status) {
  struct alignas(WORDS) In { uint8_t b[WORDS]; };
  struct alignas(WORDS * B) Out { uint8_t b[WORDS * B]; };
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    for (int k = threadIdx.x; k < z; k += IL_TPB) {
      int bad = 0;
#pragma unroll
      for (int s = 0; s < B; ++s) bad |= pstatus[(long)k * B + s];
      status[k] = bad ? 1 : 0;
    }
  }
  const long i0 = ((long)blockIdx.x * IL_TPB + threadIdx.x) * WORDS;
  if (i0 >= plane) return;                   // WORDS > 1 only when plane % WORDS == 0: a group is inside or outside as a whole
  for (int k = blockIdx.y; k < z; k += gridDim.y) {
    Out o;
#pragma unroll
    for (int s = 0; s < B; ++s) {
      const In in = *reinterpret_cast<const In*>(planes + ((long)k * B + s) * stride + i0);
#pragma unroll
      for (int j = 0; j < WORDS; ++j) o.b[j * B + (B - 1 - s)] = in.b[j];
    }
    *reinterpret_cast<Out*>(pixels + ((long)k * plane + i0) * B) = o;
  }
}

namespace {

long rle_plane_stride(long plane) { return (plane + 15) / 16 * 16; }

struct RleWorkspace { size_t planes, pstatus, bytes; };
RleWorkspace rle_carve(long plane, int z, int B) {
  Carver c;
  RleWorkspace w;
  w.planes = c.take(B > 1 ? (size_t)rle_plane_stride(plane) * z * B : 0);
  w.pstatus = c.take((size_t)z * B * sizeof(int32_t));
  w.bytes = c.cur;
  return w;
}

template <int B>
void rle_interleave(const uint8_t* planes, long stride, long plane, int z, uint8_t* pixels, const int32_t* pstatus, int32_t* status,
                    hipStream_t stream) {
  constexpr int WORDS = 16 / B;
  const bool vec = plane % WORDS == 0 && (plane * B) % 16 == 0 && (uintptr_t)pixels % 16 == 0;
  const int gx = cdiv(plane, (long)IL_TPB * (vec ? WORDS : 1));
  const int gy = z < 1024 ? z : 1024;
  if (vec) MMNN_LAUNCH((rle_interleave_kernel<B, WORDS>), dim3(gx, gy), dim3(IL_TPB), 0, stream, planes, stride, plane, z, pixels, pstatus, status);
  else MMNN_LAUNCH((rle_interleave_kernel<B, 1>), dim3(gx, gy), dim3(IL_TPB), 0, stream, planes, stride, plane, z, pixels, pstatus, status);
}

constexpr StreamCall RLE_CALL{"rle_expand", "segments", 32, "none of 8, 16, 32"};

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_rle_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t bits_allocated) {
  if (!stream_extent_ok(x, y, z) || !stream_depth_ok(RLE_CALL, bits_allocated)) {
    set_error("rle_workspace_bytes: extent %d x %d x %d at %d bits", x, y, z, bits_allocated);
    return -1;
  }
  return (int64_t)rle_carve((long)x * y, z, bits_allocated / 8).bytes;
}

int mmnn_rle_expand(const mmnn_rle_desc* d, const void* payload, const int64_t* segments, void* pixels, int32_t* status, void* workspace,
                    void* stream_) {
  if (stream_check_args(RLE_CALL, d, payload, segments, pixels, status, workspace)) return 1;
  const int B = d->bits_allocated / 8;
  const long plane = (long)d->x * d->y;
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const RleWorkspace w = rle_carve(plane, d->z, B);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  RleArgs a{};
  a.payload = static_cast<const uint8_t*>(payload);
  a.payload_bytes = d->payload_bytes;
  a.segments = segments;
  a.plane = plane;
  if (B == 1) {
    a.planes = static_cast<uint8_t*>(pixels); a.stride = plane; a.pstatus = status;
  } else {
    a.planes = ws + w.planes; a.stride = rle_plane_stride(plane); a.pstatus = reinterpret_cast<int32_t*>(ws + w.pstatus);
  }
  MMNN_LAUNCH(rle_planes_kernel, dim3((unsigned)(d->z * B)), dim3(RL_TPB), 0, stream, a);
  if (B == 2) rle_interleave<2>(a.planes, a.stride, plane, d->z, static_cast<uint8_t*>(pixels), a.pstatus, status, stream);
  if (B == 4) rle_interleave<4>(a.planes, a.stride, plane, d->z, static_cast<uint8_t*>(pixels), a.pstatus, status, stream);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
