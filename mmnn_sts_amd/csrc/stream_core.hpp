// What the compressed-series decoders (csrc/rle_core.hpp, csrc/jpegll_core.hpp) share below their own syntax: the clamp of an untrusted
// span of the payload, one round of the pointer doubling that resolves a successor chain, the record of where the chain leaves a
// chunk, and the progress that carries a stream from chunk to chunk.  Plain C++ with no HIP call: the kernels run it on LDS
// (csrc/stream_window.hpp holds the workgroup side), the stand-alone host checks on exact-size heap buffers (tests/stream_check.hpp).
//
// A decoder passes its stream through a window of CHUNK + look-ahead bytes.  The positions of a chunk (bytes for RLE, bits for JPEG)
// that start something -- a run, a symbol -- form a chain: each says where the next one starts.  A syntax supplies three things: the
// SUCCESSOR of a position (as if something started there; N where the chain leaves the chunk), what the thing at a chain member IS
// (classify: its length, its output, whether it is cut), and how its output is EMITTED at the rank a prefix sum gives it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MMNN_STREAM_HD __host__ __device__ __forceinline__
#else
#define MMNN_STREAM_HD inline
#endif

namespace mmnn {

// A record's span of the device table, clamped into [0, payload_bytes): the kernels trust neither number.
struct StreamSpan { int64_t off, len; };
MMNN_STREAM_HD StreamSpan stream_clamp(int64_t off, int64_t len, int64_t payload_bytes) {
  if (off < 0) off = 0;
  if (off > payload_bytes) off = payload_bytes;
  if (len < 0) len = 0;
  if (len > payload_bytes - off) len = payload_bytes - off;
  return StreamSpan{off, len};
}

// One round of pointer doubling for position p of a chunk of N positions, in two phases with a barrier between them and behind them.
// Phase one: a marked p marks hop[p], and the value to store is read, hop[hop[p]].  Phase two: hop[p] = that value.  With
// mark[entry] = 1 and hop = the successor before round 0, after round k every chain member up to 2^(k+1) - 1 steps from the entry is
// marked and hop[p] is 2^(k+1) steps on; marks only ever land on chain members, in whatever order the positions of a round are
// visited.  ROUNDS with 2^ROUNDS >= N cover a chunk of single-position steps; the rounds can stop once hop[entry] has left the chunk.
// A hop of N (or more) means "left the chunk".
template <int N>
MMNN_STREAM_HD uint16_t chain_hop(const uint16_t* hop, uint8_t* mark, int p) {
  static_assert(N < 65536, "positions are uint16");
  const int j = hop[p];
  if (j >= N) return (uint16_t)N;
  if (mark[p]) mark[j] = 1;
  return hop[j];
}

// Where the chain leaves the chunk, from its last member in it (marked, successor == N): `next` is the position where the next thing
// starts, in this window's terms, and `spent` says that nothing follows: the stream ended or the last thing was cut.
struct ChainExit { int next, spent; };

// A stream from chunk to chunk.  `base`: payload offset of the window's first byte, a multiple of 16 (behind the first window too:
// it starts at the 16-byte boundary at or in front of the span), so the window is filled by aligned 16-byte loads; `entry`: where
// the chain enters the window; `done` of the `plane` outputs (bytes, samples) are written so far.
struct StreamProgress {
  int64_t base, done, plane;
  int entry, spent;
};
MMNN_STREAM_HD void stream_begin(StreamProgress& st, StreamSpan s, int64_t plane, int entry) {
  st.base = s.off & ~(int64_t)15;
  st.done = 0;
  st.plane = plane;
  st.entry = entry;
  st.spent = s.len <= 0;
}
MMNN_STREAM_HD bool stream_more(const StreamProgress& st) { return st.done < st.plane && !st.spent; }
// what of the chunk's `total` outputs the plane still takes: what would overfill it is clipped
MMNN_STREAM_HD uint32_t stream_take(const StreamProgress& st, uint32_t total) {
  const int64_t room = st.plane - st.done;
  return (int64_t)total < room ? total : (uint32_t)room;
}
// on to the window `chunk_bytes` further: `origin` is that window's position 0 in this window's terms
MMNN_STREAM_HD void stream_advance(StreamProgress& st, ChainExit w, uint32_t taken, int chunk_bytes, int origin) {
  st.done += taken;
  st.spent = w.spent;
  st.base += chunk_bytes;
  st.entry = w.next - origin;
}
// behind the last chunk: the plane is short (status 1, its outputs from `done` on are zeros) unless it is full
MMNN_STREAM_HD bool stream_short(const StreamProgress& st) { return st.done < st.plane; }

}  // namespace mmnn
