// The decode core of mmnn_rle_expand (the contract is the comment above it in include/mmnn_sts.h): what one PackBits control byte
// means, the clamps, the successor chain that pointer doubling resolves, the lookup of the run that holds an output byte, and the state
// that carries a segment from chunk to chunk.  Plain C++ over byte arrays with no HIP call: csrc/dicom_rle.hip runs it on LDS, and
// tests/rle_core_check.cpp runs it on exact-size heap buffers under the host's sanitizers.  The span clamp, the round of pointer
// doubling, the exit record and the chunk-to-chunk progress are csrc/stream_core.hpp, shared with the JPEG Lossless core; what is here
// is PackBits: the successor, what a run is, and the lookup and cursor that emit its bytes.
//
// A segment passes through a WINDOW of RLE_CHUNK + RLE_LOOK bytes.  The runs whose control byte lies in the first RLE_CHUNK bytes are
// decoded from this window; a run holds at most 1 + 128 bytes, so all of it lies inside the window (RLE_LOOK >= 129).  The next window
// starts RLE_CHUNK bytes further on, and the chain enters it where the last run of this one ended, at most 129 bytes in.
// Every position below is relative to the window's first byte; `end` is where the segment ends in those terms (it may lie far behind
// the window).  Nothing here reads `win` at or behind RLE_WINDOW, or at or behind `end`, whatever the bytes hold.
#pragma once
#include "stream_core.hpp"

namespace mmnn {

constexpr int RLE_CHUNK = 4096;              // MMNN_RLE_CHUNK
constexpr int RLE_LOOK = 144;                // look-ahead: >= 129, a multiple of 16
constexpr int RLE_WINDOW = RLE_CHUNK + RLE_LOOK;

// The run whose control byte sits at p (p < RLE_CHUNK, p < end): `out` bytes of output, `step` to the next control byte.  A literal's
// bytes are win[p + 1 ...], a repeat's value is win[p + 1].  `cut`: the run's bytes do not all lie in front of `end` -- it gives no
// output and ends the segment.  A no-op (128) is out 0, step 1.
struct RleRun { int out, step, literal, cut; };
MMNN_STREAM_HD RleRun rle_classify(const uint8_t* win, int p, int64_t end) {
  const int c = win[p];
  if (c == 128) return RleRun{0, 1, 0, 0};
  if (c < 128) return p + 2 + c > end ? RleRun{0, 0, 1, 1} : RleRun{c + 1, c + 2, 1, 0};
  return p + 2 > end ? RleRun{0, 0, 0, 1} : RleRun{257 - c, 2, 0, 0};
}

// The control bytes of a segment form a chain: each says where the next one sits.  Pointer doubling resolves it in parallel.
// rle_successor: the control byte that follows the one at p (whatever p holds, were it a control byte), or RLE_CHUNK where the chain
// leaves the chunk: the next one lies behind it, the segment ends, or the run at p is cut.
MMNN_STREAM_HD int rle_successor(const uint8_t* win, int p, int64_t end) {
  if (p >= end) return RLE_CHUNK;
  const RleRun r = rle_classify(win, p, end);
  const int j = p + r.step;
  return r.cut || j >= RLE_CHUNK || j >= end ? RLE_CHUNK : j;
}
constexpr int RLE_ROUNDS = 12;               // of chain_hop<RLE_CHUNK>: a chunk of single-byte steps
static_assert((1 << RLE_ROUNDS) >= RLE_CHUNK, "rounds of pointer doubling");
// Where the chain leaves the chunk, from its last member in it (marked, rle_successor == RLE_CHUNK): `next` is the position of the
// control byte that follows, i.e. the next window's entry + RLE_CHUNK, and `spent` says that the segment ended or a run was cut.
MMNN_STREAM_HD ChainExit rle_exit(const uint8_t* win, int p, int64_t end) {
  const RleRun r = rle_classify(win, p, end);
  return ChainExit{p + r.step, r.cut || p + r.step >= end};
}
// the chain of a window whose entry is no control byte of the segment: nothing to decode, the segment is spent
MMNN_STREAM_HD bool rle_enters(int entry, int64_t end) { return entry >= 0 && entry < RLE_CHUNK && entry < end; }

// The output length that position p adds to the chunk (0 where no chain member sits, and for a no-op or a cut run): what the workgroup
// prefix sum runs over.
MMNN_STREAM_HD uint32_t rle_length(const uint8_t* win, const uint8_t* mark, int p, int64_t end) {
  return mark[p] ? (uint32_t)rle_classify(win, p, end).out : 0u;
}

// off[p]: the exclusive prefix sum of rle_length over the chunk's positions.  The run that holds output byte o (o < the chunk's total)
// starts at the largest p with off[p] <= o: behind a run start off grows by its length, and the unmarked positions up to the next
// start repeat that sum.
MMNN_STREAM_HD int rle_locate(const uint32_t* off, uint32_t o) {
  int lo = 0, hi = RLE_CHUNK - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= o) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// A reader of consecutive output bytes: opened at the run that holds its first byte, it moves from run to run on its own.
struct RleCursor {
  int p;                                     // the run's control byte
  uint32_t first, last;                      // its output bytes are [first, last)
  int literal;
  uint8_t value;                             // of a repeat run
};
MMNN_STREAM_HD void rle_open(RleCursor& c, const uint8_t* win, const uint32_t* off, int p, int64_t end) {
  const RleRun r = rle_classify(win, p, end);
  c.p = p;
  c.first = off[p];
  c.last = c.first + (uint32_t)r.out;
  c.literal = r.literal;
  c.value = r.literal || r.cut ? 0 : win[p + 1];
}
// Output byte o of the chunk, o >= the cursor's current run's first byte and o < the chunk's total.  The clamps keep every index inside
// the chunk and the window even if that promise is broken.
MMNN_STREAM_HD uint8_t rle_byte(RleCursor& c, const uint8_t* win, const uint32_t* off, uint32_t o, int64_t end) {
  while (o >= c.last) {
    const int step = rle_classify(win, c.p, end).step;
    int p = c.p + step;
    while (p < RLE_CHUNK && p < end && win[p] == 128) ++p;
    if (step == 0 || p >= RLE_CHUNK || p >= end) break;      // (a cut run, or the chunk's or the segment's end: nothing follows)
    rle_open(c, win, off, p, end);
  }
  if (!c.literal) return c.value;
  const uint32_t at = (uint32_t)c.p + 1u + (o - c.first);
  return at < (uint32_t)RLE_WINDOW ? win[at] : 0;
}

// One (frame, plane) from chunk to chunk: the progress, and where the segment ends in the payload.  The chain enters the first window
// at the segment's first byte; the next window's position 0 is this one's RLE_CHUNK.
struct RleState : StreamProgress { int64_t seg_end; };
MMNN_STREAM_HD RleState rle_begin(StreamSpan s, int64_t plane_bytes) {
  RleState st;
  stream_begin(st, s, plane_bytes, (int)(s.off & 15));
  st.seg_end = s.off + s.len;
  return st;
}
MMNN_STREAM_HD int64_t rle_end(const RleState& st) { return st.seg_end - st.base; }
MMNN_STREAM_HD void rle_advance(RleState& st, ChainExit w, uint32_t taken) { stream_advance(st, w, taken, RLE_CHUNK, RLE_CHUNK); }

}  // namespace mmnn
