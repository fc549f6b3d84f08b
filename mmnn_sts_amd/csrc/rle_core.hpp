// The decode core of mmnn_rle_expand (the contract is the comment above it in include/mmnn_sts.h): what one PackBits control byte
// means, the clamps, the successor chain that pointer doubling resolves, the lookup of the run that holds an output byte, and the state
// that carries a segment from chunk to chunk.  Plain C++ over byte arrays with no HIP call: csrc/dicom_rle.hip runs it on LDS, and
// tests/rle_core_check.cpp runs it on exact-size heap buffers under the host's sanitizers.
//
// A segment passes through a WINDOW of RLE_CHUNK + RLE_LOOK bytes.  The runs whose control byte lies in the first RLE_CHUNK bytes are
// decoded from this window; a run holds at most 1 + 128 bytes, so all of it lies inside the window (RLE_LOOK >= 129).  The next window
// starts RLE_CHUNK bytes further on, and the chain enters it where the last run of this one ended, at most 129 bytes in.
// Every position below is relative to the window's first byte; `end` is where the segment ends in those terms (it may lie far behind
// the window).  Nothing here reads `win` at or behind RLE_WINDOW, or at or behind `end`, whatever the bytes hold.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MMNN_RLE_HD __host__ __device__ __forceinline__
#else
#define MMNN_RLE_HD inline
#endif

namespace mmnn {

constexpr int RLE_CHUNK = 4096;              // MMNN_RLE_CHUNK
constexpr int RLE_LOOK = 144;                // look-ahead: >= 129, a multiple of 16
constexpr int RLE_WINDOW = RLE_CHUNK + RLE_LOOK;

// A segment record of the device table, clamped into [0, payload_bytes): the kernel trusts neither number.
struct RleSpan { int64_t off, len; };
MMNN_RLE_HD RleSpan rle_clamp(int64_t off, int64_t len, int64_t payload_bytes) {
  if (off < 0) off = 0;
  if (off > payload_bytes) off = payload_bytes;
  if (len < 0) len = 0;
  if (len > payload_bytes - off) len = payload_bytes - off;
  return RleSpan{off, len};
}

// The run whose control byte sits at p (p < RLE_CHUNK, p < end): `out` bytes of output, `step` to the next control byte.  A literal's
// bytes are win[p + 1 ...], a repeat's value is win[p + 1].  `cut`: the run's bytes do not all lie in front of `end` -- it gives no
// output and ends the segment.  A no-op (128) is out 0, step 1.
struct RleRun { int out, step, literal, cut; };
MMNN_RLE_HD RleRun rle_classify(const uint8_t* win, int p, int64_t end) {
  const int c = win[p];
  if (c == 128) return RleRun{0, 1, 0, 0};
  if (c < 128) return p + 2 + c > end ? RleRun{0, 0, 1, 1} : RleRun{c + 1, c + 2, 1, 0};
  return p + 2 > end ? RleRun{0, 0, 0, 1} : RleRun{257 - c, 2, 0, 0};
}

// The control bytes of a segment form a chain: each says where the next one sits.  Pointer doubling resolves it in parallel.
// rle_successor: the control byte that follows the one at p (whatever p holds, were it a control byte), or RLE_CHUNK where the chain
// leaves the chunk: the next one lies behind it, the segment ends, or the run at p is cut.
MMNN_RLE_HD int rle_successor(const uint8_t* win, int p, int64_t end) {
  if (p >= end) return RLE_CHUNK;
  const RleRun r = rle_classify(win, p, end);
  const int j = p + r.step;
  return r.cut || j >= RLE_CHUNK || j >= end ? RLE_CHUNK : j;
}
// One round for position p, in two phases with a barrier between them and behind them.  Phase one: a marked p marks hop[p], and the
// value to store is read, hop[hop[p]].  Phase two: hop[p] = that value.  With mark[entry] = 1 and hop = rle_successor before round 0,
// after round k every chain member up to 2^(k+1) - 1 steps from the entry is marked and hop[p] is 2^(k+1) steps on; marks only ever
// land on chain members, in whatever order the positions of a round are visited.  RLE_ROUNDS rounds cover a chunk of single-byte
// steps; the rounds can stop once hop[entry] has left the chunk.
constexpr int RLE_ROUNDS = 12;
static_assert((1 << RLE_ROUNDS) >= RLE_CHUNK, "rounds of pointer doubling");
MMNN_RLE_HD uint16_t rle_hop(const uint16_t* hop, uint8_t* mark, int p) {
  const int j = hop[p];
  if (j >= RLE_CHUNK) return (uint16_t)RLE_CHUNK;
  if (mark[p]) mark[j] = 1;
  return hop[j];
}
// Where the chain leaves the chunk, from its last member in it (marked, rle_successor == RLE_CHUNK): `next` is the position of the
// control byte that follows, i.e. the next window's entry + RLE_CHUNK, and `spent` says that the segment ended or a run was cut.
struct RleExit { int next, spent; };
MMNN_RLE_HD RleExit rle_exit(const uint8_t* win, int p, int64_t end) {
  const RleRun r = rle_classify(win, p, end);
  return RleExit{p + r.step, r.cut || p + r.step >= end};
}
// the chain of a window whose entry is no control byte of the segment: nothing to decode, the segment is spent
MMNN_RLE_HD bool rle_enters(int entry, int64_t end) { return entry >= 0 && entry < RLE_CHUNK && entry < end; }

// The output length that position p adds to the chunk (0 where no chain member sits, and for a no-op or a cut run): what the workgroup
// prefix sum runs over.
MMNN_RLE_HD uint32_t rle_length(const uint8_t* win, const uint8_t* mark, int p, int64_t end) {
  return mark[p] ? (uint32_t)rle_classify(win, p, end).out : 0u;
}

// off[p]: the exclusive prefix sum of rle_length over the chunk's positions.  The run that holds output byte o (o < the chunk's total)
// starts at the largest p with off[p] <= o: behind a run start off grows by its length, and the unmarked positions up to the next
// start repeat that sum.
MMNN_RLE_HD int rle_locate(const uint32_t* off, uint32_t o) {
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
MMNN_RLE_HD void rle_open(RleCursor& c, const uint8_t* win, const uint32_t* off, int p, int64_t end) {
  const RleRun r = rle_classify(win, p, end);
  c.p = p;
  c.first = off[p];
  c.last = c.first + (uint32_t)r.out;
  c.literal = r.literal;
  c.value = r.literal || r.cut ? 0 : win[p + 1];
}
// Output byte o of the chunk, o >= the cursor's current run's first byte and o < the chunk's total.  The clamps keep every index inside
// the chunk and the window even if that promise is broken.
MMNN_RLE_HD uint8_t rle_byte(RleCursor& c, const uint8_t* win, const uint32_t* off, uint32_t o, int64_t end) {
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

// One (frame, plane) from chunk to chunk.  `base`: payload offset of the window's first byte, a multiple of 16 behind the first
// window, so the window is filled by aligned 16-byte loads; `entry`: where the chain enters it; `done`: plane bytes written so far.
struct RleState {
  int64_t base, seg_end, done, plane;
  int entry, spent;
};
MMNN_RLE_HD RleState rle_begin(RleSpan s, int64_t plane_bytes) {
  RleState st;
  st.base = s.off & ~(int64_t)15;
  st.seg_end = s.off + s.len;
  st.done = 0;
  st.plane = plane_bytes;
  st.entry = (int)(s.off - st.base);
  st.spent = s.len <= 0;
  return st;
}
MMNN_RLE_HD bool rle_more(const RleState& st) { return st.done < st.plane && !st.spent; }
MMNN_RLE_HD int64_t rle_end(const RleState& st) { return st.seg_end - st.base; }
// what of the chunk's `total` output bytes the plane still takes: a run that would overfill it is clipped
MMNN_RLE_HD uint32_t rle_take(const RleState& st, uint32_t total) {
  const int64_t room = st.plane - st.done;
  return (int64_t)total < room ? total : (uint32_t)room;
}
MMNN_RLE_HD void rle_advance(RleState& st, RleExit w, uint32_t taken) {
  st.done += taken;
  st.spent = w.spent;
  st.base += RLE_CHUNK;
  st.entry = w.next - RLE_CHUNK;
}
// behind the last chunk: the plane is short (status 1, its bytes from `done` on are zeros) unless it is full
MMNN_RLE_HD bool rle_short(const RleState& st) { return st.done < st.plane; }

}  // namespace mmnn
