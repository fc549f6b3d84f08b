// The positional core of mmnn_jpegll_decode (the contract is the comment above it in include/mmnn_sts.h): which bytes of the
// entropy-coded data are stuffed zeros and where a marker ends it, the canonical Huffman table of T.81 Annex C, what the symbol that
// starts at a bit position means, the successor chain over bit positions that pointer doubling resolves, and the state that carries a
// frame from chunk to chunk.  Plain C++ over byte arrays with no HIP call: csrc/dicom_jpegll.hip runs it on LDS, and
// tests/jpegll_core_check.cpp runs it on exact-size heap buffers under the host's sanitizers.  The span clamp, the round of pointer
// doubling, the exit record and the chunk-to-chunk progress are csrc/stream_core.hpp, shared with the RLE core; what is here is JPEG:
// judging and unstuffing, the Huffman table, the successor and what a symbol is.
//
// A frame's data passes through a RAW window of JLL_CHUNK + JLL_LOOK bytes as the file holds them.  The first JLL_JUDGED of them are
// judged (a byte is judged with its follower in view): kept, a stuffed zero, or the end of the data.  The kept bytes are compacted into
// the UNSTUFFED array `u`, padded with FF behind the last one.  The symbols that start in the n_chunk unstuffed bytes that come from the
// window's first JLL_CHUNK raw bytes are decoded from this window: a symbol is at most 16 + 15 bits long, so it ends at most 4 unstuffed
// bytes behind the byte it starts in, and 15 judged raw bytes of look-ahead hold at least 7 unstuffed ones.  The next window starts
// JLL_CHUNK raw bytes further on and the chain enters it at the bit where the last symbol of this one ended.
// Bit positions are relative to u[0], most significant bit first.  Nothing here reads `raw` at or behind JLL_WINDOW or `u` at or behind
// JLL_UNSTUFFED, whatever the bytes hold.
#pragma once
#include "stream_core.hpp"

namespace mmnn {

constexpr int JLL_CHUNK = 1024;              // MMNN_JPEGLL_CHUNK: raw bytes per chunk
constexpr int JLL_LOOK = 16;                 // raw look-ahead, a multiple of 16
constexpr int JLL_WINDOW = JLL_CHUNK + JLL_LOOK;
constexpr int JLL_JUDGED = JLL_WINDOW - 1;
constexpr int JLL_UNSTUFFED = JLL_JUDGED + 8;          // `u`: at most JLL_JUDGED kept bytes, then FF
constexpr int JLL_BITS = 8 * JLL_CHUNK;      // bit positions of a chunk; as a successor: the chain leaves the chunk
constexpr int JLL_ROUNDS = 13;               // of chain_hop<JLL_BITS>: a chunk of one-bit symbols
static_assert((1 << JLL_ROUNDS) >= JLL_BITS && JLL_BITS < 65536, "rounds of pointer doubling over uint16 positions");
static_assert((JLL_LOOK - 1) / 2 >= 4 && JLL_CHUNK + 4 < JLL_UNSTUFFED, "look-ahead of a symbol");

MMNN_STREAM_HD int jll_precision(int p) { return p < 2 ? 2 : p > 16 ? 16 : p; }

// The canonical code of BITS / HUFFVAL (T.81 Annex C) in the form a 16-bit peek w is decoded by: lim[l] is the first code that is
// NOT of length <= l, left-justified in 16 bits, so the code's length is the smallest l with w < lim[l] (none: w matches no code) and
// its value is val[base[l] + (w >> (16 - l))].  The counts are clamped so that they sum to at most 17: with lim[l - 1] <= w < lim[l]
// the index lies in 0..16 whatever BITS holds (an over-subscribed table only makes lim exceed 2^16, in 32 bits).
struct JllTable {
  uint32_t lim[17];
  int32_t base[17];
  uint8_t val[17];
};
MMNN_STREAM_HD void jll_build(JllTable& t, const uint8_t* bits, const uint8_t* huffval) {
  uint32_t code = 0;
  int n = 0;
  t.lim[0] = 0;
  t.base[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    int c = bits[l - 1];
    if (c > 17 - n) c = 17 - n;
    t.base[l] = n - (int32_t)code;
    code += (uint32_t)c;
    n += c;
    t.lim[l] = code << (16 - l);
    code <<= 1;
  }
  for (int i = 0; i < 17; ++i) t.val[i] = huffval[i];
}

// ---- the raw window -> the unstuffed bytes ---------------------------------------------------------------------------------------------
// One frame from chunk to chunk: the progress (`entry`: the bit of `u` where the chain enters; `done`: samples decoded so far), and
// the data, payload[lo, hi).
struct JllState : StreamProgress { int64_t lo, hi; };
MMNN_STREAM_HD JllState jll_begin(StreamSpan s, int64_t plane) {
  JllState st;
  stream_begin(st, s, plane, 0);
  st.lo = s.off;
  st.hi = s.off + s.len;
  return st;
}
MMNN_STREAM_HD bool jll_in(const JllState& st, int i) { return st.base + i >= st.lo && st.base + i < st.hi; }
// the payload offset of the raw byte in front of the window, or -1 when the data does not hold it (read by the caller: `prev`)
MMNN_STREAM_HD int64_t jll_prev_at(const JllState& st) { return st.base - 1 >= st.lo && st.base - 1 < st.hi ? st.base - 1 : -1; }

// What raw byte i (i < JLL_JUDGED) is: JLL_KEEP, a byte of the unstuffed data; JLL_END, the data ends in front of it (an FF that no 00
// follows, or the first byte behind payload[lo, hi)); 0, a stuffed zero, or a byte outside the data.  Only the bytes in front of the
// first JLL_END count.  `prev`: the raw byte in front of the window, -1 for none.
constexpr uint32_t JLL_KEEP = 1u, JLL_END = 1u << 16;
MMNN_STREAM_HD uint32_t jll_judge(const uint8_t* raw, const JllState& st, int i, int prev) {
  if (!jll_in(st, i)) return st.base + i == st.hi ? JLL_END : 0u;
  const int c = raw[i];
  if (c == 0xFF) return jll_in(st, i + 1) && raw[i + 1] == 0 ? JLL_KEEP : JLL_END;
  if (c == 0) {
    const int before = i > 0 ? (jll_in(st, i - 1) ? raw[i - 1] : -1) : prev;
    if (before == 0xFF) return 0u;
  }
  return JLL_KEEP;
}
// What the judged bytes of a window amount to.  n_chunk: unstuffed bytes from the chunk's own raw bytes -- the symbols that start in
// them belong to this window; n_all: with those of the look-ahead; ended: the data ends inside the judged window, at bit 8 * n_all;
// last: it ends inside the chunk's own bytes, so no window follows.
struct JllChunk { int n_chunk, n_all, ended, last; };
// The chunk's own bytes in terms of the exclusive prefix sum of jll_judge over i < JLL_CHUNK: `first_end`, whether an END lies among
// them, and `kept`, the KEEPs in front of it (without one: all of them).
MMNN_STREAM_HD JllChunk jll_chunk(bool first_end, int kept) { return JllChunk{kept, kept, first_end, first_end}; }
// The look-ahead, serially (15 bytes), for a chunk whose own bytes hold no END: its kept bytes go behind the chunk's in `u`.
MMNN_STREAM_HD void jll_look(const uint8_t* raw, const JllState& st, uint8_t* u, JllChunk& c) {
  for (int i = JLL_CHUNK; i < JLL_JUDGED; ++i) {
    const uint32_t f = jll_judge(raw, st, i, -1);
    if (f == JLL_END) {
      c.ended = 1;
      return;
    }
    if (f == JLL_KEEP && c.n_all < JLL_UNSTUFFED) u[c.n_all++] = raw[i];
  }
}
MMNN_STREAM_HD int64_t jll_endbits(const JllChunk& c) { return c.ended ? 8 * (int64_t)c.n_all : (int64_t)1 << 40; }

// ---- a symbol --------------------------------------------------------------------------------------------------------------------------
// The symbol that starts at bit p (p < 8 * n_chunk <= JLL_BITS): `len` bits of code and extra bits, and the difference modulo 2^16.
// `cut`: its 16 bits (FF-padded behind the data) match no code, its value exceeds 16, or it does not end in front of the data's end:
// it gives no output and ends the frame.  Reads u[p / 8 .. p / 8 + 4].
struct JllSym { int len, cut; uint16_t diff; };
MMNN_STREAM_HD JllSym jll_classify(const JllTable& t, const uint8_t* u, int p, int64_t endbits) {
  const int b = p >> 3, o = p & 7;
  const uint64_t v = (uint64_t)u[b] << 32 | (uint64_t)u[b + 1] << 24 | (uint64_t)u[b + 2] << 16 | (uint64_t)u[b + 3] << 8 | (uint64_t)u[b + 4];
  const uint32_t w = (uint32_t)(v >> (24 - o)) & 0xFFFFu;
  int l = 1;
  while (l <= 16 && w >= t.lim[l]) ++l;
  if (l > 16) return JllSym{0, 1, 0};
  int at = t.base[l] + (int)(w >> (16 - l));
  at = at < 0 ? 0 : at > 16 ? 16 : at;       // (in 0..16 by construction)
  const int s = t.val[at];
  if (s > 16) return JllSym{0, 1, 0};
  const int extra = s < 16 ? s : 0, len = l + extra;
  if (p + len > endbits) return JllSym{0, 1, 0};
  const uint32_t e = extra ? (uint32_t)(v >> (40 - o - len)) & ((1u << extra) - 1u) : 0u;
  const uint32_t d = s == 0 ? 0u : s == 16 ? 32768u : e >= (1u << (s - 1)) ? e : e - (1u << s) + 1u;
  return JllSym{len, 0, (uint16_t)d};
}

// ---- the chain -------------------------------------------------------------------------------------------------------------------------
// The symbols of a frame form a chain: each says where the next one starts.  jll_successor: the bit where the symbol behind the one at p
// starts (whatever p holds, were a symbol to start there), or JLL_BITS where the chain leaves the chunk: the next one starts in the next
// window's bytes, or the symbol at p is cut.
MMNN_STREAM_HD int jll_successor(const JllTable& t, const uint8_t* u, int p, const JllChunk& c) {
  if (p >= 8 * c.n_chunk) return JLL_BITS;
  const JllSym s = jll_classify(t, u, p, jll_endbits(c));
  const int j = p + s.len;
  return s.cut || j >= 8 * c.n_chunk ? JLL_BITS : j;
}
MMNN_STREAM_HD bool jll_enters(int entry, const JllChunk& c) { return entry >= 0 && entry < 8 * c.n_chunk; }
// Where the chain leaves the chunk, from its last member in it (marked, jll_successor == JLL_BITS): `next` is the bit where the next
// symbol starts, and `spent` says that a symbol was cut or the data ended in this chunk's own bytes: nothing follows.
MMNN_STREAM_HD ChainExit jll_exit(const JllSym& s, int p, const JllChunk& c) { return ChainExit{p + s.len, s.cut || c.last}; }
MMNN_STREAM_HD bool jll_leaves(const JllSym& s, int p, const JllChunk& c) { return s.cut || p + s.len >= 8 * c.n_chunk; }

// the next window's bit 0 is this one's bit 8 * n_chunk
MMNN_STREAM_HD void jll_advance(JllState& st, ChainExit w, const JllChunk& c, uint32_t taken) { stream_advance(st, w, taken, JLL_CHUNK, 8 * c.n_chunk); }

}  // namespace mmnn
