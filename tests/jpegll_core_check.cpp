// Stand-alone host check of csrc/jpegll_core.hpp, the positional core of mmnn_jpegll_decode: the chunk loop of jpegll_symbols_kernel
// restated serially over heap buffers of exactly the sizes the kernel's LDS arrays and device buffers have, so that the host's address
// and undefined-behaviour sanitizers see every index the core forms.  Built and run by tests/test_dicom_jpegll_cpu.py:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/jpegll_core_check.cpp -o jpegll_core_check
//   jpegll_core_check FIXTURE > RESULT
//
// FIXTURE and RESULT: tests/stream_check.hpp; a case's records are the z frame records of 56 bytes (int64 offset, length, int32
// precision, 16 BITS, 17 HUFFVAL, 3 reserved).  Never loaded into Python, never run on a GPU.
#include "../mmnn_sts_amd/csrc/jpegll_core.hpp"
#include "stream_check.hpp"

using namespace mmnn;
using stream_check::Case;

struct Record {
  int64_t offset, length;
  int32_t precision;
  uint8_t bits[16], huffval[17], reserved[3];
};
static_assert(sizeof(Record) == 56, "frame record");

// one frame: what a workgroup of jpegll_symbols_kernel does, window by window; returns 1 when the frame fell short
static int decode_frame(const Case& cs, const Record& fr, uint16_t* diff) {
  std::unique_ptr<uint8_t[]> raw(new uint8_t[JLL_WINDOW]), u(new uint8_t[JLL_UNSTUFFED]), mark(new uint8_t[JLL_BITS]);
  std::unique_ptr<uint16_t[]> hop(new uint16_t[JLL_BITS]), on(new uint16_t[JLL_BITS]);
  JllTable table;
  jll_build(table, fr.bits, fr.huffval);
  JllState st = jll_begin(stream_clamp(fr.offset, fr.length, cs.payload_bytes), cs.plane);
  while (stream_more(st)) {
    stream_check::fill<JLL_WINDOW>(raw.get(), cs, st.base);
    std::memset(u.get(), 0xFF, JLL_UNSTUFFED);
    std::memset(mark.get(), 0, JLL_BITS);
    // the judgements and their exclusive prefix sum, serially
    const int64_t pa = jll_prev_at(st);
    JllChunk c{0, 0, 0, 0};
    uint32_t before = 0;
    bool ended = false;
    for (int i = 0; i < JLL_CHUNK; ++i) {
      const uint32_t f = jll_judge(raw.get(), st, i, i == 0 && pa >= 0 ? cs.payload[pa] : -1);
      const bool live = before < JLL_END;
      if (live && f == JLL_KEEP) u[before & 0xFFFFu] = raw[i];
      if (live && f == JLL_END) {
        c = jll_chunk(true, (int)(before & 0xFFFFu));
        ended = true;
      }
      before += f;
    }
    if (!ended) c = jll_chunk(false, (int)(before & 0xFFFFu));
    if (!c.last) jll_look(raw.get(), st, u.get(), c);
    const bool enters = jll_enters(st.entry, c);
    stream_check::resolve<JLL_BITS, JLL_ROUNDS>(hop.get(), on.get(), mark.get(), st.entry, enters,
                                                [&](int p) { return jll_successor(table, u.get(), p, c); });
    // the symbols in position order: their rank is their sample index
    ChainExit w{st.entry, 1};
    const int64_t endbits = jll_endbits(c);
    uint32_t total = 0;
    int last = 0;
    for (int p = 0; p < JLL_BITS; ++p) {
      if (!mark[p]) continue;
      const JllSym s = jll_classify(table, u.get(), p, endbits);
      if (jll_leaves(s, p, c)) {
        w = jll_exit(s, p, c);
        ++last;
      }
      if (s.cut) continue;
      if (st.done + total < st.plane) diff[st.done + total] = s.diff;
      ++total;
    }
    stream_check::one_exit(last, enters);
    jll_advance(st, w, c, stream_take(st, total));
  }
  if (!stream_short(st)) return 0;
  for (int64_t o = st.done; o < st.plane; ++o) diff[o] = 0;
  return 1;
}

int main(int argc, char** argv) {
  return stream_check::run_cases<Record>(argc, argv, false, [](const Case& c, const Record* frames, int32_t* status, uint8_t* pixels) {
    for (int k = 0; k < c.z; ++k) {
      std::unique_ptr<uint16_t[]> diff(new uint16_t[(size_t)c.plane]);                // exactly one frame of differences
      status[k] = decode_frame(c, frames[k], diff.get());
      // the two prefix sums, as the kernels form them: down column 0, then along each row
      uint32_t first = 1u << (jll_precision(frames[k].precision) - 1);
      for (int j = 0; j < c.y; ++j) {
        first += diff[(size_t)j * c.x];
        uint32_t v = first;
        for (int i = 0; i < c.x; ++i) {
          if (i) v += diff[(size_t)j * c.x + i];
          uint8_t* at = pixels + (size_t)(((int64_t)k * c.plane + (int64_t)j * c.x + i) * c.B);
          at[0] = (uint8_t)v;
          if (c.B == 2) at[1] = (uint8_t)(v >> 8);
        }
      }
    }
  });
}
