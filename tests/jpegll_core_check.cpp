// Stand-alone host check of csrc/jpegll_core.hpp, the positional core of mmnn_jpegll_decode: the chunk loop of jpegll_symbols_kernel
// restated serially over heap buffers of exactly the sizes the kernel's LDS arrays and device buffers have, so that the host's address
// and undefined-behaviour sanitizers see every index the core forms.  Built and run by tests/test_dicom_jpegll_cpu.py:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/jpegll_core_check.cpp -o jpegll_core_check
//   jpegll_core_check FIXTURE > RESULT
//
// FIXTURE (tests/_dicom_jpegll_ref.write_fixture), little endian: int32 count; per case int32 x, y, z, bits_allocated, int64
// payload_bytes, the z frame records of 56 bytes (int64 offset, length, int32 precision, 16 BITS, 17 HUFFVAL, 3 reserved), the payload.
// RESULT: per case the z int32 status words, then the x * y * z words.  Never loaded into Python, never run on a GPU.
#include "../mmnn_sts_amd/csrc/jpegll_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace mmnn;

struct Record {
  int64_t offset, length;
  int32_t precision;
  uint8_t bits[16], huffval[17], reserved[3];
};
static_assert(sizeof(Record) == 56, "frame record");

// one frame: what a workgroup of jpegll_symbols_kernel does, window by window; returns 1 when the frame fell short
static int decode_frame(const uint8_t* payload, int64_t payload_bytes, const Record& fr, uint16_t* diff, int64_t plane) {
  std::unique_ptr<uint8_t[]> raw(new uint8_t[JLL_WINDOW]), u(new uint8_t[JLL_UNSTUFFED]), mark(new uint8_t[JLL_BITS]);
  std::unique_ptr<uint16_t[]> hop(new uint16_t[JLL_BITS]), on(new uint16_t[JLL_BITS]);
  JllTable table;
  jll_build(table, fr.bits, fr.huffval);
  JllState st = jll_begin(jll_clamp(fr.offset, fr.length, payload_bytes), plane);
  while (jll_more(st)) {
    for (int i = 0; i < JLL_WINDOW; ++i) {
      const int64_t g = st.base + i;
      raw[i] = g < payload_bytes ? payload[g] : 0;
    }
    std::memset(u.get(), 0xFF, JLL_UNSTUFFED);
    std::memset(mark.get(), 0, JLL_BITS);
    // the judgements and their exclusive prefix sum, serially
    const int64_t pa = jll_prev_at(st);
    JllChunk c{0, 0, 0, 0};
    uint32_t before = 0;
    bool ended = false;
    for (int i = 0; i < JLL_CHUNK; ++i) {
      const uint32_t f = jll_judge(raw.get(), st, i, i == 0 && pa >= 0 ? payload[pa] : -1);
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
    // the chain by pointer doubling: a round's two phases one after the other, the positions of a phase in ascending or descending
    // order by turns (on the device they run in no particular order)
    JllExit w{st.entry, 1};
    for (int p = 0; p < JLL_BITS; ++p) hop[p] = (uint16_t)jll_successor(table, u.get(), p, c);
    if (jll_enters(st.entry, c)) {
      mark[st.entry] = 1;
      for (int k = 0; k < JLL_ROUNDS; ++k) {
        for (int i = 0; i < JLL_BITS; ++i) {
          const int p = k & 1 ? JLL_BITS - 1 - i : i;
          on[p] = jll_hop(hop.get(), mark.get(), p);
        }
        for (int p = 0; p < JLL_BITS; ++p) hop[p] = on[p];
        if (hop[st.entry] >= JLL_BITS) break;
      }
    }
    // the symbols in position order: their rank is their sample index
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
      if (st.done + total < plane) diff[st.done + total] = s.diff;
      ++total;
    }
    if (last != (jll_enters(st.entry, c) ? 1 : 0)) {
      std::fprintf(stderr, "%d last members of the chain in one chunk\n", last);
      std::abort();
    }
    jll_advance(st, w, c, jll_take(st, total));
  }
  if (!jll_short(st)) return 0;
  for (int64_t o = st.done; o < plane; ++o) diff[o] = 0;
  return 1;
}

template <typename T>
static bool take(FILE* f, T* v, size_t count) { return std::fread(v, sizeof(T), count, f) == count; }

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s FIXTURE > RESULT\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  int32_t cases = 0;
  if (!f || !take(f, &cases, 1)) {
    std::fprintf(stderr, "%s: cannot read\n", argv[1]);
    return 2;
  }
  for (int32_t n = 0; n < cases; ++n) {
    int32_t head[4];
    int64_t payload_bytes = 0;
    if (!take(f, head, 4) || !take(f, &payload_bytes, 1)) return 2;
    const int x = head[0], y = head[1], z = head[2], B = head[3] / 8;
    const int64_t plane = (int64_t)x * y;
    std::vector<Record> frames((size_t)z);
    std::unique_ptr<uint8_t[]> payload(new uint8_t[(size_t)payload_bytes]);          // exactly payload_bytes: one byte further is a finding
    if (!take(f, frames.data(), frames.size()) || !take(f, payload.get(), (size_t)payload_bytes)) return 2;
    std::vector<int32_t> status((size_t)z, 0);
    std::unique_ptr<uint8_t[]> pixels(new uint8_t[(size_t)(plane * z * B)]);
    for (int k = 0; k < z; ++k) {
      std::unique_ptr<uint16_t[]> diff(new uint16_t[(size_t)plane]);                  // exactly one frame of differences
      status[k] = decode_frame(payload.get(), payload_bytes, frames[k], diff.get(), plane);
      // the two prefix sums, as the kernels form them: down column 0, then along each row
      uint32_t first = 1u << (jll_precision(frames[k].precision) - 1);
      for (int j = 0; j < y; ++j) {
        first += diff[(size_t)j * x];
        uint32_t v = first;
        for (int i = 0; i < x; ++i) {
          if (i) v += diff[(size_t)j * x + i];
          uint8_t* at = pixels.get() + (size_t)(((int64_t)k * plane + (int64_t)j * x + i) * B);
          at[0] = (uint8_t)v;
          if (B == 2) at[1] = (uint8_t)(v >> 8);
        }
      }
    }
    std::fwrite(status.data(), sizeof(int32_t), status.size(), stdout);
    std::fwrite(pixels.get(), 1, (size_t)(plane * z * B), stdout);
  }
  std::fclose(f);
  return 0;
}
