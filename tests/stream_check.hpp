// What the stand-alone host checks of the compressed-series cores share (tests/rle_core_check.cpp, tests/jpegll_core_check.cpp): the
// fixture reader and the case loop, the result writer, and the serial restatement of the kernels' pointer doubling
// (csrc/stream_window.hpp: chain_resolve).  Host only; built with the programs under the address and undefined-behaviour sanitizers.
//
// FIXTURE (tests/_dicom_stream_harness.write_fixture), little endian: int32 count; per case int32 x, y, z, bits_allocated, int64
// payload_bytes, the table of records, the payload.  RESULT: per case the z int32 status words, then the x * y * z words.
#pragma once
#include "../mmnn_sts_amd/csrc/stream_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace stream_check {

template <typename T>
bool take(FILE* f, T* v, size_t count) { return std::fread(v, sizeof(T), count, f) == count; }

struct Case {
  int x, y, z, B;
  int64_t plane, payload_bytes;
  const uint8_t* payload;                    // exactly payload_bytes on the heap: one byte further is a finding
};

// main(): for every case of the fixture, decode(case, its records, status[z], pixels[plane * z * B]) and the result written out.
// A case holds z * B records of type Rec when `per_plane`, else z.
template <typename Rec, typename Decode>
int run_cases(int argc, char** argv, bool per_plane, Decode decode) {
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
    Case c{head[0], head[1], head[2], head[3] / 8, (int64_t)head[0] * head[1], payload_bytes, nullptr};
    std::vector<Rec> table((size_t)c.z * (per_plane ? c.B : 1));
    std::unique_ptr<uint8_t[]> payload(new uint8_t[(size_t)payload_bytes]);
    if (!take(f, table.data(), table.size()) || !take(f, payload.get(), (size_t)payload_bytes)) return 2;
    c.payload = payload.get();
    std::vector<int32_t> status((size_t)c.z, 0);
    const size_t bytes = (size_t)(c.plane * c.z * c.B);
    std::unique_ptr<uint8_t[]> pixels(new uint8_t[bytes]);
    decode(c, table.data(), status.data(), pixels.get());
    std::fwrite(status.data(), sizeof(int32_t), status.size(), stdout);
    std::fwrite(pixels.get(), 1, bytes, stdout);
  }
  std::fclose(f);
  return 0;
}

// lds[0, WINDOW) as window_fill leaves it
template <int WINDOW>
void fill(uint8_t* win, const Case& c, int64_t base) {
  for (int i = 0; i < WINDOW; ++i) win[i] = base + i < c.payload_bytes ? c.payload[base + i] : 0;
}

// The chain by pointer doubling as chain_resolve runs it: hop = successor, the entry marked, then a round's two phases one after the
// other, the positions of a phase in ascending or descending order by turns (on the device they run in no particular order).
// `hop`, `on` and `mark` hold exactly N entries; `mark` is all zero.
template <int N, int ROUNDS, typename Successor>
void resolve(uint16_t* hop, uint16_t* on, uint8_t* mark, int entry, bool enters, Successor successor) {
  for (int p = 0; p < N; ++p) hop[p] = (uint16_t)successor(p);
  if (!enters) return;
  mark[entry] = 1;
  for (int k = 0; k < ROUNDS; ++k) {
    for (int i = 0; i < N; ++i) {
      const int p = k & 1 ? N - 1 - i : i;
      on[p] = mmnn::chain_hop<N>(hop, mark, p);
    }
    for (int p = 0; p < N; ++p) hop[p] = on[p];
    if (hop[entry] >= N) break;
  }
}

// `last`: how many marked positions said that the chain leaves the chunk behind them.  One writer of the kernels' `left` word, no more
// and no fewer, when the chain enters the chunk; none when it does not.
inline void one_exit(int last, bool enters) {
  if (last == (enters ? 1 : 0)) return;
  std::fprintf(stderr, "%d last members of the chain in one chunk\n", last);
  std::abort();
}

}  // namespace stream_check
