// Stand-alone host check of csrc/rle_core.hpp, the decode core of mmnn_rle_expand: the chunk loop of rle_planes_kernel restated
// serially over heap buffers of exactly the sizes the kernel's LDS arrays and device buffers have, so that the host's address and
// undefined-behaviour sanitizers see every index the core forms.  Built and run by tests/test_dicom_rle_cpu.py:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/rle_core_check.cpp -o rle_core_check
//   rle_core_check FIXTURE > RESULT
//
// FIXTURE (tests/_dicom_rle_ref.write_fixture), little endian: int32 count; per case int32 x, y, z, bits, int64 payload_bytes, the
// z * B * 2 int64 of the segment table (offset into the payload, length), the payload.  RESULT: per case the z int32 status words, then
// the x * y * z words.  Never loaded into Python, never run on a GPU.
#include "../mmnn_sts_amd/csrc/rle_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace mmnn;

// one (frame, plane): what a workgroup of rle_planes_kernel does, window by window; returns 1 when the plane fell short
static int expand_plane(const uint8_t* payload, int64_t payload_bytes, int64_t seg_off, int64_t seg_len, uint8_t* dst, int64_t plane) {
  std::unique_ptr<uint8_t[]> win(new uint8_t[RLE_WINDOW]), mark(new uint8_t[RLE_CHUNK]);
  std::unique_ptr<uint32_t[]> off(new uint32_t[RLE_CHUNK]);
  std::unique_ptr<uint16_t[]> hop(new uint16_t[RLE_CHUNK]), on(new uint16_t[RLE_CHUNK]);
  RleState st = rle_begin(rle_clamp(seg_off, seg_len, payload_bytes), plane);
  while (rle_more(st)) {
    for (int i = 0; i < RLE_WINDOW; ++i) {
      const int64_t g = st.base + i;
      win[i] = g < payload_bytes ? payload[g] : 0;
    }
    std::memset(mark.get(), 0, RLE_CHUNK);
    const int64_t end = rle_end(st);
    // the chain by pointer doubling: a round's two phases one after the other, the positions of a phase in ascending or descending
    // order by turns (on the device they run in no particular order)
    RleExit w{st.entry, 1};
    for (int p = 0; p < RLE_CHUNK; ++p) hop[p] = (uint16_t)rle_successor(win.get(), p, end);
    if (rle_enters(st.entry, end)) {
      mark[st.entry] = 1;
      for (int k = 0; k < RLE_ROUNDS; ++k) {
        for (int i = 0; i < RLE_CHUNK; ++i) {
          const int p = k & 1 ? RLE_CHUNK - 1 - i : i;
          on[p] = rle_hop(hop.get(), mark.get(), p);
        }
        for (int p = 0; p < RLE_CHUNK; ++p) hop[p] = on[p];
        if (hop[st.entry] >= RLE_CHUNK) break;
      }
      int last = 0;
      for (int p = 0; p < RLE_CHUNK; ++p)
        if (mark[p] && rle_successor(win.get(), p, end) == RLE_CHUNK) {
          w = rle_exit(win.get(), p, end);
          ++last;
        }
      if (last != 1) {
        std::fprintf(stderr, "%d last members of the chain in one chunk\n", last);
        std::abort();
      }
    }
    uint32_t total = 0;
    for (int p = 0; p < RLE_CHUNK; ++p) {
      off[p] = total;
      total += rle_length(win.get(), mark.get(), p, end);
    }
    const uint32_t n = rle_take(st, total);
    uint8_t* d = dst + st.done;
    const uint32_t lead = (uint32_t)(st.done & 15);            // cells of 16 bytes with a ragged first and last one, as on the device
    const uint32_t cells = (lead + n + 15u) / 16u;
    for (uint32_t g = 0; g < cells; ++g) {
      const long lo = 16l * g - lead;
      const uint32_t o0 = lo < 0 ? 0u : (uint32_t)lo;
      const uint32_t o1 = lo + 16 < (long)n ? (uint32_t)(lo + 16) : n;
      RleCursor c;
      rle_open(c, win.get(), off.get(), rle_locate(off.get(), o0), end);
      for (uint32_t o = o0; o < o1; ++o) d[o] = rle_byte(c, win.get(), off.get(), o, end);
    }
    rle_advance(st, w, n);
  }
  if (!rle_short(st)) return 0;
  for (int64_t o = st.done; o < st.plane; ++o) dst[o] = 0;
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
    std::vector<int64_t> table((size_t)z * B * 2);
    std::unique_ptr<uint8_t[]> payload(new uint8_t[(size_t)payload_bytes]);          // exactly payload_bytes: one byte further is a finding
    if (!take(f, table.data(), table.size()) || !take(f, payload.get(), (size_t)payload_bytes)) return 2;
    std::vector<int32_t> status((size_t)z, 0);
    std::unique_ptr<uint8_t[]> pixels(new uint8_t[(size_t)(plane * z * B)]);
    for (int k = 0; k < z; ++k)
      for (int s = 0; s < B; ++s) {
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[(size_t)plane]);                 // exactly one plane
        const size_t at = ((size_t)k * B + s) * 2;
        status[k] |= expand_plane(payload.get(), payload_bytes, table[at], table[at + 1], bytes.get(), plane);
        for (int64_t i = 0; i < plane; ++i) pixels[(size_t)(((int64_t)k * plane + i) * B + (B - 1 - s))] = bytes[(size_t)i];
      }
    std::fwrite(status.data(), sizeof(int32_t), status.size(), stdout);
    std::fwrite(pixels.get(), 1, (size_t)(plane * z * B), stdout);
  }
  std::fclose(f);
  return 0;
}
