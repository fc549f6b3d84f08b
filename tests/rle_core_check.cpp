// Stand-alone host check of csrc/rle_core.hpp, the decode core of mmnn_rle_expand: the chunk loop of rle_planes_kernel restated
// serially over heap buffers of exactly the sizes the kernel's LDS arrays and device buffers have, so that the host's address and
// undefined-behaviour sanitizers see every index the core forms.  Built and run by tests/test_dicom_rle_cpu.py:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/rle_core_check.cpp -o rle_core_check
//   rle_core_check FIXTURE > RESULT
//
// FIXTURE and RESULT: tests/stream_check.hpp; a case's records are the z * B * 2 int64 of the segment table (offset into the payload,
// length).  Never loaded into Python, never run on a GPU.
#include "../mmnn_sts_amd/csrc/rle_core.hpp"
#include "stream_check.hpp"

using namespace mmnn;
using stream_check::Case;

struct Segment { int64_t off, len; };

// one (frame, plane): what a workgroup of rle_planes_kernel does, window by window; returns 1 when the plane fell short
static int expand_plane(const Case& c, Segment seg, uint8_t* dst) {
  std::unique_ptr<uint8_t[]> win(new uint8_t[RLE_WINDOW]), mark(new uint8_t[RLE_CHUNK]);
  std::unique_ptr<uint32_t[]> off(new uint32_t[RLE_CHUNK]);
  std::unique_ptr<uint16_t[]> hop(new uint16_t[RLE_CHUNK]), on(new uint16_t[RLE_CHUNK]);
  RleState st = rle_begin(stream_clamp(seg.off, seg.len, c.payload_bytes), c.plane);
  while (stream_more(st)) {
    stream_check::fill<RLE_WINDOW>(win.get(), c, st.base);
    std::memset(mark.get(), 0, RLE_CHUNK);
    const int64_t end = rle_end(st);
    const bool enters = rle_enters(st.entry, end);
    stream_check::resolve<RLE_CHUNK, RLE_ROUNDS>(hop.get(), on.get(), mark.get(), st.entry, enters,
                                                 [&](int p) { return rle_successor(win.get(), p, end); });
    ChainExit w{st.entry, 1};
    int last = 0;
    for (int p = 0; p < RLE_CHUNK; ++p)
      if (mark[p] && rle_successor(win.get(), p, end) == RLE_CHUNK) {
        w = rle_exit(win.get(), p, end);
        ++last;
      }
    stream_check::one_exit(last, enters);
    uint32_t total = 0;
    for (int p = 0; p < RLE_CHUNK; ++p) {
      off[p] = total;
      total += rle_length(win.get(), mark.get(), p, end);
    }
    const uint32_t n = stream_take(st, total);
    uint8_t* d = dst + st.done;
    const uint32_t lead = (uint32_t)(st.done & 15);            // cells of 16 bytes with a ragged first and last one, as on the device
    const uint32_t cells = (lead + n + 15u) / 16u;
    for (uint32_t g = 0; g < cells; ++g) {
      const long lo = 16l * g - lead;
      const uint32_t o0 = lo < 0 ? 0u : (uint32_t)lo;
      const uint32_t o1 = lo + 16 < (long)n ? (uint32_t)(lo + 16) : n;
      RleCursor cur;
      rle_open(cur, win.get(), off.get(), rle_locate(off.get(), o0), end);
      for (uint32_t o = o0; o < o1; ++o) d[o] = rle_byte(cur, win.get(), off.get(), o, end);
    }
    rle_advance(st, w, n);
  }
  if (!stream_short(st)) return 0;
  for (int64_t o = st.done; o < st.plane; ++o) dst[o] = 0;
  return 1;
}

int main(int argc, char** argv) {
  return stream_check::run_cases<Segment>(argc, argv, true, [](const Case& c, const Segment* table, int32_t* status, uint8_t* pixels) {
    for (int k = 0; k < c.z; ++k)
      for (int s = 0; s < c.B; ++s) {
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[(size_t)c.plane]);               // exactly one plane
        status[k] |= expand_plane(c, table[(size_t)k * c.B + s], bytes.get());
        for (int64_t i = 0; i < c.plane; ++i) pixels[(size_t)(((int64_t)k * c.plane + i) * c.B + (c.B - 1 - s))] = bytes[(size_t)i];
      }
  });
}
