// The host-side refusals that mmnn_rle_expand and mmnn_jpegll_decode share (include/mmnn_sts.h lists them under each call): every one
// happens before any launch and leaves its reason, prefixed with the call's name, in the error channel.
#pragma once
#include "common.hpp"

namespace mmnn {

// What differs between the two calls: the prefix of their messages, what they call their table of records, and the bit depths
// they take (8, 16 and, where `max_bits` is 32, 32) with the words that name them.
struct StreamCall {
  const char* fn;
  const char* table;
  int max_bits;
  const char* depths;
};

inline bool stream_extent_ok(int x, int y, int z) { return x >= 1 && y >= 1 && z >= 1 && (double)x * y * z < 2147483648.0; }
inline bool stream_depth_ok(const StreamCall& c, int bits) { return bits == 8 || bits == 16 || (bits == 32 && c.max_bits == 32); }

// 0, or 1 with the reason set.  `Desc`: mmnn_rle_desc or mmnn_jpegll_desc (x, y, z, bits_allocated, payload_bytes).
template <typename Desc>
int stream_check_args(const StreamCall& c, const Desc* d, const void* payload, const void* table, const void* pixels, const void* status,
                      const void* workspace) {
  MMNN_REQUIRE(d, "%s: null descriptor", c.fn);
  MMNN_REQUIRE(d->x >= 1 && d->y >= 1 && d->z >= 1, "%s: non-positive extent %d x %d x %d", c.fn, d->x, d->y, d->z);
  MMNN_REQUIRE(stream_extent_ok(d->x, d->y, d->z), "%s: extent %d x %d x %d holds 2^31 voxels or more", c.fn, d->x, d->y, d->z);
  MMNN_REQUIRE(stream_depth_ok(c, d->bits_allocated), "%s: bits_allocated %d is %s", c.fn, d->bits_allocated, c.depths);
  MMNN_REQUIRE(d->payload_bytes >= 1, "%s: payload_bytes %lld is not positive", c.fn, (long long)d->payload_bytes);
  MMNN_REQUIRE(payload && table && pixels && status && workspace, "%s: null argument", c.fn);
  const int B = d->bits_allocated / 8;
  MMNN_REQUIRE((uintptr_t)payload % 16 == 0, "%s: payload not aligned to 16 bytes", c.fn);
  MMNN_REQUIRE((uintptr_t)table % 8 == 0, "%s: %s not aligned to 8 bytes", c.fn, c.table);
  MMNN_REQUIRE((uintptr_t)pixels % B == 0, "%s: pixels not aligned to its element size", c.fn);
  MMNN_REQUIRE((uintptr_t)status % 4 == 0, "%s: status not aligned to 4 bytes", c.fn);
  MMNN_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace not aligned to 16 bytes", c.fn);
  const uintptr_t p0 = (uintptr_t)payload, p1 = p0 + (size_t)d->payload_bytes;
  const uintptr_t o0 = (uintptr_t)pixels, o1 = o0 + (size_t)d->x * d->y * d->z * B;
  const uintptr_t s0 = (uintptr_t)status, s1 = s0 + (size_t)d->z * sizeof(int32_t);
  MMNN_REQUIRE(p1 <= o0 || o1 <= p0, "%s: payload and pixels overlap", c.fn);
  MMNN_REQUIRE(p1 <= s0 || s1 <= p0, "%s: payload and status overlap", c.fn);
  return 0;
}

}  // namespace mmnn
