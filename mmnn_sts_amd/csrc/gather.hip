// Rows of a device table -> a contiguous batch (the contract is the comment above mmnn_gather_rows in include/mmnn_sts.h).  What the
// volume cache (mmnn_sts_amd/data/cache.py) assembles a batch with: a streaming copy, bound by its loads and stores.
//
//   gather_rows_kernel<T>  blockIdx.y = output row i, whose source row slots[i] is read from the kernel arguments (the slots travel by
//                          value: the host has checked them, and no index buffer is uploaded).  blockIdx.x walks the row in chunks
//                          of GR_TPB * GR_UNROLL units of T (u32x4: 16 bytes, or unsigned: 4), grid-strided when a row has more
//                          chunks than the grid's x extent, which the host caps so that n * gridDim.x stays near 2048 workgroups.
//                          A lane issues its GR_UNROLL loads (a wave reads 1 KiB without a gap per load when T is u32x4) before its
//                          first store.  Every offset is 64-bit.  No LDS, no atomics; bits are copied, never interpreted.
//                          The loads are non-temporal and the stores plain: a row is read once per epoch out of a table larger than
//                          the last-level cache, and the batch is read next by the model.  Measured with tools/cache_time.py, the
//                          builds alternating three times in one session: the planes of a (2, 2, 128^3) batch take 12.86-12.87 us
//                          against 13.17-13.21 us with plain loads (2.4 %); non-temporal stores change nothing (13.17-13.20 us
//                          alone, 12.89-12.90 us beside the loads).
#include "../../include/mmnn_sts.h"
#include "common.hpp"

namespace mmnn {

constexpr int GR_TPB = 256;
constexpr int GR_UNROLL = 4;
constexpr int GR_MAX_BLOCKS = 2048;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // (a native vector: an array of HIP's uint4 struct is parked in LDS)

struct GrArgs {
  const char* table;
  char* out;
  long row_bytes;
  long units;                               // row_bytes / sizeof(T)
  int slots[MMNN_GATHER_MAX_ROWS];
};

template <typename T>
__global__ void __launch_bounds__(GR_TPB) gather_rows_kernel(const GrArgs a) {
  const T* src = reinterpret_cast<const T*>(a.table + (long)a.slots[blockIdx.y] * a.row_bytes);
  T* dst = reinterpret_cast<T*>(a.out + (long)blockIdx.y * a.row_bytes);
  constexpr long CHUNK = (long)GR_TPB * GR_UNROLL;
  for (long u0 = (long)blockIdx.x * CHUNK + threadIdx.x; u0 < a.units; u0 += (long)gridDim.x * CHUNK) {
    T v[GR_UNROLL];                         // loads past the row's end re-read its last unit: unconditional, so v stays in registers
#pragma unroll
    for (int k = 0; k < GR_UNROLL; ++k) {
      const long u = u0 + (long)k * GR_TPB;
      v[k] = __builtin_nontemporal_load(&src[u < a.units ? u : a.units - 1]);
    }
#pragma unroll
    for (int k = 0; k < GR_UNROLL; ++k) {
      const long u = u0 + (long)k * GR_TPB;
      if (u < a.units) dst[u] = v[k];
    }
  }
}

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int mmnn_gather_rows(const void* table, int64_t n_rows, int64_t row_bytes, const int32_t* slots, int32_t n, void* out, void* stream_) {
  MMNN_REQUIRE(table, "gather_rows: table is null");
  MMNN_REQUIRE(slots, "gather_rows: slots is null");
  MMNN_REQUIRE(out, "gather_rows: out is null");
  MMNN_REQUIRE(n_rows >= 1, "gather_rows: n_rows %lld below 1", (long long)n_rows);
  MMNN_REQUIRE(row_bytes >= 4 && row_bytes % 4 == 0, "gather_rows: row_bytes %lld is not a positive multiple of 4", (long long)row_bytes);
  MMNN_REQUIRE(n_rows <= INT64_MAX / row_bytes, "gather_rows: n_rows %lld of row_bytes %lld exceed 2^63 bytes", (long long)n_rows, (long long)row_bytes);
  MMNN_REQUIRE(n >= 1 && n <= MMNN_GATHER_MAX_ROWS, "gather_rows: n %d outside 1..%d", n, MMNN_GATHER_MAX_ROWS);
  for (int i = 0; i < n; ++i)
    MMNN_REQUIRE(slots[i] >= 0 && slots[i] < n_rows, "gather_rows: slots[%d] = %d outside 0..%lld", i, slots[i], (long long)(n_rows - 1));
  const uintptr_t t0 = (uintptr_t)table, o0 = (uintptr_t)out;
  MMNN_REQUIRE(t0 % 4 == 0, "gather_rows: table not aligned to 4 bytes");
  MMNN_REQUIRE(o0 % 4 == 0, "gather_rows: out not aligned to 4 bytes");
  const uintptr_t t1 = t0 + (uintptr_t)n_rows * (uintptr_t)row_bytes, o1 = o0 + (uintptr_t)n * (uintptr_t)row_bytes;
  MMNN_REQUIRE(t1 <= o0 || o1 <= t0, "gather_rows: out overlaps the table");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  GrArgs a{};
  a.table = static_cast<const char*>(table);
  a.out = static_cast<char*>(out);
  a.row_bytes = row_bytes;
  for (int i = 0; i < n; ++i) a.slots[i] = slots[i];
  const bool wide = row_bytes % 16 == 0 && t0 % 16 == 0 && o0 % 16 == 0;
  a.units = row_bytes / (wide ? 16 : 4);
  const long chunks = (a.units + (long)GR_TPB * GR_UNROLL - 1) / ((long)GR_TPB * GR_UNROLL);
  const long cap = GR_MAX_BLOCKS / n > 1 ? GR_MAX_BLOCKS / n : 1;
  const dim3 grid((unsigned)(chunks < cap ? chunks : cap), (unsigned)n);
  if (wide)
    MMNN_LAUNCH(gather_rows_kernel<u32x4>, grid, dim3(GR_TPB), 0, stream, a);
  else
    MMNN_LAUNCH(gather_rows_kernel<unsigned>, grid, dim3(GR_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
