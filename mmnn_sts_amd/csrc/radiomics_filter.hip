// The Laplacian-of-Gaussian image filter of the radiomics path: a separable 3-D FIR with caller-computed, spacing-dependent taps, fp64
// accumulation and edge replication.  The contract is the comment above mmnn_log_filter in include/mmnn_sts.h.  Everything is enqueued on
// the caller's stream; nothing is read back and the host never waits.
//
//   log_x_kernel   LF_XR rows x LF_XT outputs along x per workgroup: the rows' scaled voxels, tile plus halo, are staged in LDS as fp64
//                  with the source index clamped while staging (the tap loop has no bounds test), the taps beside them; one output per
//                  lane and row, two sums (g_x, h_x); the tap loop is outermost, so a tap is read once for the lane's 4 rows
//                                                                                                 scan -> A0, A2
//   log_col_kernel<0>  a tile of LF_CT columns along x (128 contiguous bytes of fp64) x LF_LT outputs along y, both fields staged with
//                  the clamped halo along y; lane (column, row) owns rows row, row + 16, row + 32, row + 48 and runs the taps
//                  outermost over the four; three sums each                                       A0, A2 -> B0, C
//   log_col_kernel<1>  the same tile along z; two sums, the one rounding to fp32                  B0, C -> out
//
// Order.  Every sum starts from +0.0 and runs over the taps -r .. +r ascending, product then addition (the build passes
// -ffp-contract=off), one lane per output: no reduction across lanes, no atomics, so the result depends on nothing but the contract.
// LDS.  The column tile holds 2 fields x (LF_LT + 2 r) x LF_CT fp64 = 256 (64 + 2 r) bytes and the 2 (2 r + 1) taps: 62.8 KiB at
// r = MMNN_LOG_FILTER_MAX_RADIUS = 88, inside the 64 KiB a launch gets without asking for more and two workgroups in a CU's 160 KiB.  The
// size follows the radius in use (29 KiB at r = 25).
// No scalar memory writes.
#include "ingest_load.hpp"
#include "radiomics.hpp"

#include <cmath>

namespace mmnn {

constexpr int LF_XT = RAD_TPB;              // outputs along x per workgroup of the x pass: one per lane
constexpr int LF_XR = 4;                    // rows per workgroup of the x pass
constexpr int LF_CT = 16;                   // columns (along x) of a y / z tile
constexpr int LF_LT = 64;                   // outputs along the filtered axis of a y / z tile
constexpr int LF_LANES_L = RAD_TPB / LF_CT; // lane rows of a y / z tile
constexpr int LF_MAX_R = MMNN_LOG_FILTER_MAX_RADIUS;
constexpr int LF_PER = LF_LT / LF_LANES_L;  // outputs per lane of a y / z tile
static_assert(LF_LT % LF_LANES_L == 0, "whole trips over the tile");
static_assert((size_t)(2 * (LF_LT + 2 * LF_MAX_R) * LF_CT + 2 * (2 * LF_MAX_R + 1)) * 8 <= 64 * 1024, "the column tile at the largest radius");

struct LogArgs {
  const void* scan;
  const double* taps;
  double* f[4];                             // A0, A2, B0, C: [Z][Y][X] fp64 each
  float* out;
  int X, Y, Z, code;
  IgScale sc;
  int r[3];                                 // x, y, z
  int toff[3];                              // g_a at taps + toff[a], h_a behind it
  double w[3];
};

struct LogLayout { size_t f[4], total; };

inline LogLayout log_layout(long n) {
  LogLayout L;
  Carver cv;
  for (int k = 0; k < 4; ++k) L.f[k] = cv.take((size_t)n * 8);
  L.total = cv.cur;
  return L;
}

inline size_t log_x_lds(int r) { return (size_t)(2 * (2 * r + 1) + LF_XR * (LF_XT + 2 * r)) * 8; }
inline size_t log_col_lds(int r) { return (size_t)(2 * (2 * r + 1) + 2 * (LF_LT + 2 * r) * LF_CT) * 8; }

__device__ __forceinline__ int log_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__global__ void __launch_bounds__(RAD_TPB) log_x_kernel(const LogArgs a) {
  extern __shared__ __attribute__((aligned(16))) double log_lds[];
  const int t = threadIdx.x, r = a.r[0], nt = 2 * r + 1, span = LF_XT + 2 * r;
  double* g = log_lds;
  double* h = g + nt;
  double* tile = h + nt;                    // [LF_XR][span]
  const int tiles = (a.X + LF_XT - 1) / LF_XT;
  const long rows = (long)a.Y * a.Z, row0 = (long)(blockIdx.x / tiles) * LF_XR;
  const int x0 = (int)(blockIdx.x % tiles) * LF_XT;
  const int nrow = rows - row0 < LF_XR ? (int)(rows - row0) : LF_XR;
  for (int i = t; i < 2 * nt; i += RAD_TPB) g[i] = a.taps[a.toff[0] + i];
  for (int k = 0; k < LF_XR; ++k) {          // a row past the last one is staged as the last one: computed, not stored
    const long row = row0 + (k < nrow ? k : nrow - 1);
    for (int i = t; i < span; i += RAD_TPB) {
      double v[1];
      ig_load<1>(a.scan, a.code, row * a.X + log_clamp(x0 - r + i, a.X), v);
      tile[k * span + i] = ig_scaled(v[0], a.sc);
    }
  }
  __syncthreads();
  const int x = x0 + t;
  if (x >= a.X) return;
  // the taps outermost: one read of g[u], h[u] serves the lane's LF_XR outputs; each output still adds its taps in ascending order
  double s0[LF_XR], s2[LF_XR];
#pragma unroll
  for (int k = 0; k < LF_XR; ++k) s0[k] = s2[k] = 0.0;
  const double* p = tile + t;
  for (int u = 0; u < nt; ++u) {
    const double gu = g[u], hu = h[u];
#pragma unroll
    for (int k = 0; k < LF_XR; ++k) {
      const double v = p[k * span + u];
      s0[k] += gu * v;
      s2[k] += hu * v;
    }
  }
#pragma unroll
  for (int k = 0; k < LF_XR; ++k)
    if (k < nrow) {
      const long o = (row0 + k) * a.X + x;
      a.f[0][o] = s0[k];
      a.f[1][o] = s2[k];
    }
}

// ZPASS 0: along y, A0 / A2 -> B0 / C.  ZPASS 1: along z, B0 / C -> out.
template <int ZPASS>
__global__ void __launch_bounds__(RAD_TPB) log_col_kernel(const LogArgs a) {
  extern __shared__ __attribute__((aligned(16))) double log_lds[];
  const int t = threadIdx.x, r = a.r[1 + ZPASS], nt = 2 * r + 1, span = LF_LT + 2 * r;
  double* g = log_lds;
  double* h = g + nt;
  double* f0 = h + nt;                      // [span][LF_CT]: A0 (y pass), B0 (z pass)
  double* f1 = f0 + span * LF_CT;           //                A2,          C
  const double* in0 = a.f[2 * ZPASS];
  const double* in1 = a.f[2 * ZPASS + 1];
  const int L = ZPASS ? a.Z : a.Y;
  const long stride = ZPASS ? (long)a.X * a.Y : (long)a.X, ostride = ZPASS ? (long)a.X : (long)a.X * a.Y;
  const int tiles_x = (a.X + LF_CT - 1) / LF_CT, tiles_l = (L + LF_LT - 1) / LF_LT;
  unsigned b = blockIdx.x;
  const int x0 = (int)(b % tiles_x) * LF_CT;
  b /= tiles_x;
  const int l0 = (int)(b % tiles_l) * LF_LT;
  const int o = (int)(b / tiles_l);         // the other axis (z, y): the grid is tiles_x * tiles_l * its extent
  const long base = o * ostride;
  for (int i = t; i < 2 * nt; i += RAD_TPB) g[i] = a.taps[a.toff[1 + ZPASS] + i];
  for (int i = t; i < span * LF_CT; i += RAD_TPB) {
    const int x = x0 + (i % LF_CT);
    if (x < a.X) {
      const long s = base + log_clamp(l0 - r + i / LF_CT, L) * stride + x;
      f0[i] = in0[s];
      f1[i] = in1[s];
    }
  }
  __syncthreads();
  const int c = t % LF_CT, x = x0 + c;
  if (x >= a.X) return;
  // the taps outermost: one read of g[u], h[u] serves the lane's LF_PER outputs (rows lr, lr + 16, ...; the halo is staged for every
  // row of the tile, so a row past the extent is computed from defined values and not stored); each output adds its taps in ascending order
  const int lr = t / LF_CT;
  const double* p0 = f0 + lr * LF_CT + c;
  const double* p1 = f1 + lr * LF_CT + c;
  double s0[LF_PER], s1[LF_PER], s2[LF_PER];   // y: B0, g . A2, h . A0;  z: g . C, h . B0 (s0 unused)
#pragma unroll
  for (int j = 0; j < LF_PER; ++j) s0[j] = s1[j] = s2[j] = 0.0;
  for (int u = 0; u < nt; ++u) {
    const double gu = g[u], hu = h[u];
#pragma unroll
    for (int j = 0; j < LF_PER; ++j) {
      const double v0 = p0[(j * LF_LANES_L + u) * LF_CT], v1 = p1[(j * LF_LANES_L + u) * LF_CT];
      if (ZPASS == 0) s0[j] += gu * v0;
      s1[j] += gu * v1;
      s2[j] += hu * v0;
    }
  }
#pragma unroll
  for (int j = 0; j < LF_PER; ++j) {
    const int l = lr + j * LF_LANES_L;
    if (l0 + l < L) {
      const long idx = base + (l0 + l) * stride + x;
      if (ZPASS == 0) {
        a.f[2][idx] = s0[j];
        a.f[3][idx] = s1[j] * a.w[0] + s2[j] * a.w[1];
      } else {
        a.out[idx] = (float)(s1[j] + s2[j] * a.w[2]);
      }
    }
  }
}

namespace {

int log_validate(int x, int y, int z) {
  MMNN_REQUIRE(x >= 1 && y >= 1 && z >= 1, "log_filter: non-positive extent %d x %d x %d", x, y, z);
  MMNN_REQUIRE((double)x * y * z < 2147483648.0, "log_filter: extent %d x %d x %d holds 2^31 voxels or more", x, y, z);
  return 0;
}

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_log_filter_workspace_bytes(int32_t x, int32_t y, int32_t z) {
  if (log_validate(x, y, z) != 0) return -1;
  return (int64_t)log_layout((long)x * y * z).total;
}

int mmnn_log_filter(const mmnn_log_filter_desc* d, const void* scan, const double* taps, float* out, void* ws, void* stream_) {
  MMNN_REQUIRE(d, "log_filter: null descriptor");
  if (log_validate(d->x, d->y, d->z) != 0) return 1;
  const int ssz = ig_type_size(d->scan_type);
  MMNN_REQUIRE(ssz != 0, "log_filter: unsupported scan datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->scan_type);
  for (int k = 0; k < 3; ++k) {
    MMNN_REQUIRE(d->radius[k] >= 1 && d->radius[k] <= LF_MAX_R, "log_filter: radius[%d] = %d outside 1..%d", k, d->radius[k], LF_MAX_R);
    MMNN_REQUIRE(std::isfinite(d->weight[k]), "log_filter: weight[%d] is not finite", k);
  }
  MMNN_REQUIRE(scan && taps && out && ws, "log_filter: null argument");
  MMNN_REQUIRE((uintptr_t)scan % ssz == 0, "log_filter: scan buffer not aligned to its element size");
  MMNN_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)taps % 8 == 0 && (uintptr_t)out % 4 == 0, "log_filter: misaligned workspace / taps / out");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const LogLayout L = log_layout((long)d->x * d->y * d->z);
  char* wsb = static_cast<char*>(ws);
  LogArgs a{};
  a.scan = scan; a.taps = taps; a.out = out;
  for (int k = 0; k < 4; ++k) a.f[k] = reinterpret_cast<double*>(wsb + L.f[k]);
  a.X = d->x; a.Y = d->y; a.Z = d->z; a.code = d->scan_type;
  a.sc = rad_scale(d->scan_slope, d->scan_inter);
  int off = 0;
  for (int k = 0; k < 3; ++k) {
    a.r[k] = d->radius[k];
    a.w[k] = d->weight[k];
    a.toff[k] = off;
    off += 2 * (2 * d->radius[k] + 1);
  }
  // every grid is below 2^31 workgroups: each workgroup owns at least one voxel
  const long rows = (long)d->y * d->z;
  const long gx = (long)cdiv(d->x, LF_XT) * ((rows + LF_XR - 1) / LF_XR);
  const long gy = (long)cdiv(d->x, LF_CT) * cdiv(d->y, LF_LT) * d->z;
  const long gz = (long)cdiv(d->x, LF_CT) * cdiv(d->z, LF_LT) * d->y;
  MMNN_LAUNCH(log_x_kernel, dim3((unsigned)gx), dim3(RAD_TPB), log_x_lds(a.r[0]), stream, a);
  MMNN_LAUNCH(log_col_kernel<0>, dim3((unsigned)gy), dim3(RAD_TPB), log_col_lds(a.r[1]), stream, a);
  MMNN_LAUNCH(log_col_kernel<1>, dim3((unsigned)gz), dim3(RAD_TPB), log_col_lds(a.r[2]), stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
