// The margin step behind the mask routes: an exact, bounded Euclidean distance to the mask under the scan's voxel spacing, thresholded at
// a radius in mm (DILATE: the tumour plus its rim; SHELL: the rim alone).  The contract is the comment above mmnn_mask_margin in
// include/mmnn_sts.h.  Everything is enqueued on the caller's stream; nothing is read back and the host never waits.
//
//   margin_x_kernel    MM_XR rows x MM_XT outputs along x per workgroup: the rows' set flags, tile plus halo, are staged in LDS as bytes
//                      (0 outside the volume); one output per lane and row: the smallest k <= r_x with a set voxel at x - k or x + k,
//                      MM_NONE when there is none                                               mask -> K (one byte per voxel)
//   margin_col_kernel<0>  a tile of MM_CT columns along x x MM_LT outputs along y, staged with its halo as fp64 t_x(K) (+inf for
//                      MM_NONE and outside the volume), the t_y table beside it; lane (column, row) owns the MM_PER adjacent rows
//                      4 row .. 4 row + 3 and slides one window over them: a staged value is read once for the four outputs, each
//                      of which takes the minimum of fl(t_x + t_y(|dy|)) over its own 2 r + 1 entries   K -> B (fp64)
//   margin_col_kernel<1>  the same tile along z over B; thresholds at R2                        B -> out, dist2
//
// Why three passes give the brute-force minimum bit for bit: a rounded addition is monotone in each operand, so min_q fl(a_q + c) =
// fl((min_q a_q) + c).  The x pass finds the smallest t_x per (row, x), the y pass the smallest fl(t_x + t_y) per (x, y', z) -- for a
// fixed dy the smallest t_x gives the smallest sum -- and the z pass likewise over fl(. + t_z).  A minimum does not depend on the order
// it is taken in (no NaN can arise: every term is >= 0, and +inf only ever meets finite terms or +inf under an addition).
// Every loop bound is r_a = min(reach_a, extent_a - 1), from the descriptor alone: no walk depends on the data.  One lane per output,
// no atomics.
// LDS.  The column tile holds (MM_LT + 2 r) rows of MM_PITCH = 20 fp64 (16 columns and 4 of padding, so that the two lane rows of a
// half-wave, four tile rows apart, read disjoint banks) = 160 (64 + 2 r) bytes, and the 2 r + 8 entries of the term table (t(|d|) for
// |d| <= r, +inf around it, which is what lets four outputs share one window): 52.1 KiB at r = MMNN_MARGIN_MAX_REACH = 128, inside the
// 64 KiB a launch gets without asking for more.  The x tile is MM_XR (256 + 2 r) bytes.
// No scalar memory writes.
#include "ingest_load.hpp"
#include "radiomics.hpp"

#include <cmath>

namespace mmnn {

constexpr int MM_TPB = 256;
constexpr int MM_XT = MM_TPB;               // outputs along x per workgroup of the x pass: one per lane
constexpr int MM_XR = 4;                    // rows per workgroup of the x pass
constexpr int MM_CT = 16;                   // columns (along x) of a y / z tile
constexpr int MM_LT = 64;                   // outputs along the searched axis of a y / z tile
constexpr int MM_LANES_L = MM_TPB / MM_CT;  // lane rows of a y / z tile
constexpr int MM_PER = MM_LT / MM_LANES_L;  // outputs per lane of a y / z tile: adjacent along the searched axis
constexpr int MM_PITCH = MM_CT + 4;         // fp64 per staged tile row
constexpr int MM_MAX_R = MMNN_MARGIN_MAX_REACH;
constexpr int MM_NONE = 255;                // K: no set voxel within r_x along the row
static_assert(MM_LT % MM_LANES_L == 0, "whole trips over the tile");
static_assert(MM_MAX_R < MM_NONE, "an index distance and the sentinel share a byte");
static_assert(MM_MAX_R >= 75, "30 mm at 0.4 mm in-plane");
static_assert((size_t)((MM_LT + 2 * MM_MAX_R) * MM_PITCH + 2 * MM_MAX_R + 2 * MM_PER) * 8 <= 64 * 1024, "the column tile at the largest reach");
static_assert((MM_PER * MM_PITCH * 8) % 256 == 128, "lane rows of a half-wave half a bank period apart");
static_assert((size_t)MM_XR * (MM_XT + 2 * MM_MAX_R) <= 64 * 1024, "the x tile at the largest reach");

struct MarginArgs {
  const void* mask;
  uint8_t* k;                               // [Z][Y][X] bytes
  double* b;                                // [Z][Y][X] fp64
  uint8_t* out;
  double* dist2;                            // may be null
  int X, Y, Z, code;
  IgScale sc;
  int r[3];                                 // x, y, z: min(reach, extent - 1)
  double s[3];
  double r2;
  int shell;
};

struct MarginLayout { size_t k, b, total; };

inline MarginLayout margin_layout(long n) {
  MarginLayout L;
  Carver cv;
  L.k = cv.take((size_t)n);
  L.b = cv.take((size_t)n * 8);
  L.total = cv.cur;
  return L;
}

inline size_t margin_x_lds(int r) { return (size_t)MM_XR * (MM_XT + 2 * r); }
inline size_t margin_col_lds(int r) { return (size_t)((MM_LT + 2 * r) * MM_PITCH + 2 * r + 2 * MM_PER) * 8; }

// t_a(k) = fl(fl(k s) fl(k s)), on the host and on the device (the file is built without contraction)
__host__ __device__ inline double margin_term(int k, double s) {
  const double d = (double)k * s;
  return d * d;
}

__global__ void __launch_bounds__(MM_TPB) margin_x_kernel(const MarginArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mm_flags[];   // [MM_XR][span]
  const int t = threadIdx.x, r = a.r[0], span = MM_XT + 2 * r;
  const int tiles = (a.X + MM_XT - 1) / MM_XT;
  const long rows = (long)a.Y * a.Z, row0 = (long)(blockIdx.x / tiles) * MM_XR;
  const int x0 = (int)(blockIdx.x % tiles) * MM_XT;
  for (int k = 0; k < MM_XR; ++k) {          // a row past the last one and a voxel outside the row are staged as not set
    const long row = row0 + k;
    for (int i = t; i < span; i += MM_TPB) {
      const int x = x0 - r + i;
      unsigned char f = 0;
      if (row < rows && x >= 0 && x < a.X) {
        double v[1];
        ig_load<1>(a.mask, a.code, row * a.X + x, v);
        f = !(ig_scaled(v[0], a.sc) == 0.0);  // a NaN counts as set
      }
      mm_flags[k * span + i] = f;
    }
  }
  __syncthreads();
  const int x = x0 + t;
  if (x >= a.X) return;
  int best[MM_XR];
#pragma unroll
  for (int k = 0; k < MM_XR; ++k) best[k] = MM_NONE;
  const unsigned char* p = mm_flags + t + r;   // the lane's own voxel; p[-r] .. p[+r] are staged
  for (int d = r; d >= 0; --d) {
#pragma unroll
    for (int k = 0; k < MM_XR; ++k)
      if (p[k * span - d] | p[k * span + d]) best[k] = d;
  }
#pragma unroll
  for (int k = 0; k < MM_XR; ++k)
    if (row0 + k < rows) a.k[(row0 + k) * a.X + x] = (uint8_t)best[k];
}

// ZPASS 0: along y, K -> B.  ZPASS 1: along z, B -> out, dist2.
template <int ZPASS>
__global__ void __launch_bounds__(MM_TPB) margin_col_kernel(const MarginArgs a) {
  extern __shared__ __attribute__((aligned(16))) double mm_lds[];
  const int t = threadIdx.x, r = a.r[1 + ZPASS], span = MM_LT + 2 * r;
  const int nt = 2 * r + 2 * MM_PER;
  double* term = mm_lds;                    // [nt]: entry e is t_a(|d|) for d = e - r - (MM_PER - 1) when |d| <= r, else +inf
  double* tile = term + nt;                 // [span][MM_PITCH]
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const int L = ZPASS ? a.Z : a.Y;
  const long stride = ZPASS ? (long)a.X * a.Y : (long)a.X, ostride = ZPASS ? (long)a.X : (long)a.X * a.Y;
  const int tiles_x = (a.X + MM_CT - 1) / MM_CT, tiles_l = (L + MM_LT - 1) / MM_LT;
  unsigned b = blockIdx.x;
  const int x0 = (int)(b % tiles_x) * MM_CT;
  b /= tiles_x;
  const int l0 = (int)(b % tiles_l) * MM_LT;
  const int o = (int)(b / tiles_l);         // the other axis (z, y): the grid is tiles_x * tiles_l * its extent
  const long base = o * ostride;
  for (int i = t; i < nt; i += MM_TPB) {
    const int d = i - r - (MM_PER - 1), k = d < 0 ? -d : d;
    term[i] = k <= r ? margin_term(k, a.s[1 + ZPASS]) : inf;
  }
  for (int i = t; i < span * MM_CT; i += MM_TPB) {   // every entry the lanes read is written: +inf outside the volume
    const int col = i % MM_CT, row = i / MM_CT, x = x0 + col, l = l0 - r + row;
    double v = inf;
    if (x < a.X && l >= 0 && l < L) {
      const long s = base + l * stride + x;
      if (ZPASS == 0) {
        const int k = a.k[s];
        if (k != MM_NONE) v = margin_term(k, a.s[0]);
      } else {
        v = a.b[s];
      }
    }
    tile[row * MM_PITCH + col] = v;
  }
  __syncthreads();
  const int c = t % MM_CT, x = x0 + c;
  if (x >= a.X) return;
  // Output j of the lane is row MM_PER lr + j of the tile; staged row MM_PER lr + u lies d = u - j - r from it, so at step u output j
  // adds term[u - j + MM_PER - 1]: the four terms shift down by one per step and one new one is read.  A step outside an output's own
  // window adds +inf, which leaves its minimum alone.  (The halo is staged for every row of the tile, so a row past the extent is
  // computed from defined values and not stored.)
  const int lr = t / MM_CT;
  const double* p = tile + lr * MM_PER * MM_PITCH + c;
  double m[MM_PER], tt[MM_PER];
#pragma unroll
  for (int j = 0; j < MM_PER; ++j) {
    m[j] = inf;
    tt[j] = term[MM_PER - 1 - j];
  }
#pragma unroll MM_PER
  for (int u = 0; u < 2 * r + MM_PER; ++u) {   // (unrolled by MM_PER the shift of the terms is a renaming, not moves)
    const double v = p[u * MM_PITCH];
#pragma unroll
    for (int j = 0; j < MM_PER; ++j) {
      m[j] = fmin(m[j], v + tt[j]);         // (one v_min_f64; no operand is ever a NaN)
    }
#pragma unroll
    for (int j = MM_PER - 1; j > 0; --j) tt[j] = tt[j - 1];
    tt[0] = term[u + MM_PER];               // the last step reads entry 2 r + 2 MM_PER - 1, the table's last (+inf)
  }
#pragma unroll
  for (int j = 0; j < MM_PER; ++j) {
    const int l = lr * MM_PER + j;
    if (l0 + l < L) {
      const long idx = base + (l0 + l) * stride + x;
      if (ZPASS == 0) {
        a.b[idx] = m[j];
      } else {
        const bool in = m[j] <= a.r2;
        a.out[idx] = (uint8_t)(in && !(a.shell && m[j] == 0.0));
        if (a.dist2) a.dist2[idx] = in ? m[j] : inf;
      }
    }
  }
}

namespace {

int margin_validate(int x, int y, int z) {
  MMNN_REQUIRE(x >= 1 && y >= 1 && z >= 1, "mask_margin: non-positive extent %d x %d x %d", x, y, z);
  MMNN_REQUIRE((double)x * y * z < 2147483648.0, "mask_margin: extent %d x %d x %d holds 2^31 voxels or more", x, y, z);
  return 0;
}

// reach_a: the largest k with t_a(k) <= R2 (t_a is non-decreasing in k); the search stops one past the cap, which the caller refuses.
int margin_reach(const double spacing[3], double radius, int32_t reach[3]) {
  MMNN_REQUIRE(std::isfinite(radius) && radius > 0.0, "mask_margin: radius %g is not finite and > 0", radius);
  const double r2 = radius * radius;
  for (int a = 0; a < 3; ++a) {
    MMNN_REQUIRE(std::isfinite(spacing[a]) && spacing[a] > 0.0, "mask_margin: spacing[%d] = %g is not finite and > 0", a, spacing[a]);
    int k = 0;
    while (k <= MM_MAX_R && margin_term(k + 1, spacing[a]) <= r2) ++k;
    reach[a] = k;
  }
  return 0;
}

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int mmnn_mask_margin_reach(const double spacing[3], double radius, int32_t reach[3]) {
  MMNN_REQUIRE(spacing && reach, "mask_margin: null spacing or reach");
  int32_t r[3];
  if (margin_reach(spacing, radius, r) != 0) return 1;
  for (int a = 0; a < 3; ++a)
    MMNN_REQUIRE(r[a] <= MM_MAX_R, "mask_margin: a radius of %g mm reaches more than %d voxels along axis %d (spacing %g mm)", radius, MM_MAX_R, a,
                 spacing[a]);
  for (int a = 0; a < 3; ++a) reach[a] = r[a];
  return 0;
}

int64_t mmnn_mask_margin_workspace_bytes(int32_t x, int32_t y, int32_t z) {
  if (margin_validate(x, y, z) != 0) return -1;
  return (int64_t)margin_layout((long)x * y * z).total;
}

int mmnn_mask_margin(const mmnn_mask_margin_desc* d, const void* mask, uint8_t* out, double* dist2, void* ws, void* stream_) {
  MMNN_REQUIRE(d, "mask_margin: null descriptor");
  MMNN_REQUIRE(mask && out && ws, "mask_margin: null mask, out or workspace");
  if (margin_validate(d->x, d->y, d->z) != 0) return 1;
  const int ssz = ig_type_size(d->mask_type);
  MMNN_REQUIRE(ssz != 0, "mask_margin: unsupported mask datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->mask_type);
  MMNN_REQUIRE(d->mode == MMNN_MARGIN_DILATE || d->mode == MMNN_MARGIN_SHELL, "mask_margin: mode %d is neither MMNN_MARGIN_DILATE nor MMNN_MARGIN_SHELL",
               d->mode);
  int32_t reach[3];
  if (mmnn_mask_margin_reach(d->spacing, d->radius, reach) != 0) return 1;
  const long n = (long)d->x * d->y * d->z;
  const uintptr_t m0 = (uintptr_t)mask, o0 = (uintptr_t)out;
  MMNN_REQUIRE(m0 + (uintptr_t)n * ssz <= o0 || o0 + (uintptr_t)n <= m0, "mask_margin: mask and out overlap");
  MMNN_REQUIRE(m0 % ssz == 0, "mask_margin: mask buffer not aligned to its element size");
  MMNN_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)dist2 % 8 == 0, "mask_margin: misaligned workspace / dist2");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MarginLayout L = margin_layout(n);
  char* wsb = static_cast<char*>(ws);
  MarginArgs a{};
  a.mask = mask; a.out = out; a.dist2 = dist2;
  a.k = reinterpret_cast<uint8_t*>(wsb + L.k);
  a.b = reinterpret_cast<double*>(wsb + L.b);
  a.X = d->x; a.Y = d->y; a.Z = d->z; a.code = d->mask_type;
  a.sc = rad_scale(d->mask_slope, d->mask_inter);
  const int ext[3] = {d->x, d->y, d->z};
  for (int k = 0; k < 3; ++k) {
    a.r[k] = reach[k] < ext[k] - 1 ? reach[k] : ext[k] - 1;   // no voxel of the volume lies farther along the axis
    a.s[k] = d->spacing[k];
  }
  a.r2 = d->radius * d->radius;
  a.shell = d->mode == MMNN_MARGIN_SHELL;
  // every grid is below 2^31 workgroups: each workgroup owns at least one voxel
  const long rows = (long)d->y * d->z;
  const long gx = (long)cdiv(d->x, MM_XT) * ((rows + MM_XR - 1) / MM_XR);
  const long gy = (long)cdiv(d->x, MM_CT) * cdiv(d->y, MM_LT) * d->z;
  const long gz = (long)cdiv(d->x, MM_CT) * cdiv(d->z, MM_LT) * d->y;
  MMNN_LAUNCH(margin_x_kernel, dim3((unsigned)gx), dim3(MM_TPB), margin_x_lds(a.r[0]), stream, a);
  MMNN_LAUNCH(margin_col_kernel<0>, dim3((unsigned)gy), dim3(MM_TPB), margin_col_lds(a.r[1]), stream, a);
  MMNN_LAUNCH(margin_col_kernel<1>, dim3((unsigned)gz), dim3(MM_TPB), margin_col_lds(a.r[2]), stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
