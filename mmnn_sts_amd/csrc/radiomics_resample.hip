// The two pre-steps of the radiomics path: whole-scan intensity normalisation and resampling of the (scan, mask) pair onto a grid of a
// stated spacing, cubic B-spline for the scan and nearest neighbour for the mask.  The contracts are the comments above
// mmnn_normalize_scan and mmnn_resample_pair in include/mmnn_sts.h.  Everything is enqueued on the caller's stream; nothing is read back
// and the host never waits.
//
//   norm_sum_kernel<0>  workgroup p of `parts` takes the chunks p + k * parts of NM_TPB voxels, k ascending -> part[p] = sum v and the
//                       count of non-finite voxels; one block_reduce per workgroup                scan -> part, bad
//   norm_sum_kernel<1>  every workgroup folds part[] to the mean (lane p holds part p; block_reduce), then the same partition
//                       of (v - mean)^2                                                            scan, part -> part2
//   norm_write_kernel   every workgroup folds part[] and part2[] again (two block_reduces of at most NM_MAX_PARTS values: cheaper than
//                       a launch of one workgroup in between), then strides over the voxels, each output computed by one lane alone;
//                       workgroup 0 writes the result block
//   rs_prefilter_x_kernel  one wave carries RS_XL = 16 lines along x; chunks of RS_XC = 64 samples go through an LDS tile
//                       [RS_XL][RS_XC + 1] fp64: staged with lanes along x (one line's 64 samples per trip: 512 contiguous bytes of fp64,
//                       128 of int16; the loads of RS_BATCH lines in flight together), recursed by lanes 0 .. 15 with one line each (the
//                       odd row pitch spreads the lines over the banks), stored with lanes along x.  The walk is a chain of dependent
//                       LDS reads and fp64 operations that nothing in its wave overlaps, and Y * Z lines are few: 16 lines per wave
//                       instead of 64 puts four times as many waves on the chip (the times are in DESIGN.md 16.5).  Forward over the
//                       chunks (scan -> c+ in coef), then backward (c+ -> c-, in place).
//                       The 40 samples of the initial sum are read from global memory by the line's own lane, strided.
//   rs_prefilter_line_kernel<ZPASS>  y and z: one lane per line, lanes along x, so every load and store of the serial walk is
//                       coalesced as it is; in place on coef
//   rs_eval_kernel<AXIS>, rs_eval_z_kernel  the separable 4-tap gather, lanes along x, every output computed by one lane alone:
//                       coef -> T1 [Z][Y][MX] -> T2 [Z][MY][MX] -> out [MZ][MY][MX] float32, the mask byte in the last launch,
//                       whose lanes walk RS_ZRUN output planes each
//
// Order.  Every sum starts from +0.0 and runs over k ascending, product then addition (the build passes -ffp-contract=off); the
// recursions are one lane per line.  No reduction across lanes but the fp64 sums of the normalisation, which are block_reduce
// (reduce.hpp) over a partition fixed by the extents: no atomics anywhere, repeated calls are bit-identical.
// No scalar memory writes.
#include "radiomics.hpp"

#include <cmath>

namespace mmnn {

constexpr int NM_TPB = RAD_TPB;             // lanes of a normalisation workgroup; one chunk of the partition is NM_TPB voxels
constexpr int NM_MAX_PARTS = RAD_MAX_PARTS; // workgroups of a sum pass: min(NM_MAX_PARTS, ceil(n / NM_TPB))
constexpr int NM_BATCH = 4;                 // loads a lane keeps in flight in the three passes
constexpr int NM_WRITE_GROUPS = 2048;       // workgroups of the write pass at most: each folds the parts once, then strides over the voxels
constexpr int RS_XL = 16;                   // lines per workgroup (one wave) of the x prefilter: lanes 0 .. RS_XL - 1 walk one each
constexpr int RS_XC = 64;                   // samples along x per chunk of the x prefilter: one per lane while a chunk is staged or stored
constexpr int RS_TPB = RAD_TPB;             // lanes per workgroup of the y / z prefilter and of the evaluation
constexpr int RS_BATCH = 8;                 // samples of a line (lines of a tile) whose loads are issued together
constexpr int RS_ZRUN = 16;                 // consecutive output planes a workgroup of the last gather walks
constexpr int RS_H = MMNN_RESAMPLE_HORIZON;
static_assert(RS_XL % RS_BATCH == 0, "whole batches over the tile's lines");
static_assert(NM_MAX_PARTS <= NM_TPB, "one lane per part when the parts are folded");
static_assert((size_t)RS_XL * (RS_XC + 1) * 8 <= 64 * 1024, "the x prefilter's tile");

struct NormArgs {
  const void* scan;
  float* out;
  double* part;                             // [NM_MAX_PARTS] sums of v
  double* part2;                            // [NM_MAX_PARTS] sums of (v - mean)^2
  long long* bad;                           // [NM_MAX_PARTS] non-finite voxels
  mmnn_normalize_result* result;
  long n;
  int parts, code;
  IgScale sc;
  double scale, bound;                      // bound = outliers * scale; 0: no clamp
};

struct NormLayout { size_t part, part2, bad, total; };

inline NormLayout norm_layout() {
  NormLayout L;
  Carver cv;
  L.part = cv.take((size_t)NM_MAX_PARTS * 8);
  L.part2 = cv.take((size_t)NM_MAX_PARTS * 8);
  L.bad = cv.take((size_t)NM_MAX_PARTS * 8);
  L.total = cv.cur;
  return L;
}

__device__ __forceinline__ double norm_value(const NormArgs& a, long i) {
  double v[1];
  ig_load<1>(a.scan, a.code, i, v);
  return ig_scaled(v[0], a.sc);
}

// The parts' values folded: lane p holds part p (+0.0 past the last); block_reduce folds the lanes of each wave by the butterfly, then
// the waves in index order.
__device__ __forceinline__ double norm_fold(const double* part, int parts, double* lds) {
  const int t = threadIdx.x;
  return block_reduce<NM_TPB / 64>(t < parts ? part[t] : 0.0, lds, Sum{});
}

template <int PASS>
__device__ __forceinline__ void norm_add(double v, double mean, double& s, long long& bad) {
  if (PASS == 0) {
    s += v;
    bad += !isfinite(v);
  } else {
    const double d = v - mean;
    s += d * d;
  }
}

template <int PASS>
__global__ void __launch_bounds__(NM_TPB) norm_sum_kernel(const NormArgs a) {
  __shared__ double lds[NM_TPB / 64];
  __shared__ long long ldsb[NM_TPB / 64];
  const int t = threadIdx.x;
  double mean = 0.0;
  if (PASS == 1) {
    mean = norm_fold(a.part, a.parts, lds) / (double)a.n;
  }
  double s = 0.0;
  long long bad = 0;
  const long step = (long)a.parts * NM_TPB;
  long i = (long)blockIdx.x * NM_TPB + t;
  // NM_BATCH loads in flight per lane; the additions keep the order k ascending
  for (; i + (NM_BATCH - 1) * step < a.n; i += NM_BATCH * step) {
    double v[NM_BATCH];
#pragma unroll
    for (int j = 0; j < NM_BATCH; ++j) v[j] = norm_value(a, i + j * step);
#pragma unroll
    for (int j = 0; j < NM_BATCH; ++j) norm_add<PASS>(v[j], mean, s, bad);
  }
  for (; i < a.n; i += step) norm_add<PASS>(norm_value(a, i), mean, s, bad);
  s = block_reduce<NM_TPB / 64>(s, lds, Sum{});
  if (PASS == 0) {
    bad = block_reduce<NM_TPB / 64>(bad, ldsb, Sum{});
    if (t == 0) {
      a.part[blockIdx.x] = s;
      a.bad[blockIdx.x] = bad;
    }
  } else if (t == 0) {
    a.part2[blockIdx.x] = s;
  }
}

__device__ __forceinline__ float norm_out(const NormArgs& a, double v, double mean, double sd) {
  double u = ((v - mean) / sd) * a.scale;
  if (a.bound > 0.0) u = u < -a.bound ? -a.bound : (u > a.bound ? a.bound : u);   // a NaN passes both comparisons and stays
  return (float)u;
}

__global__ void __launch_bounds__(NM_TPB) norm_write_kernel(const NormArgs a) {
  __shared__ double lds[NM_TPB / 64];
  __shared__ long long ldsb[NM_TPB / 64];
  const int t = threadIdx.x;
  const double mean = norm_fold(a.part, a.parts, lds) / (double)a.n;
  const double ssq = norm_fold(a.part2, a.parts, lds);
  const long long bad = block_reduce<NM_TPB / 64>(t < a.parts ? a.bad[t] : 0ll, ldsb, Sum{});
  const double sd = sqrt(ssq / (double)(a.n - 1));
  if (blockIdx.x == 0 && t == 0) {
    a.result->n = a.n;
    a.result->mean = mean;
    a.result->sd = sd;
    a.result->nonfinite = bad != 0;
  }
  // a non-finite voxel has made mean and sd NaN, a constant scan gives 0 / 0: NaN everywhere
  const long step = (long)gridDim.x * NM_TPB;
  long i = (long)blockIdx.x * NM_TPB + t;
  for (; i + (NM_BATCH - 1) * step < a.n; i += NM_BATCH * step) {
    double v[NM_BATCH];
#pragma unroll
    for (int j = 0; j < NM_BATCH; ++j) v[j] = norm_value(a, i + j * step);
#pragma unroll
    for (int j = 0; j < NM_BATCH; ++j) a.out[i + j * step] = norm_out(a, v[j], mean, sd);
  }
  for (; i < a.n; i += step) a.out[i] = norm_out(a, norm_value(a, i), mean, sd);
}

// ---- resampling -------------------------------------------------------------------------------------------------------------------------
struct ResArgs {
  const void* scan; const void* mask;
  const mmnn_resample_entry* tab[3];        // the device tables of x, y, z
  double* coef;                             // [Z][Y][X]
  double* t1;                               // [Z][Y][MX]
  double* t2;                               // [Z][MY][MX]
  float* out;                               // [MZ][MY][MX]
  uint8_t* omask;
  int X, Y, Z, MX, MY, MZ, scode, mcode;
  IgScale ss, ms;
  double pole, pole_gain, gain;
  double zpow[RS_H];
};

struct ResLayout { size_t coef, t1, t2, total; };

inline ResLayout res_layout(long x, long y, long z, long mx, long my) {
  ResLayout L;
  Carver cv;
  L.coef = cv.take((size_t)(x * y * z) * 8);
  L.t1 = cv.take((size_t)(mx * y * z) * 8);
  L.t2 = cv.take((size_t)(mx * my * z) * 8);
  L.total = cv.cur;
  return L;
}

// Whole-sample symmetric reflection of k, 0 <= k < RS_H, into 0 .. n - 1, period 2 n - 2 (n >= 2).  Only an axis shorter than the
// horizon reflects at all, so the period is formed from an n below RS_H and cannot overflow at any extent.
__device__ __forceinline__ int rs_mirror(int k, int n) {
  if (k < n) return k;
  const int p = 2 * n - 2, r = k % p;
  return r < n ? r : p - r;
}

__global__ void __launch_bounds__(RS_XC) rs_prefilter_x_kernel(const ResArgs a) {
  __shared__ double tile[RS_XL][RS_XC + 1];
  const int t = threadIdx.x, X = a.X;
  const long lines = (long)a.Y * a.Z, line0 = (long)blockIdx.x * RS_XL;
  const int nl = lines - line0 < RS_XL ? (int)(lines - line0) : RS_XL;
  const bool mine = t < nl, filt = X > 1;   // an axis of extent 1 is left as it is: coef = the scaled scan
  const long base = (line0 + t) * X;
  double c = 0.0, cprev = 0.0;
  if (mine && filt) {                       // c+[0]: the horizon's samples of this lane's line, strided
    for (int k = 0; k < RS_H; ++k) {
      double v[1];
      ig_load<1>(a.scan, a.scode, base + rs_mirror(k, X), v);
      c += a.zpow[k] * (a.gain * ig_scaled(v[0], a.ss));
    }
  }
  for (int x0 = 0; x0 < X; x0 += RS_XC) {   // forward: scan -> c+
    const int w = X - x0 < RS_XC ? X - x0 : RS_XC;
    if (t < w)
      for (int l0 = 0; l0 < nl; l0 += RS_BATCH) {       // RS_BATCH loads in flight per lane; a line past the last is read as the last
        double v[RS_BATCH][1];
#pragma unroll
        for (int j = 0; j < RS_BATCH; ++j) ig_load<1>(a.scan, a.scode, (line0 + (l0 + j < nl ? l0 + j : nl - 1)) * X + x0 + t, v[j]);
#pragma unroll
        for (int j = 0; j < RS_BATCH; ++j) {
          const double s = ig_scaled(v[j][0], a.ss);
          tile[l0 + j][t] = filt ? a.gain * s : s;
        }
      }
    __syncthreads();
    if (mine && filt)
      for (int i = 0; i < w; ++i) {
        if (x0 + i > 0) {
          cprev = c;
          c = tile[t][i] + a.pole * c;
        }
        tile[t][i] = c;
      }
    __syncthreads();
    for (int l = 0; l < nl; ++l)
      if (t < w) a.coef[(line0 + l) * X + x0 + t] = tile[l][t];
    __syncthreads();
  }
  // backward: c+ -> c-, in place.  c is c+[X - 1] and cprev c+[X - 2] here.
  if (!filt) return;
  double m = a.pole_gain * (c + a.pole * cprev);
  for (int x0 = (X - 1) / RS_XC * RS_XC; x0 >= 0; x0 -= RS_XC) {
    const int w = X - x0 < RS_XC ? X - x0 : RS_XC;
    if (t < w)
      for (int l0 = 0; l0 < nl; l0 += RS_BATCH) {
        double v[RS_BATCH];
#pragma unroll
        for (int j = 0; j < RS_BATCH; ++j) v[j] = a.coef[(line0 + (l0 + j < nl ? l0 + j : nl - 1)) * X + x0 + t];
#pragma unroll
        for (int j = 0; j < RS_BATCH; ++j) tile[l0 + j][t] = v[j];
      }
    __syncthreads();
    if (mine)
      for (int i = w - 1; i >= 0; --i) {
        if (x0 + i < X - 1) m = a.pole * (m - tile[t][i]);
        tile[t][i] = m;
      }
    __syncthreads();
    for (int l = 0; l < nl; ++l)
      if (t < w) a.coef[(line0 + l) * X + x0 + t] = tile[l][t];
    __syncthreads();
  }
}

// ZPASS 0: along y, lines (x, z).  ZPASS 1: along z, lines (x, y).  In place on coef.
template <int ZPASS>
__global__ void __launch_bounds__(RS_TPB) rs_prefilter_line_kernel(const ResArgs a) {
  const long XY = (long)a.X * a.Y, lines = ZPASS ? XY : (long)a.X * a.Z, line = (long)blockIdx.x * RS_TPB + threadIdx.x;
  if (line >= lines) return;
  const int n = ZPASS ? a.Z : a.Y;
  const long es = ZPASS ? XY : (long)a.X;
  double* p = a.coef + (ZPASS ? line : (line / a.X) * XY + line % a.X);
  double c = 0.0, cprev = 0.0;
  for (int k = 0; k < RS_H; ++k) c += a.zpow[k] * (a.gain * p[rs_mirror(k, n) * es]);
  p[0] = c;
  // the loads of RS_BATCH samples are issued together (they do not depend on the recursion); a sample past the end is read as the last
  for (int k0 = 1; k0 < n; k0 += RS_BATCH) {
    double v[RS_BATCH];
#pragma unroll
    for (int j = 0; j < RS_BATCH; ++j) v[j] = p[(k0 + j < n ? k0 + j : n - 1) * es];
#pragma unroll
    for (int j = 0; j < RS_BATCH; ++j)
      if (k0 + j < n) {
        cprev = c;
        c = a.gain * v[j] + a.pole * c;
        p[(k0 + j) * es] = c;
      }
  }
  double m = a.pole_gain * (c + a.pole * cprev);
  p[(n - 1) * es] = m;
  for (int k0 = n - 2; k0 >= 0; k0 -= RS_BATCH) {
    double v[RS_BATCH];
#pragma unroll
    for (int j = 0; j < RS_BATCH; ++j) v[j] = p[(k0 - j >= 0 ? k0 - j : 0) * es];
#pragma unroll
    for (int j = 0; j < RS_BATCH; ++j)
      if (k0 - j >= 0) {
        m = a.pole * (m - v[j]);
        p[(k0 - j) * es] = m;
      }
  }
}

// AXIS 0: coef -> t1 along x; 1: t1 -> t2 along y.
template <int AXIS>
__global__ void __launch_bounds__(RS_TPB) rs_eval_kernel(const ResArgs a) {
  const long W = a.MX, H = AXIS == 1 ? a.MY : a.Y;
  const long o = (long)blockIdx.x * RS_TPB + threadIdx.x;
  if (o >= W * H * a.Z) return;
  const int jx = (int)(o % W), jy = (int)(o / W % H), jz = (int)(o / (W * H));
  const mmnn_resample_entry e = a.tab[AXIS][AXIS == 0 ? jx : jy];
  const double* in = AXIS == 0 ? a.coef + ((long)jz * a.Y + jy) * a.X : a.t1 + (long)jz * a.Y * W + jx;
  const long es = AXIS == 0 ? 1 : W;        // the gathered line's element stride
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) s += e.w[k] * in[e.i[k] * es];
  (AXIS == 0 ? a.t1 : a.t2)[o] = s;
}

// t2 -> out along z, and the mask byte.  A workgroup owns RS_TPB positions (jx, jy) and walks RS_ZRUN consecutive jz: neighbouring
// output planes gather from nearly the same four planes of t2, which the walk finds in the cache it has just filled; a grid with jz
// slowest took a quarter longer at 410 x 410 x 240 from 48 planes, supposedly because it fetched those planes again for every output
// plane (the times are in DESIGN.md 16.5; no counter was collected).
__global__ void __launch_bounds__(RS_TPB) rs_eval_z_kernel(const ResArgs a) {
  const long WH = (long)a.MX * a.MY, groups = (WH + RS_TPB - 1) / RS_TPB;
  const long pos = (long)(blockIdx.x % groups) * RS_TPB + threadIdx.x;
  if (pos >= WH) return;
  const int jx = (int)(pos % a.MX), jy = (int)(pos / a.MX), jz0 = (int)(blockIdx.x / groups) * RS_ZRUN;
  const mmnn_resample_entry* tx = a.tab[0] + jx;
  const mmnn_resample_entry* ty = a.tab[1] + jy;
  const bool inxy = tx->inside && ty->inside;
  const long near = (long)ty->nearest * a.X + tx->nearest, XY = (long)a.X * a.Y;
  const double* in = a.t2 + pos;
  for (int jz = jz0; jz < jz0 + RS_ZRUN && jz < a.MZ; ++jz) {
    const mmnn_resample_entry e = a.tab[2][jz];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += e.w[k] * in[e.i[k] * WH];
    const bool inside = inxy && e.inside;
    const long o = jz * WH + pos;
    a.out[o] = inside ? (float)s : 0.0f;
    double mv[1] = {0.0};
    if (inside) ig_load<1>(a.mask, a.mcode, e.nearest * XY + near, mv);
    a.omask[o] = inside && !(ig_scaled(mv[0], a.ms) == 0.0) ? 1 : 0;
  }
}

namespace {

int norm_validate(int x, int y, int z) {
  MMNN_REQUIRE(x >= 1 && y >= 1 && z >= 1, "normalize_scan: non-positive extent %d x %d x %d", x, y, z);
  MMNN_REQUIRE((double)x * y * z < 2147483648.0, "normalize_scan: extent %d x %d x %d holds 2^31 voxels or more", x, y, z);
  return 0;
}

int res_validate(int x, int y, int z, int mx, int my, int mz) {
  MMNN_REQUIRE(x >= 1 && y >= 1 && z >= 1, "resample_pair: non-positive extent %d x %d x %d", x, y, z);
  MMNN_REQUIRE(mx >= 1 && my >= 1 && mz >= 1, "resample_pair: non-positive output extent %d x %d x %d", mx, my, mz);
  MMNN_REQUIRE((double)x * y * z < 2147483648.0, "resample_pair: extent %d x %d x %d holds 2^31 voxels or more", x, y, z);
  MMNN_REQUIRE((double)mx * my * mz < 2147483648.0, "resample_pair: output extent %d x %d x %d holds 2^31 voxels or more", mx, my, mz);
  MMNN_REQUIRE((double)mx * y * z < 2147483648.0 && (double)mx * my * z < 2147483648.0,
               "resample_pair: an intermediate of %d x %d x %d -> %d x %d x %d holds 2^31 elements or more", x, y, z, mx, my, mz);
  return 0;
}

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_normalize_scan_workspace_bytes(int32_t x, int32_t y, int32_t z) {
  if (norm_validate(x, y, z) != 0) return -1;
  return (int64_t)norm_layout().total;
}

int mmnn_normalize_scan(const mmnn_normalize_desc* d, const void* scan, float* out, mmnn_normalize_result* result, void* ws, void* stream_) {
  MMNN_REQUIRE(d, "normalize_scan: null descriptor");
  if (norm_validate(d->x, d->y, d->z) != 0) return 1;
  const int ssz = ig_type_size(d->scan_type);
  MMNN_REQUIRE(ssz != 0, "normalize_scan: unsupported scan datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->scan_type);
  MMNN_REQUIRE(std::isfinite(d->scale) && d->scale > 0.0, "normalize_scan: scale must be finite and positive");
  MMNN_REQUIRE(std::isfinite(d->outliers) && d->outliers >= 0.0, "normalize_scan: outliers must be finite and not negative");
  MMNN_REQUIRE(scan && out && result && ws, "normalize_scan: null argument");
  MMNN_REQUIRE((uintptr_t)scan % ssz == 0, "normalize_scan: scan buffer not aligned to its element size (misaligned)");
  MMNN_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)result % 8 == 0 && (uintptr_t)out % 4 == 0, "normalize_scan: misaligned workspace / result / out");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const NormLayout L = norm_layout();
  char* wsb = static_cast<char*>(ws);
  NormArgs a{};
  a.scan = scan; a.out = out; a.result = result;
  a.part = reinterpret_cast<double*>(wsb + L.part);
  a.part2 = reinterpret_cast<double*>(wsb + L.part2);
  a.bad = reinterpret_cast<long long*>(wsb + L.bad);
  a.n = (long)d->x * d->y * d->z;
  const long chunks = (a.n + NM_TPB - 1) / NM_TPB;
  a.parts = chunks < NM_MAX_PARTS ? (int)chunks : NM_MAX_PARTS;
  a.code = d->scan_type;
  a.sc = rad_scale(d->scan_slope, d->scan_inter);
  a.scale = d->scale;
  a.bound = d->outliers * d->scale;
  MMNN_LAUNCH(norm_sum_kernel<0>, dim3((unsigned)a.parts), dim3(NM_TPB), 0, stream, a);
  MMNN_LAUNCH(norm_sum_kernel<1>, dim3((unsigned)a.parts), dim3(NM_TPB), 0, stream, a);
  MMNN_LAUNCH(norm_write_kernel, dim3((unsigned)(chunks < NM_WRITE_GROUPS ? chunks : NM_WRITE_GROUPS)), dim3(NM_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int64_t mmnn_resample_pair_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t mx, int32_t my, int32_t mz) {
  if (res_validate(x, y, z, mx, my, mz) != 0) return -1;
  return (int64_t)res_layout(x, y, z, mx, my).total;
}

int mmnn_resample_pair(const mmnn_resample_desc* d, const void* scan, const void* mask, const mmnn_resample_entry* tables_host,
                       const mmnn_resample_entry* tables, float* out, uint8_t* out_mask, void* ws, void* stream_) {
  MMNN_REQUIRE(d, "resample_pair: null descriptor");
  if (res_validate(d->x, d->y, d->z, d->mx, d->my, d->mz) != 0) return 1;
  const int ssz = ig_type_size(d->scan_type), msz = ig_type_size(d->mask_type);
  MMNN_REQUIRE(ssz != 0, "resample_pair: unsupported scan datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->scan_type);
  MMNN_REQUIRE(msz != 0, "resample_pair: unsupported mask datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->mask_type);
  MMNN_REQUIRE(std::isfinite(d->pole) && std::isfinite(d->pole_gain) && std::isfinite(d->gain), "resample_pair: a non-finite prefilter constant");
  for (int k = 0; k < RS_H; ++k) MMNN_REQUIRE(std::isfinite(d->pole_power[k]), "resample_pair: pole_power[%d] is not finite", k);
  MMNN_REQUIRE(scan && mask && tables_host && tables && out && out_mask && ws, "resample_pair: null argument");
  MMNN_REQUIRE((uintptr_t)scan % ssz == 0 && (uintptr_t)mask % msz == 0, "resample_pair: scan / mask buffer not aligned to its element size (misaligned)");
  MMNN_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)tables % 8 == 0 && (uintptr_t)tables_host % 8 == 0 && (uintptr_t)out % 4 == 0,
               "resample_pair: misaligned workspace / tables / out");
  const int n[3] = {d->x, d->y, d->z}, m[3] = {d->mx, d->my, d->mz};
  const mmnn_resample_entry* e = tables_host;
  for (int ax = 0; ax < 3; ++ax)
    for (int j = 0; j < m[ax]; ++j, ++e) {
      for (int k = 0; k < 4; ++k) {
        MMNN_REQUIRE(e->i[k] >= 0 && e->i[k] < n[ax], "resample_pair: table of axis %d, entry %d: source index %d outside 0..%d", ax, j, e->i[k], n[ax] - 1);
        MMNN_REQUIRE(std::isfinite(e->w[k]), "resample_pair: table of axis %d, entry %d: weight %d is not finite", ax, j, k);
      }
      MMNN_REQUIRE(e->nearest >= 0 && e->nearest < n[ax], "resample_pair: table of axis %d, entry %d: nearest index %d outside 0..%d", ax, j, e->nearest, n[ax] - 1);
    }
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const ResLayout L = res_layout(d->x, d->y, d->z, d->mx, d->my);
  char* wsb = static_cast<char*>(ws);
  ResArgs a{};
  a.scan = scan; a.mask = mask; a.out = out; a.omask = out_mask;
  a.tab[0] = tables; a.tab[1] = tables + d->mx; a.tab[2] = tables + d->mx + d->my;
  a.coef = reinterpret_cast<double*>(wsb + L.coef);
  a.t1 = reinterpret_cast<double*>(wsb + L.t1);
  a.t2 = reinterpret_cast<double*>(wsb + L.t2);
  a.X = d->x; a.Y = d->y; a.Z = d->z; a.MX = d->mx; a.MY = d->my; a.MZ = d->mz;
  a.scode = d->scan_type; a.mcode = d->mask_type;
  a.ss = rad_scale(d->scan_slope, d->scan_inter);
  a.ms = rad_scale(d->mask_slope, d->mask_inter);
  a.pole = d->pole; a.pole_gain = d->pole_gain; a.gain = d->gain;
  for (int k = 0; k < RS_H; ++k) a.zpow[k] = d->pole_power[k];
  const long lines = (long)d->y * d->z;
  // every grid is below 2^31 workgroups: each workgroup owns at least one element of an array of fewer than 2^31
  MMNN_LAUNCH(rs_prefilter_x_kernel, dim3((unsigned)cdiv(lines, RS_XL)), dim3(RS_XC), 0, stream, a);
  if (d->y > 1) MMNN_LAUNCH(rs_prefilter_line_kernel<0>, dim3((unsigned)cdiv((long)d->x * d->z, RS_TPB)), dim3(RS_TPB), 0, stream, a);
  if (d->z > 1) MMNN_LAUNCH(rs_prefilter_line_kernel<1>, dim3((unsigned)cdiv((long)d->x * d->y, RS_TPB)), dim3(RS_TPB), 0, stream, a);
  MMNN_LAUNCH(rs_eval_kernel<0>, dim3((unsigned)cdiv((long)d->mx * d->y * d->z, RS_TPB)), dim3(RS_TPB), 0, stream, a);
  MMNN_LAUNCH(rs_eval_kernel<1>, dim3((unsigned)cdiv((long)d->mx * d->my * d->z, RS_TPB)), dim3(RS_TPB), 0, stream, a);
  MMNN_LAUNCH(rs_eval_z_kernel, dim3((unsigned)((long)cdiv((long)d->mx * d->my, RS_TPB) * cdiv(d->mz, RS_ZRUN))), dim3(RS_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
