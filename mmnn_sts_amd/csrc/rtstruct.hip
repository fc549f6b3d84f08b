// RTSTRUCT contours -> a 0 / 1 byte mask on the scan's grid (the contract is the comment above mmnn_rasterize_contours in
// include/mmnn_sts.h).  A scanline fill: a row tests the edges of its slice once, finds the few that cross it and XORs `i < xc` over
// the voxels of the row; no voxel loops over edges, nothing is accumulated in global memory.
//
//   rasterize_kernel  one workgroup of RC_TPB threads (four waves) = one slice, a band of RC_BAND rows and an x span of RC_SPAN voxels;
//                     grid = x spans * bands * slices, flat.  The slice's edges (contour after contour, each closed from its last point
//                     to its first) are staged into LDS in chunks of MMNN_RASTERIZE_CHUNK_EDGES as (x0, y0, x1, y1) in fp64, together
//                     with the chunk's y range, so that a row above or below every edge of the chunk skips it.  A wave takes rows
//                     wave, wave + 4, ... of the band.  For a row its lanes stride over the staged edges; of each group of 64 the ones
//                     that cross the row put their crossing abscissa into the wave's LDS list (ballot + prefix popcount: at most 64
//                     entries, so the list cannot overflow), and every lane then XORs the list into the 16 parity bits of the 16
//                     consecutive voxels it owns.  For integer i, `i < xc` is `i < ceil(xc)`, exactly: a crossing flips the first
//                     clamp(ceil(xc) - i0, 0, 16) of a lane's voxels, one mask instead of 16 comparisons.  The parity bits of the
//                     band's rows stay in registers across the chunks of a slice; at the end a lane stores its 16 bytes at once.
//                     The lanes' groups are aligned to 16 bytes of the ADDRESS, not of the row: a row that starts `s` bytes past a
//                     16-byte boundary shifts its groups left by s, and only the groups cut by the span's or the row's ends fall back
//                     to byte stores.  That is why a span is 1008 = 1024 - 16 voxels.  Every byte of the slice is written, also when
//                     the slice has no contours.  A slice of many tiny contours (one rectangle per run of voxels, as the synthetic
//                     writer makes them) stages them one after the other: correct, not fast; a drawn contour has hundreds of points.
//                     Contour records that point outside `points` and slice ranges outside `contours` are ignored, not followed.
#include "../../include/mmnn_sts.h"
#include "common.hpp"
#include "mask_bytes.hpp"
#include "reduce.hpp"

#include <cmath>

namespace mmnn {

constexpr int RC_WAVES = 4;
constexpr int RC_TPB = 64 * RC_WAVES;
constexpr int RC_ROWS = 8;                              // rows per wave
constexpr int RC_BAND = RC_ROWS * RC_WAVES;             // rows per workgroup
constexpr int RC_SPAN = 64 * 16 - 16;                   // voxels per workgroup along x (see above)
constexpr int RC_CHUNK = MMNN_RASTERIZE_CHUNK_EDGES;

struct RcArgs {
  const double* points;                     // [n_points][2]
  const int* contours;                      // [n_contours][2]
  const int* slice_first;                   // [Z + 1]
  uint8_t* out;
  long n_points;
  int n_contours;
  int X, Y, Z;
  int nx, nbands;
};

// the first voxel of the lane's 16-byte group in the row that starts at `row`: the group is aligned in memory (i0 may be below 0 or
// below the span's first voxel; the caller cuts it to the span and the row)
__device__ __forceinline__ int rc_group_start(const uint8_t* row, int span0, int lane) {
  return span0 - (int)((uintptr_t)(row + span0) & 15) + lane * 16;
}

__global__ void __launch_bounds__(RC_TPB) rasterize_kernel(const RcArgs a) {
  __shared__ double ex0[RC_CHUNK], ey0[RC_CHUNK], ex1[RC_CHUNK], ey1[RC_CHUNK];
  __shared__ double xlist[RC_WAVES][64];
  __shared__ double yred[2 * RC_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned b = blockIdx.x;
  const int span0 = (int)(b % (unsigned)a.nx) * RC_SPAN;
  b /= (unsigned)a.nx;
  const int band0 = (int)(b % (unsigned)a.nbands) * RC_BAND;
  const int k = (int)(b / (unsigned)a.nbands);
  uint8_t* const slice = a.out + (long)k * a.Y * a.X;

  unsigned bits[RC_ROWS];
#pragma unroll
  for (int r = 0; r < RC_ROWS; ++r) bits[r] = 0u;

  int c = a.slice_first[k], c1 = a.slice_first[k + 1];
  if (c < 0) c = 0;
  if (c1 > a.n_contours) c1 = a.n_contours;
  int e0 = 0;                               // edges of contour c already staged
  while (true) {
    // ---- stage up to one chunk of edges, contour after contour
    int fill = 0;
    double yr[2] = {INFINITY, -INFINITY};    // min, max of the chunk's y
    while (c < c1 && fill < RC_CHUNK) {
      const long first = a.contours[2 * c];
      int n = a.contours[2 * c + 1];
      if (first < 0 || n < 0 || first + n > a.n_points) n = 0;
      int take = n - e0;
      if (take > RC_CHUNK - fill) take = RC_CHUNK - fill;
      for (int t = tid; t < take; t += RC_TPB) {
        const int e = e0 + t;
        const long p = first + e, q = first + (e + 1 == n ? 0 : e + 1);
        const double x0 = a.points[2 * p], y0 = a.points[2 * p + 1], x1 = a.points[2 * q], y1 = a.points[2 * q + 1];
        ex0[fill + t] = x0; ey0[fill + t] = y0; ex1[fill + t] = x1; ey1[fill + t] = y1;
        yr[0] = fmin(yr[0], fmin(y0, y1));
        yr[1] = fmax(yr[1], fmax(y0, y1));
      }
      if (take > 0) { fill += take; e0 += take; }
      if (e0 >= n) { ++c; e0 = 0; }
    }
    if (fill == 0) break;
    // ---- the chunk's y range
    block_reduce<RC_WAVES>(yr, yred, FMinMax{});     // (its barriers also publish the staged edges)
    const double lo = yr[0], hi = yr[1];
    // ---- the band's rows against the chunk
#pragma unroll
    for (int r = 0; r < RC_ROWS; ++r) {
      const int j = band0 + r * RC_WAVES + wave;
      const double dj = (double)j;
      if (j < a.Y && lo <= dj && dj < hi) {                    // (wave-uniform)
        const double di0 = (double)rc_group_start(slice + (long)j * a.X, span0, lane);
        for (int g = 0; g < fill; g += 64) {
          const int e = g + lane;
          bool cross = false;
          double xc = 0.0;
          if (e < fill) {
            const double y0 = ey0[e], y1 = ey1[e];
            cross = (y0 <= dj && dj < y1) || (y1 <= dj && dj < y0);
            if (cross) {
              const double x0 = ex0[e];
              xc = __dadd_rn(x0, __ddiv_rn(__dmul_rn(__dsub_rn(dj, y0), __dsub_rn(ex1[e], x0)), __dsub_rn(y1, y0)));
            }
          }
          const unsigned long long m = __ballot(cross);
          if (m != 0ull) {                                     // (wave-uniform)
            if (cross) xlist[wave][__popcll(m & ((1ull << lane) - 1ull))] = xc;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int cnt = __popcll(m);
            for (int q = 0; q < cnt; ++q) {
              // voxels i0 .. i0 + 15: i < xc for the first clamp(ceil(xc) - i0, 0, 16) of them (a NaN crossing flips none)
              const int nset = (int)fmin(fmax(__dsub_rn(ceil(xlist[wave][q]), di0), 0.0), 16.0);
              bits[r] ^= (1u << nset) - 1u;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
          }
        }
      }
    }
    if (c >= c1) break;
    __syncthreads();                        // every wave is done with the chunk before the next one is staged
  }

  // ---- the band's rows: 16 bytes per lane
  int span1 = span0 + RC_SPAN;
  if (span1 > a.X) span1 = a.X;
#pragma unroll
  for (int r = 0; r < RC_ROWS; ++r) {
    const int j = band0 + r * RC_WAVES + wave;
    if (j >= a.Y) continue;
    uint8_t* const row = slice + (long)j * a.X;
    const int i0 = rc_group_start(row, span0, lane);
    const int ib = i0 > span0 ? i0 : span0, ie = i0 + 16 < span1 ? i0 + 16 : span1;
    if (ib >= ie) continue;
    store_mask_bits(row + i0, ib - i0, ie - i0, bits[r], 1u);
  }
}

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int mmnn_rasterize_contours(const mmnn_rasterize_desc* d, const double* points, const int32_t* contours, const int32_t* slice_first,
                            uint8_t* out, void* stream_) {
  MMNN_REQUIRE(d, "rasterize_contours: null descriptor");
  MMNN_REQUIRE(d->x >= 1 && d->y >= 1 && d->z >= 1, "rasterize_contours: non-positive extent %d x %d x %d", d->x, d->y, d->z);
  MMNN_REQUIRE(d->x <= MMNN_INGEST_MAX_X, "rasterize_contours: x extent %d above %d", d->x, MMNN_INGEST_MAX_X);
  MMNN_REQUIRE(d->n_contours >= 0, "rasterize_contours: n_contours %d is negative", d->n_contours);
  MMNN_REQUIRE(d->n_points >= 0, "rasterize_contours: n_points %lld is negative", (long long)d->n_points);
  MMNN_REQUIRE(slice_first && out, "rasterize_contours: null argument");
  MMNN_REQUIRE(d->n_contours == 0 || (points && contours), "rasterize_contours: %d contours and a null points / contours pointer", d->n_contours);
  MMNN_REQUIRE((uintptr_t)points % sizeof(double) == 0 && (uintptr_t)contours % sizeof(int32_t) == 0 && (uintptr_t)slice_first % sizeof(int32_t) == 0,
               "rasterize_contours: points / contours / slice_first not aligned to their element size");
  const int nx = cdiv(d->x, RC_SPAN), nbands = cdiv(d->y, RC_BAND);
  MMNN_REQUIRE((double)nx * nbands * d->z < 2147483648.0, "rasterize_contours: extent %d x %d x %d needs 2^31 workgroups or more", d->x, d->y, d->z);
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  RcArgs a{};
  a.points = points; a.contours = contours; a.slice_first = slice_first; a.out = out;
  a.n_points = d->n_points; a.n_contours = d->n_contours;
  a.X = d->x; a.Y = d->y; a.Z = d->z;
  a.nx = nx; a.nbands = nbands;
  MMNN_LAUNCH(rasterize_kernel, dim3((unsigned)(nx * nbands * d->z)), dim3(RC_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
