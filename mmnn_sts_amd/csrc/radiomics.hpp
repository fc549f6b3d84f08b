// What csrc/radiomics.hip, csrc/radiomics_texture.hip, csrc/radiomics_zones.hip and csrc/radiomics_mesh.hip share: the constants, the 13 directions, the state
// block that the kernels of `mmnn_radiomics` leave in the workspace, the workspace layout, the extent checks, the prologue of the follow-on
// calls (their descriptor checks and what they read of the first call), the wave-folded count and (with csrc/radiomics_filter.hip) the
// descriptor's slope / inter rule.
// Their fp64 sums over a workgroup are block_reduce<RAD_TPB / 64>(values, lds, Sum{}) of reduce.hpp: lanes by the butterfly, then the
// waves in index order.
#pragma once
#include "../../include/mmnn_sts.h"
#include "common.hpp"
#include "ingest_load.hpp"
#include "reduce.hpp"

#include <cmath>

namespace mmnn {

constexpr int RAD_TPB = 256;
constexpr int RAD_MAX_PARTS = 256;          // workgroups of a voxel pass (the fixed partition of the fp64 sums)
constexpr int RAD_SLOTS = 24;               // 64-bit partial results per workgroup and pass
constexpr int RAD_RANKS = 10;
constexpr int RAD_DIGITS = 65536;           // 16-bit radix digits: four passes over the 64-bit key
constexpr int RAD_LDS_NG = 128;             // the LDS matrix: RAD_LDS_NG^2 * 4 B = 64 KiB of the CU's 160, two workgroups per CU
constexpr int RAD_DIRS = MMNN_RADIOMICS_DIRECTIONS;
constexpr int RAD_GLCM_CHUNKS = 64;         // workgroups per direction in glcm_count_kernel
constexpr int RAD_NF = MMNN_RADIOMICS_GLCM;
constexpr int RAD_MAX_BINS = MMNN_RADIOMICS_MAX_BINS;
constexpr double RAD_EPS = 2.220446049250313e-16;   // 2^-52

#if defined(__HIPCC__)
static __constant__ int rad_dirs[RAD_DIRS][3] = {      // (dz, dy, dx), first non-zero component positive, lexicographic
    {0, 0, 1}, {0, 1, -1}, {0, 1, 0}, {0, 1, 1}, {1, -1, -1}, {1, -1, 0}, {1, -1, 1}, {1, 0, -1}, {1, 0, 0}, {1, 0, 1}, {1, 1, -1},
    {1, 1, 0}, {1, 1, 1}};
#endif

struct RadState {
  long long n;
  int flagged;                              // overflow | nonfinite | empty
  int n_bins;
  double low, bw, mean, vmin, vmax, sum, sumsq;
  double cen[4];                            // sum |d|, d^2, d^3, d^4
  long long rob_n;
  double rob_sum, rob_mean, rob_abs;
  double p10, p90;
  unsigned long long prefix[RAD_RANKS];
  unsigned long long rank[RAD_RANKS];       // rank among the values that share the prefix
  int rep[RAD_RANKS];                       // the first rank with the same prefix: its histogram is the one that is filled
};

#if defined(__HIPCC__)
__device__ __forceinline__ double rad_plogp(double p) { return p * log2(p + RAD_EPS); }

// The quiet NaN that fills a result block when a flag is set or a matrix is empty.
__device__ __forceinline__ double rad_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// A flat voxel index (x fastest) -> (x, y, z) by two 32-bit divisions; XY = X * Y (x * y * z < 2^31).
__device__ __forceinline__ void rad_split(unsigned idx, unsigned X, unsigned XY, int& x, int& y, int& z) {
  const unsigned zq = idx / XY, r = idx - zq * XY, yq = r / X;
  x = (int)(r - yq * X);
  y = (int)yq;
  z = (int)zq;
}

// One count per active lane into h[digit].  Called by whole waves; a wave whose active lanes agree sends one add of their number.
__device__ __forceinline__ void rad_count(unsigned* h, unsigned digit, bool active) {
  const unsigned long long m = __ballot(active);
  if (m == 0ull) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
  const unsigned d0 = (unsigned)__shfl((int)digit, leader, 64);
  if (__ballot(active && digit != d0) == 0ull) {
    if (lane == leader) atomicAdd(&h[d0], (unsigned)__popcll(m));
  } else if (active) {
    atomicAdd(&h[digit], 1u);
  }
}
#endif

struct RadLayout { size_t state, part, rhist, dirf, bins, total; };

inline RadLayout rad_layout(long n) {
  RadLayout L;
  Carver cv;
  L.state = cv.take(sizeof(RadState));
  L.part = cv.take((size_t)RAD_SLOTS * RAD_MAX_PARTS * 8);
  L.rhist = cv.take((size_t)RAD_RANKS * RAD_DIGITS * 4);
  L.dirf = cv.take((size_t)RAD_DIRS * (RAD_NF + 1) * 8);
  L.bins = cv.take((size_t)n * 2);
  L.total = cv.cur;
  return L;
}

// The fp64 slope / inter pair of a descriptor, as ig_scale reads a header's pair.
inline IgScale rad_scale(double slope, double inter) {
  IgScale s{1.0, 0.0, 0};
  if (slope == 0.0 || !std::isfinite(slope)) return s;
  s.slope = slope;
  s.inter = std::isfinite(inter) ? inter : 0.0;
  s.on = !(s.slope == 1.0 && s.inter == 0.0);
  return s;
}

inline int rad_validate(int x, int y, int z, int max_bins) {
  MMNN_REQUIRE(x >= 1 && y >= 1 && z >= 1, "radiomics: non-positive extent %d x %d x %d", x, y, z);
  MMNN_REQUIRE((double)x * y * z < 2147483648.0, "radiomics: extent %d x %d x %d holds 2^31 voxels or more", x, y, z);
  MMNN_REQUIRE(max_bins >= 1 && max_bins <= RAD_MAX_BINS, "radiomics: max_bins %d outside 1..%d", max_bins, RAD_MAX_BINS);
  return 0;
}

// What a follow-on call (texture, zones, mesh) requires of the descriptor the first call ran under; `who` prefixes the message.
inline int rad_validate_follow(const char* who, const mmnn_radiomics_desc* d) {
  MMNN_REQUIRE(d, "%s: null descriptor", who);
  if (rad_validate(d->x, d->y, d->z, d->max_bins) != 0) return 1;
  MMNN_REQUIRE(ig_type_size(d->scan_type) != 0, "%s: unsupported scan datatype code %d", who, d->scan_type);
  MMNN_REQUIRE(ig_type_size(d->mask_type) != 0, "%s: unsupported mask datatype code %d", who, d->mask_type);
  MMNN_REQUIRE(std::isfinite(d->bin_width) && d->bin_width > 0.0, "%s: bin_width must be finite and positive", who);
  return 0;
}

// What every follow-on call reads of the first one: the bin volume (0 outside the ROI) and the state block in its workspace, the extents.
struct RadFollow {
  const uint16_t* bins;                     // [Z][Y][X]
  const RadState* st;
  int X, Y, Z;
  unsigned N;                               // X * Y * Z
};

inline RadFollow rad_follow(const mmnn_radiomics_desc* d, const void* ws) {
  const long n = (long)d->x * d->y * d->z;
  const RadLayout R = rad_layout(n);
  const char* wsb = static_cast<const char*>(ws);
  return RadFollow{reinterpret_cast<const uint16_t*>(wsb + R.bins), reinterpret_cast<const RadState*>(wsb + R.state), d->x, d->y, d->z,
                   (unsigned)n};
}

}  // namespace mmnn
