// Scan ingest: one raw NIfTI scan and its mask -> one S^3 fp32 channel plane, as upstream's image datasets prepare it per patient and
// modality (data/ImageDatasets.py:431-470, :599-637): image * mask, every all-zero slice dropped along each axis, area resize to S^3.
// S is a run-time argument of the kernels, 1..MMNN_INGEST_MAX_SIZE, and MMNN_INGEST_SIZE = 64 (upstream's) where the caller names none;
// no kernel is specialised on it, so an S = 64 call runs the one code every other S runs.
// The contract is the comment above mmnn_ingest_volume in include/mmnn_sts.h.  Neither a float copy nor a cropped copy of the volume
// is ever written: the scan and the mask are read in their on-disk types, twice (the second time only inside the kept region).
//
//   memset                the occupancy flags of the three axes
//   ingest_flags_kernel   pass A, over the whole scan and mask: flag_x[x] / flag_y[y] / flag_z[z] = 1 where a voxel with !(v == 0) lies.
//                         Lanes along x, each a fixed group of x columns whose flags it keeps in registers over all its rows; a wave
//                         covers one row segment at a time, so the y and z flags are reduced with one ballot and written by one lane.
//                         Every writer writes the constant 1: ordinary stores, no atomics.
//   ingest_scan_kernel    pass B, one workgroup: exclusive scans of the flags -> kept-index lists and the extents M.
//   ingest_area_kernel    pass C: a wave per output (b, c) = (y window, z window).  Lanes along the kept x indices sum v over the rows of
//                         the window in fp64 (registers), leave one column sum per kept x in LDS, and then a lane adds the columns of
//                         each of its x windows a = lane, lane + 64, ... < S, divides by the window's voxel count and rounds once to fp32.
// v is formed identically in passes A and C (`ingest_value`): a rounded multiply and a rounded add, never an FMA -- whether a voxel is
// exactly zero decides which slices survive.
//
//   resample_mask_kernel  mmnn_resample_mask, a call of its own ahead of the three passes when the mask was drawn on another grid:
//                         sitk.Resample(mask, image) with its defaults, then upstream's rebinarisation, to one byte per scan voxel.
//   maps_taps_kernel, maps_to_scan_kernel   mmnn_maps_to_scan, the inverse path: S^3 maps of the model back onto the scan's grid,
//                         by the kept-index lists that pass B left in the workspace.
#include "../../include/mmnn_sts.h"
#include "area.hpp"
#include "common.hpp"
#include "ingest_load.hpp"

#include <cmath>

namespace mmnn {

constexpr int IG_WAVES = 4;                 // waves per block in passes A and C
constexpr int IG_TPB = 64 * IG_WAVES;
constexpr int IG_SCAN_TPB = 256;

struct IgArgs {
  const void* scan; const void* mask;
  int X, Y, Z;
  int stype, mtype;                         // NIfTI datatype codes
  IgScale ss, ms;
  unsigned* flag_x; unsigned* flag_y; unsigned* flag_z;     // [X], [Y], [Z]
  int* kept_x; int* kept_y; int* kept_z;                    // kept indices in ascending order, the first M[axis] entries valid
  int* M;                                                   // [3]
  int* extents;                                             // the caller's copy of M
  float* out;                                               // [S][S][S]
  int S;                                                    // output extent per axis
};

__device__ __forceinline__ double ingest_value(double sraw, double mraw, const IgScale& ss, const IgScale& ms) {
  return __dmul_rn(ig_scaled(sraw, ss), ig_scaled(mraw, ms));
}

// ---- pass A ------------------------------------------------------------------------------------------------------------------
// grid (x groups of 64 * VEC columns, row blocks); block (64, IG_WAVES): threadIdx.y picks the row, a wave = one row segment
template <int VEC>
__global__ void __launch_bounds__(IG_TPB) ingest_flags_kernel(const IgArgs a) {
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * VEC;
  const bool in_x = x0 < a.X;                       // VEC > 1 only when X % VEC == 0: a group is inside or outside as a whole
  const int R = a.Y * a.Z;
  bool nzx[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) nzx[k] = false;
  for (int r = blockIdx.y * IG_WAVES + threadIdx.y; r < R; r += gridDim.y * IG_WAVES) {
    bool any = false;
    if (in_x) {
      const long idx = (long)r * a.X + x0;
      double s[VEC], m[VEC];
      ig_load<VEC>(a.scan, a.stype, idx, s);
      ig_load<VEC>(a.mask, a.mtype, idx, m);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool nz = !(ingest_value(s[k], m[k], a.ss, a.ms) == 0.0);
        nzx[k] |= nz;
        any |= nz;
      }
    }
    if (__ballot(any) != 0ull && threadIdx.x == 0) {   // r = y + Y z is the same in the whole wave
      a.flag_y[r % a.Y] = 1u;
      a.flag_z[r / a.Y] = 1u;
    }
  }
  if (in_x) {
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      if (nzx[k]) a.flag_x[x0 + k] = 1u;
  }
}

// ---- pass B ------------------------------------------------------------------------------------------------------------------
// one block: kept[pos] = i for every i with flag[i] != 0, pos = number of flagged indices below i; returns the count (in every thread)
__device__ int ig_compact(const unsigned* flag, int n, int* kept, int* lds) {
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += IG_SCAN_TPB) {
    const int i = c0 + threadIdx.x;
    const int f = (i < n && flag[i] != 0u) ? 1 : 0;
    __syncthreads();
    lds[threadIdx.x] = f;
    __syncthreads();
    // inclusive Hillis-Steele scan of IG_SCAN_TPB entries
    for (int o = 1; o < IG_SCAN_TPB; o <<= 1) {
      const int add = (int)threadIdx.x >= o ? lds[threadIdx.x - o] : 0;
      __syncthreads();
      lds[threadIdx.x] += add;
      __syncthreads();
    }
    const int incl = lds[threadIdx.x];
    if (f) kept[base + incl - 1] = i;
    base += lds[IG_SCAN_TPB - 1];
  }
  return base;
}

__global__ void __launch_bounds__(IG_SCAN_TPB) ingest_scan_kernel(const IgArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ig_smem[];
  int* lds = reinterpret_cast<int*>(ig_smem);
  const int mx = ig_compact(a.flag_x, a.X, a.kept_x, lds);
  const int my = ig_compact(a.flag_y, a.Y, a.kept_y, lds);
  const int mz = ig_compact(a.flag_z, a.Z, a.kept_z, lds);
  if (threadIdx.x == 0) {
    a.M[0] = mx; a.M[1] = my; a.M[2] = mz;
    a.extents[0] = mx; a.extents[1] = my; a.extents[2] = mz;
  }
}

// ---- pass C ------------------------------------------------------------------------------------------------------------------
// grid (cdiv(S, IG_WAVES), S): blockIdx.y = b (y window), wave w of block blockIdx.x = c (z window); a wave with c >= S (the last
// block when IG_WAVES does not divide S) only takes part in the barrier.  Dynamic LDS: IG_WAVES * X doubles.
__global__ void __launch_bounds__(IG_TPB) ingest_area_kernel(const IgArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ig_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* col = reinterpret_cast<double*>(ig_smem) + (long)wave * a.X;
  const int S = a.S;
  const int b = blockIdx.y, c = blockIdx.x * IG_WAVES + wave;
  const bool owns = c < S;                                      // (wave-uniform)
  const int mx = a.M[0], my = a.M[1], mz = a.M[2];
  float* dst = a.out + (long)b * S + c;                         // + xa S S for x window xa
  if (mx == 0 || my == 0 || mz == 0) {                          // the mask misses the scan: zeros (the extents tell the caller)
    if (owns)
      for (int xa = lane; xa < S; xa += 64) dst[(long)xa * S * S] = 0.f;
    return;
  }
  int yb, ye, zb, ze;
  area_window(b, my, S, 0, yb, ye);
  area_window(c, mz, S, 0, zb, ze);                             // (clamped to the last window when c >= S; not used then)
  for (int j = lane; owns && j < mx; j += 64) {
    const long x = a.kept_x[j];
    double acc = 0.0;
    for (int zi = zb; zi < ze; ++zi) {
      const long zrow = (long)a.kept_z[zi] * a.Y;
#pragma unroll 4
      for (int yi = yb; yi < ye; ++yi) {
        const long idx = (zrow + a.kept_y[yi]) * a.X + x;
        double s[1], m[1];
        ig_load<1>(a.scan, a.stype, idx, s);
        ig_load<1>(a.mask, a.mtype, idx, m);
        acc += ingest_value(s[0], m[0], a.ss, a.ms);
      }
    }
    col[j] = acc;
  }
  __syncthreads();     // (every wave of the block arrives: mx, my, mz are block-uniform, and nothing above returns once they are non-zero)
  if (!owns) return;
  for (int xa = lane; xa < S; xa += 64) {                       // x windows of this lane
    int xb, xe;
    area_window(xa, mx, S, 0, xb, xe);
    double sum = 0.0;
    for (int j = xb; j < xe; ++j) sum += col[j];
    const double count = (double)(xe - xb) * (double)(ye - yb) * (double)(ze - zb);
    dst[(long)xa * S * S] = (float)(sum / count);
  }
}

// ---- mask resample -------------------------------------------------------------------------------------------------------------
// A mask drawn on another grid -> bytes on the scan's grid (the contract is the comment above mmnn_resample_mask in the header).
// grid and block as pass A: lanes along x, VEC output voxels per lane, a wave = one row segment; the (j, k) part of the three mask
// coordinates is formed once per row.  The mask is small and each of its voxels is gathered by up to 8 * (spacing ratio)^3 scan voxels:
// plain cached loads.  Every output byte is written, with ordinary vector stores (one dword per lane when VEC = 4).
struct RsArgs {
  const void* mask;
  uint8_t* out;
  int X, Y, Z;                              // scan grid = output grid
  int MX, MY, MZ;                           // mask grid
  IgScale ms;
  double T[12];                             // rows of the 3x4 scan-index -> mask-index matrix
  double thr;
};

// SCALED: whether the mask's slope / inter apply (the same in every lane; a template parameter so that the unscaled kernel carries
// neither the multiply-add nor the select)
template <typename T, bool SCALED>
__device__ __forceinline__ double rs_value(const T* m, unsigned idx, const IgScale& s) {
  const double raw = (double)m[idx];
  return SCALED ? __dadd_rn(__dmul_rn(raw, s.slope), s.inter) : raw;
}

template <typename T, bool SCALED>
__device__ __forceinline__ uint8_t rs_voxel(const RsArgs& a, double cx, double cy, double cz) {
  // ITK's buffer test on the continuous index (a NaN or infinite coordinate fails it)
  const bool inside = cx >= -0.5 && cx < (double)a.MX - 0.5 && cy >= -0.5 && cy < (double)a.MY - 0.5 && cz >= -0.5 && cz < (double)a.MZ - 0.5;
  if (!inside) return 0;
  const double fx = floor(cx), fy = floor(cy), fz = floor(cz);
  const double wx = cx - fx, wy = cy - fy, wz = cz - fz;
  // neighbour indices clamped to the grid: inside, floor(c_r) lies in [-1, m_r - 1], so one bound each is left to apply.  Every
  // element index is below mx * my * mz < 2^31, so 32-bit arithmetic holds it, and the four rows of the 2 x 2 x 2 neighbourhood
  // differ from the first by 0 or one row (MX) and by 0 or one slice (MX * MY)
  const int gx = (int)fx, gy = (int)fy, gz = (int)fz;
  const int x0 = max(gx, 0), x1 = min(gx + 1, a.MX - 1);
  const int y0 = max(gy, 0), y1 = min(gy + 1, a.MY - 1);
  const int z0 = max(gz, 0), z1 = min(gz + 1, a.MZ - 1);
  const unsigned row = (unsigned)(z0 * a.MY + y0) * (unsigned)a.MX;
  const unsigned dy = y1 != y0 ? (unsigned)a.MX : 0u, dz = z1 != z0 ? (unsigned)a.MX * (unsigned)a.MY : 0u;
  const unsigned rows[2][2] = {{row, row + dy}, {row + dz, row + dz + dy}};
  const double ux[2] = {1.0 - wx, wx}, uy[2] = {1.0 - wy, wy}, uz[2] = {1.0 - wz, wz};
  const T* m = static_cast<const T*>(a.mask);
  // the eight-term blend, summed along x first: sum over (y, z) of uy uz (ux0 v0 + ux1 v1)
  double acc = 0.0;
#pragma unroll
  for (int kz = 0; kz < 2; ++kz)
#pragma unroll
    for (int ky = 0; ky < 2; ++ky) {
      const double v0 = rs_value<T, SCALED>(m, rows[kz][ky] + (unsigned)x0, a.ms), v1 = rs_value<T, SCALED>(m, rows[kz][ky] + (unsigned)x1, a.ms);
      acc += uy[ky] * uz[kz] * (ux[0] * v0 + ux[1] * v1);
    }
  return acc > a.thr ? 1 : 0;               // a NaN blend compares false: 0
}

template <typename T, int VEC, bool SCALED>
__device__ __forceinline__ void rs_rows(const RsArgs& a) {
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * VEC;
  if (x0 >= a.X) return;                    // VEC > 1 only when X % VEC == 0: a group is inside or outside as a whole
  const int R = a.Y * a.Z;
  for (int r = blockIdx.y * IG_WAVES + threadIdx.y; r < R; r += gridDim.y * IG_WAVES) {
    const double j = (double)(r % a.Y), k = (double)(r / a.Y);
    const double bx = a.T[1] * j + a.T[2] * k + a.T[3];
    const double by = a.T[5] * j + a.T[6] * k + a.T[7];
    const double bz = a.T[9] * j + a.T[10] * k + a.T[11];
    uint8_t b[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const double i = (double)(x0 + v);
      b[v] = rs_voxel<T, SCALED>(a, a.T[0] * i + bx, a.T[4] * i + by, a.T[8] * i + bz);
    }
    uint8_t* dst = a.out + (long)r * a.X + x0;
    if constexpr (VEC == 4) *reinterpret_cast<uint32_t*>(dst) = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    else *dst = b[0];
  }
}

template <int VEC, bool SCALED>
__device__ __forceinline__ void rs_dispatch(const RsArgs& a, int code) {
  switch (code) {
    case 2:   rs_rows<uint8_t, VEC, SCALED>(a); break;
    case 4:   rs_rows<int16_t, VEC, SCALED>(a); break;
    case 8:   rs_rows<int32_t, VEC, SCALED>(a); break;
    case 16:  rs_rows<float, VEC, SCALED>(a); break;
    case 64:  rs_rows<double, VEC, SCALED>(a); break;
    case 256: rs_rows<int8_t, VEC, SCALED>(a); break;
    case 512: rs_rows<uint16_t, VEC, SCALED>(a); break;
    default:  rs_rows<uint32_t, VEC, SCALED>(a); break;   // 768 (the host admits no other code)
  }
}

// the type code and the scaling switch are the same in every lane: two uniform branches per kernel, none per voxel
template <int VEC>
__global__ void __launch_bounds__(IG_TPB) resample_mask_kernel(const RsArgs a, const int code) {
  if (a.ms.on) rs_dispatch<VEC, true>(a, code);
  else rs_dispatch<VEC, false>(a, code);
}

// ---- maps to scan ----------------------------------------------------------------------------------------------------------------
// The way back: S^3 model-space maps -> fp32 volumes on the scan's grid (the contract is the comment above mmnn_maps_to_scan in the
// header).  The kept slices are the ingest's own: the kept-index lists and extents its pass B left in its workspace are read, never the
// scan or the mask.
//   maps_taps_kernel      one entry per scan index of each axis: the two map indices and the weight of its linear tap, or "dropped".
//                         The rank of an index is found by bisection of its axis' ascending kept list, so a thread writes its own
//                         entry only and every entry is written.
//   maps_to_scan_kernel   grid and block as pass A.  A wave owns a row (y, z); its lanes keep the x taps of their MS_XCH * VEC output
//                         voxels in registers over all rows.  Per row a lane loads the four (y tap, z tap) entries of each of its map
//                         x indices l = lane, lane + 64, ... < S -- the map's fastest axis is z, the output's is x, so a gather per
//                         output voxel would touch eight cache lines where this touches two per lane, index and row -- and blends
//                         them with the row's y and z weights into an S-entry fp64 line in LDS, one line per map; then every lane
//                         lerps its voxels along x from the line.  LDS: IG_WAVES * n_maps * S doubles, 64 KiB at 16 maps of 128^3 --
//                         the most a workgroup is given, and what caps S at MMNN_INGEST_MAX_SIZE.
//                         Dropped rows and dropped x indices are stored as zeros: every element of `out` is written.
struct MsTap {
  int i0, i1;                               // i0 < 0: the index is not in the kept list
  double w;
};

struct MsArgs {
  const int* kept_x; const int* kept_y; const int* kept_z;  // the ingest's workspace
  const int* M;
  MsTap* tx; MsTap* ty; MsTap* tz;                          // [X], [Y], [Z]
  const float* maps; float* out;
  int X, Y, Z, n_maps;
  int S;                                                    // extent per axis of the maps
};

constexpr int MS_XCH = 2;                   // x chunks of 64 * VEC voxels per block: 512 voxels of a row when VEC = 4

__device__ __forceinline__ MsTap ms_tap(const int* kept, int m, int n, int i, int S) {
  MsTap t{-1, -1, 0.0};
  m = min(max(m, 0), n);
  int lo = 0, hi = m;                       // the first position whose kept index is not below i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (kept[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  if (lo < m && kept[lo] == i) {
    const double s = fmax(((double)lo + 0.5) * (double)S / (double)m - 0.5, 0.0);
    t.i0 = min((int)floor(s), S - 1);
    t.i1 = min(t.i0 + 1, S - 1);
    t.w = s - (double)t.i0;
  }
  return t;
}

__global__ void __launch_bounds__(IG_SCAN_TPB) maps_taps_kernel(const MsArgs a) {
  const int i = blockIdx.x * IG_SCAN_TPB + threadIdx.x;
  if (i < a.X) a.tx[i] = ms_tap(a.kept_x, a.M[0], a.X, i, a.S);
  else if (i < a.X + a.Y) a.ty[i - a.X] = ms_tap(a.kept_y, a.M[1], a.Y, i - a.X, a.S);
  else if (i < a.X + a.Y + a.Z) a.tz[i - a.X - a.Y] = ms_tap(a.kept_z, a.M[2], a.Z, i - a.X - a.Y, a.S);
}

// grid (x groups of MS_XCH * 64 * VEC columns, row blocks); block (64, IG_WAVES).  Dynamic LDS: IG_WAVES * n_maps * S doubles.
template <int VEC>
__global__ void __launch_bounds__(IG_TPB) maps_to_scan_kernel(const MsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ig_smem[];
  const int lane = threadIdx.x, wave = threadIdx.y;
  const int S = a.S;
  const long S2 = (long)S * S, S3 = S2 * S;
  double* line = reinterpret_cast<double*>(ig_smem) + wave * a.n_maps * S;
  MsTap t[MS_XCH][VEC];
  int x0[MS_XCH];
#pragma unroll
  for (int c = 0; c < MS_XCH; ++c) {
    x0[c] = ((blockIdx.x * MS_XCH + c) * 64 + lane) * VEC;   // VEC > 1 only when X % VEC == 0: a group is inside or outside as a whole
#pragma unroll
    for (int k = 0; k < VEC; ++k) t[c][k] = x0[c] < a.X ? a.tx[x0[c] + k] : MsTap{-1, -1, 0.0};
  }
  const long R = (long)a.Y * a.Z, V = R * a.X;
  // the trip count is the same in every wave of the block (the barriers): a wave past the last row only waits
  for (long r0 = (long)blockIdx.y * IG_WAVES; r0 < R; r0 += (long)gridDim.y * IG_WAVES) {
    const long r = r0 + wave;                         // r = y + Y z
    bool live = false;
    if (r < R) {
      const MsTap ty = a.ty[r % a.Y], tz = a.tz[r / a.Y];
      live = ty.i0 >= 0 && tz.i0 >= 0;
      if (live) {
        for (int l = lane; l < S; l += 64) {          // map x indices of this lane
          const float* p0 = a.maps + l * S2 + (long)ty.i0 * S;
          const float* p1 = a.maps + l * S2 + (long)ty.i1 * S;
          for (int m = 0; m < a.n_maps; ++m) {
            const long mo = m * S3;
            const double v00 = (double)p0[mo + tz.i0], v01 = (double)p0[mo + tz.i1];
            const double v10 = (double)p1[mo + tz.i0], v11 = (double)p1[mo + tz.i1];
            line[m * S + l] = (1.0 - ty.w) * ((1.0 - tz.w) * v00 + tz.w * v01) + ty.w * ((1.0 - tz.w) * v10 + tz.w * v11);
          }
        }
      }
    }
    __syncthreads();
    if (r < R) {
      for (int m = 0; m < a.n_maps; ++m) {
        float* dst = a.out + (long)m * V + r * a.X;
        const double* ln = line + m * S;
#pragma unroll
        for (int c = 0; c < MS_XCH; ++c) {
          if (x0[c] >= a.X) continue;
          IgVec<float, VEC> o;
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const MsTap& q = t[c][k];
            const double v = (1.0 - q.w) * ln[max(q.i0, 0)] + q.w * ln[max(q.i1, 0)];
            o.e[k] = (live && q.i0 >= 0) ? (float)v : 0.f;
          }
          *reinterpret_cast<IgVec<float, VEC>*>(dst + x0[c]) = o;
        }
      }
    }
    __syncthreads();                                  // the lines are rewritten by the next row
  }
}

namespace {

struct IgLayout {
  size_t flags, kept, m, total;     // flags: X + Y + Z words (one memset); kept: X + Y + Z ints; m: the extents
};

IgLayout ig_layout(int x, int y, int z) {
  const size_t n = (size_t)x + (size_t)y + (size_t)z;
  IgLayout L;
  Carver cv;
  L.flags = cv.take(n * sizeof(unsigned));
  L.kept = cv.take(n * sizeof(int));
  L.m = cv.take(4 * sizeof(int));
  L.total = cv.cur;
  return L;
}

int ig_validate_extent(int x, int y, int z) {
  MMNN_REQUIRE(x >= 1 && y >= 1 && z >= 1, "ingest: non-positive extent %d x %d x %d", x, y, z);
  MMNN_REQUIRE(x <= MMNN_INGEST_MAX_X, "ingest: x extent %d above %d", x, MMNN_INGEST_MAX_X);
  MMNN_REQUIRE((long)y * z < (1l << 31) && (long)x + y + z < (1l << 30), "ingest: extent %d x %d x %d too large", x, y, z);
  return 0;
}

int ig_validate_size(int size) {
  MMNN_REQUIRE(size >= 1 && size <= MMNN_INGEST_MAX_SIZE, "ingest: size %d outside 1..%d", size, MMNN_INGEST_MAX_SIZE);
  return 0;
}

int ms_validate_extent(int x, int y, int z) {
  if (ig_validate_extent(x, y, z) != 0) return 1;
  MMNN_REQUIRE((double)x * y * z < 2147483648.0, "maps_to_scan: scan extent %d x %d x %d holds 2^31 voxels or more", x, y, z);
  return 0;
}

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_ingest_workspace_bytes(int32_t x, int32_t y, int32_t z) {
  if (ig_validate_extent(x, y, z) != 0) return -1;
  return (int64_t)ig_layout(x, y, z).total;
}

int mmnn_ingest_volume(const mmnn_ingest_desc* d, const void* scan, const void* mask, float* out_plane, int32_t* extents, void* ws,
                       void* stream_) {
  return mmnn_ingest_volume_sized(d, MMNN_INGEST_SIZE, scan, mask, out_plane, extents, ws, stream_);
}

int mmnn_ingest_volume_sized(const mmnn_ingest_desc* d, int32_t size, const void* scan, const void* mask, float* out_plane,
                             int32_t* extents, void* ws, void* stream_) {
  MMNN_REQUIRE(d, "ingest: null descriptor");
  if (ig_validate_extent(d->x, d->y, d->z) != 0 || ig_validate_size(size) != 0) return 1;
  const int ssz = ig_type_size(d->scan_type), msz = ig_type_size(d->mask_type);
  MMNN_REQUIRE(ssz != 0, "ingest: unsupported scan datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->scan_type);
  MMNN_REQUIRE(msz != 0, "ingest: unsupported mask datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->mask_type);
  MMNN_REQUIRE(scan && mask && out_plane && extents && ws, "ingest: null argument");
  MMNN_REQUIRE((uintptr_t)scan % ssz == 0 && (uintptr_t)mask % msz == 0, "ingest: scan / mask buffer not aligned to its element size");
  MMNN_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)out_plane % 4 == 0 && (uintptr_t)extents % 4 == 0, "ingest: misaligned workspace / output");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const IgLayout L = ig_layout(d->x, d->y, d->z);
  char* wsb = static_cast<char*>(ws);
  IgArgs a{};
  a.scan = scan; a.mask = mask;
  a.X = d->x; a.Y = d->y; a.Z = d->z;
  a.stype = d->scan_type; a.mtype = d->mask_type;
  a.ss = ig_scale(d->scan_slope, d->scan_inter);
  a.ms = ig_scale(d->mask_slope, d->mask_inter);
  a.flag_x = reinterpret_cast<unsigned*>(wsb + L.flags); a.flag_y = a.flag_x + d->x; a.flag_z = a.flag_y + d->y;
  a.kept_x = reinterpret_cast<int*>(wsb + L.kept); a.kept_y = a.kept_x + d->x; a.kept_z = a.kept_y + d->y;
  a.M = reinterpret_cast<int*>(wsb + L.m);
  a.extents = extents;
  a.out = out_plane;
  a.S = size;

  MMNN_HIP(hipMemsetAsync(wsb + L.flags, 0, ((size_t)d->x + d->y + d->z) * sizeof(unsigned), stream));
  // pass A: 4 voxels per lane when every row starts on a 4-voxel boundary of both buffers
  const int R = d->y * d->z;
  const bool vec4 = d->x % 4 == 0 && (uintptr_t)scan % (4 * ssz) == 0 && (uintptr_t)mask % (4 * msz) == 0;
  const int vec = vec4 ? 4 : 1;
  const int gx = cdiv(d->x, 64 * vec);
  int gy = cdiv(R, IG_WAVES);
  const int cap = cdiv(2048, gx);
  if (gy > cap) gy = cap;
  if (vec4) MMNN_LAUNCH(ingest_flags_kernel<4>, dim3(gx, gy), dim3(64, IG_WAVES), 0, stream, a);
  else MMNN_LAUNCH(ingest_flags_kernel<1>, dim3(gx, gy), dim3(64, IG_WAVES), 0, stream, a);
  MMNN_LAUNCH(ingest_scan_kernel, dim3(1), dim3(IG_SCAN_TPB), IG_SCAN_TPB * sizeof(int), stream, a);
  MMNN_LAUNCH(ingest_area_kernel, dim3(cdiv(size, IG_WAVES), size), dim3(IG_TPB), (size_t)IG_WAVES * d->x * sizeof(double), stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int mmnn_resample_mask(const mmnn_resample_mask_desc* d, const void* mask, uint8_t* out, void* stream_) {
  MMNN_REQUIRE(d, "resample_mask: null descriptor");
  MMNN_REQUIRE(d->x >= 1 && d->y >= 1 && d->z >= 1, "resample_mask: non-positive scan extent %d x %d x %d", d->x, d->y, d->z);
  MMNN_REQUIRE(d->mx >= 1 && d->my >= 1 && d->mz >= 1, "resample_mask: non-positive mask extent %d x %d x %d", d->mx, d->my, d->mz);
  MMNN_REQUIRE((double)d->x * d->y * d->z < 2147483648.0, "resample_mask: scan extent %d x %d x %d holds 2^31 voxels or more", d->x, d->y, d->z);
  MMNN_REQUIRE((double)d->mx * d->my * d->mz < 2147483648.0, "resample_mask: mask extent %d x %d x %d holds 2^31 voxels or more", d->mx, d->my, d->mz);
  const int msz = ig_type_size(d->mask_type);
  MMNN_REQUIRE(msz != 0, "resample_mask: unsupported mask datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->mask_type);
  for (int i = 0; i < 12; ++i) MMNN_REQUIRE(std::isfinite(d->index_map[i]), "resample_mask: index_map[%d] is not finite", i);
  MMNN_REQUIRE(std::isfinite(d->threshold), "resample_mask: the threshold is not finite");
  MMNN_REQUIRE(mask && out, "resample_mask: null argument");
  MMNN_REQUIRE((uintptr_t)mask % msz == 0, "resample_mask: mask buffer not aligned to its element size");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  RsArgs a{};
  a.mask = mask; a.out = out;
  a.X = d->x; a.Y = d->y; a.Z = d->z;
  a.MX = d->mx; a.MY = d->my; a.MZ = d->mz;
  a.ms = ig_scale(d->mask_slope, d->mask_inter);
  for (int i = 0; i < 12; ++i) a.T[i] = d->index_map[i];
  a.thr = d->threshold;
  // 4 voxels per lane and one dword store when every output row starts on a 4-byte boundary
  const bool vec4 = d->x % 4 == 0 && (uintptr_t)out % 4 == 0;
  const int gx = cdiv(d->x, 64 * (vec4 ? 4 : 1));
  int gy = cdiv((long)d->y * d->z, IG_WAVES);
  const int cap = cdiv(2048, gx);
  if (gy > cap) gy = cap;
  if (vec4) MMNN_LAUNCH(resample_mask_kernel<4>, dim3(gx, gy), dim3(64, IG_WAVES), 0, stream, a, d->mask_type);
  else MMNN_LAUNCH(resample_mask_kernel<1>, dim3(gx, gy), dim3(64, IG_WAVES), 0, stream, a, d->mask_type);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int64_t mmnn_maps_to_scan_workspace_bytes(int32_t x, int32_t y, int32_t z) {
  if (ms_validate_extent(x, y, z) != 0) return -1;
  Carver cv;
  cv.take(((size_t)x + (size_t)y + (size_t)z) * sizeof(MsTap));
  return (int64_t)cv.cur;
}

int mmnn_maps_to_scan(const mmnn_maps_to_scan_desc* d, const void* ingest_ws, const float* maps, float* out, void* ws, void* stream_) {
  return mmnn_maps_to_scan_sized(d, MMNN_INGEST_SIZE, ingest_ws, maps, out, ws, stream_);
}

int mmnn_maps_to_scan_sized(const mmnn_maps_to_scan_desc* d, int32_t size, const void* ingest_ws, const float* maps, float* out, void* ws,
                            void* stream_) {
  MMNN_REQUIRE(d, "maps_to_scan: null descriptor");
  if (ms_validate_extent(d->x, d->y, d->z) != 0) return 1;
  MMNN_REQUIRE(size >= 1 && size <= MMNN_INGEST_MAX_SIZE, "maps_to_scan: size %d outside 1..%d", size, MMNN_INGEST_MAX_SIZE);
  MMNN_REQUIRE(d->n_maps >= 1 && d->n_maps <= MMNN_MAPS_TO_SCAN_MAX_MAPS, "maps_to_scan: n_maps %d outside 1..%d", d->n_maps, MMNN_MAPS_TO_SCAN_MAX_MAPS);
  MMNN_REQUIRE(ingest_ws && maps && out && ws, "maps_to_scan: null argument");
  MMNN_REQUIRE((uintptr_t)ingest_ws % 256 == 0 && (uintptr_t)ws % 256 == 0 && (uintptr_t)maps % 4 == 0 && (uintptr_t)out % 4 == 0,
               "maps_to_scan: misaligned workspace / maps / output");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const IgLayout L = ig_layout(d->x, d->y, d->z);
  const char* iws = static_cast<const char*>(ingest_ws);
  MsArgs a{};
  a.kept_x = reinterpret_cast<const int*>(iws + L.kept); a.kept_y = a.kept_x + d->x; a.kept_z = a.kept_y + d->y;
  a.M = reinterpret_cast<const int*>(iws + L.m);
  a.tx = static_cast<MsTap*>(ws); a.ty = a.tx + d->x; a.tz = a.ty + d->y;
  a.maps = maps; a.out = out;
  a.X = d->x; a.Y = d->y; a.Z = d->z; a.n_maps = d->n_maps;
  a.S = size;
  MMNN_LAUNCH(maps_taps_kernel, dim3(cdiv((long)d->x + d->y + d->z, IG_SCAN_TPB)), dim3(IG_SCAN_TPB), 0, stream, a);
  // 4 voxels per lane and 16-byte stores when every output row starts on a 16-byte boundary
  const bool vec4 = d->x % 4 == 0 && (uintptr_t)out % 16 == 0;
  const int gx = cdiv(d->x, MS_XCH * 64 * (vec4 ? 4 : 1));
  int gy = cdiv((long)d->y * d->z, IG_WAVES);
  const int cap = cdiv(2048, gx);
  if (gy > cap) gy = cap;
  const size_t lds = (size_t)IG_WAVES * d->n_maps * size * sizeof(double);      // at most 64 KiB: 16 maps of 128^3
  if (vec4) MMNN_LAUNCH(maps_to_scan_kernel<4>, dim3(gx, gy), dim3(64, IG_WAVES), lds, stream, a);
  else MMNN_LAUNCH(maps_to_scan_kernel<1>, dim3(gx, gy), dim3(64, IG_WAVES), lds, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
