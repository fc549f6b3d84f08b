// The surface mesh of one ROI and what the mesh-based shape features need from it, from what `mmnn_radiomics` (csrc/radiomics.hip) left on
// the device: the uint16 bin volume (0 outside the ROI) in its workspace, the flags in the state block there and the bounding box in its
// result block.  The contract is the comment above mmnn_radiomics_mesh in include/mmnn_sts.h.  Everything is enqueued on the caller's
// stream behind the extraction; nothing is read back and the host never waits.  No triangle is ever materialised.
//
//   memsets            cfg[256]; the accumulators in ws4 (vertex cursor, the origin term of the volume, the four maxima)
//   mesh_cell_kernel   one cell (origin -1 .. extent - 1 per axis) per lane and trip: eight bounds-checked 2-byte corner reads -> the
//                      configuration byte; one count in the workgroup's LDS histogram (rad_count: a wave that agrees sends one add); the
//                      origin term (o - lo) . N[cfg] as an int64 per lane; the vertices of the cell's three forward edges (from corner 0
//                      along x, y, z: every lattice edge belongs to exactly one cell this way) appended to the list in ws4, one atomic
//                      add of the wave's total on the cursor per trip.  The histogram is flushed with one 64-bit add per used entry
//   mesh_pair_kernel   tile pairs (ti >= tj) of 256 vertices, a fixed grid that strides over the pairs counted from the DEVICE's vertex
//                      count: a workgroup stages the j tile in LDS (the transformed doubles t_r and the integer coordinates), each lane
//                      keeps one i vertex in registers and runs over the 256 staged ones; four running maxima per lane, block_reduce
//                      (Greater), then an integer atomic maximum on the bit pattern of the non-negative doubles
//   mesh_final_kernel  one workgroup, lane c = configuration c: A_c from the table and cof(L); n_triangles and the local volume term as
//                      exact integer sums; lane 0 adds cfg[c] A_c in index order and writes the result block (the NaN block with a flag)
//
// Exactness.  cfg, n_vertices, n_triangles and volume48 are integer sums (uint32 in LDS, uint64 adds in global memory); the origin term
// is accumulated modulo 2^64 and the final value (at most 48 x the ROI's voxel count) is far inside the range, so it is exact whatever
// the partial sums did.  The four squared diameters are maxima: order-free, bit-identical from call to call although the order of the
// vertex list is not.  The area is one sequential fp64 sum over 256 terms.  No floating-point atomics; no scalar memory writes.
#include "ingest_load.hpp"
#include "mesh_cell.hpp"
#include "radiomics.hpp"

#include <cmath>

namespace mmnn {

constexpr int MS_TILE = 256;                // vertices per tile = lanes per workgroup
constexpr int MS_CELL_CHUNKS = 2048;        // workgroups of the cell pass (at most): below 2^32 cells per workgroup's LDS histogram
constexpr int MS_PAIR_GRID = 2048;          // workgroups of the pair pass (at most): 8 per CU of 256
constexpr int MS_ACC = 8;
static_assert(MS_TILE == RAD_TPB, "one staged vertex and one configuration per lane");
enum { MA_NV = 0, MA_ORIGIN = 1, MA_Q = 2 };  // acc: vertex cursor, sum (o - lo) . N, then the bit patterns of the four maxima

struct MeshArgs : RadFollow {
  const mmnn_radiomics_result* res;         // the first call's block: lo[3]
  unsigned long long cells;                 // (X + 1)(Y + 1)(Z + 1)
  unsigned long long* cfg;                  // [256], caller-owned
  unsigned long long* acc;                  // [MS_ACC]
  uint32_t* vx; uint32_t* vy; uint32_t* vz; // [3 cells] each: doubled coordinate + 1 (0 .. 2 extent)
  double L[9];
  mmnn_radiomics_mesh_result* out;
};

// ---- cells -------------------------------------------------------------------------------------------------------------------------------
// Every lane of a workgroup makes the same number of trips, so the ballots (here and inside rad_count) see whole waves.
__global__ void __launch_bounds__(RAD_TPB) mesh_cell_kernel(const MeshArgs a) {
  __shared__ unsigned hist[256];
  __shared__ int nsum[256];                 // N[cfg], three signed bytes packed
  if (a.st->flagged) return;
  const int t = threadIdx.x, lane = t & 63;
  hist[t] = 0u;
  nsum[t] = (int)(((unsigned)(uint8_t)mesh_nsum_dev[t][0]) | ((unsigned)(uint8_t)mesh_nsum_dev[t][1] << 8) | ((unsigned)(uint8_t)mesh_nsum_dev[t][2] << 16));
  __syncthreads();
  const unsigned ng = (unsigned)a.st->n_bins;
  const long long lox = a.res->lo[0], loy = a.res->lo[1], loz = a.res->lo[2];
  const unsigned long long X1 = (unsigned)a.X + 1u, Y1 = (unsigned)a.Y + 1u;
  const bool narrow = (a.cells >> 32) == 0ull;
  const unsigned long long stride = (unsigned long long)gridDim.x * RAD_TPB;
  const unsigned long long trips = (a.cells + stride - 1ull) / stride;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long idx = (unsigned long long)blockIdx.x * RAD_TPB + t;
  long long origin = 0;
  for (unsigned long long trip = 0; trip < trips; ++trip, idx += stride) {
    const bool valid = idx < a.cells;
    unsigned c = 0u;
    int ox = 0, oy = 0, oz = 0;
    if (valid) {
      unsigned long long cx, cy, cz;
      if (narrow) {                                                     // (uniform) 32-bit divisions where the cell count allows them
        const unsigned i32 = (unsigned)idx, r = i32 / (unsigned)X1;
        cx = i32 - r * (unsigned)X1; cz = r / (unsigned)Y1; cy = r - (unsigned)cz * (unsigned)Y1;
      } else {
        const unsigned long long r = idx / X1;
        cx = idx - r * X1; cz = r / Y1; cy = r - cz * Y1;
      }
      ox = (int)cx - 1; oy = (int)cy - 1; oz = (int)cz - 1;
      c = mesh_cell_config(a.bins, a.X, a.Y, a.Z, ng, ox, oy, oz);
    }
    rad_count(hist, c, valid);
    if (c != 0u && c != 255u) {
      const int p = nsum[c];
      origin += (ox - lox) * (long long)(int8_t)p + (oy - loy) * (long long)(int8_t)(p >> 8) + (oz - loz) * (long long)(int8_t)(p >> 16);
    }
    // the three forward edges of corner 0: towards corner 1 (x), 2 (y) and 4 (z)
    const bool e0 = ((c ^ (c >> 1)) & 1u) != 0u, e1 = ((c ^ (c >> 2)) & 1u) != 0u, e2 = ((c ^ (c >> 4)) & 1u) != 0u;
    const unsigned long long m0 = __ballot(e0), m1 = __ballot(e1), m2 = __ballot(e2);
    const unsigned n0 = (unsigned)__popcll(m0), n1 = (unsigned)__popcll(m1), n2 = (unsigned)__popcll(m2);
    if (n0 + n1 + n2 == 0u) continue;                                   // (uniform over the wave)
    unsigned long long base = 0ull;
    if (lane == 0) base = atomicAdd(&a.acc[MA_NV], (unsigned long long)(n0 + n1 + n2));
    base = __shfl(base, 0, 64);                                         // at most 3 cells vertices in all: every slot lies in the list
    const unsigned ux = 2u * (unsigned)ox + 1u, uy = 2u * (unsigned)oy + 1u, uz = 2u * (unsigned)oz + 1u;     // the corner, + 1, modulo 2^32
    if (e0) { const unsigned long long s = base + (unsigned)__popcll(m0 & below); a.vx[s] = ux + 1u; a.vy[s] = uy; a.vz[s] = uz; }
    if (e1) { const unsigned long long s = base + n0 + (unsigned)__popcll(m1 & below); a.vx[s] = ux; a.vy[s] = uy + 1u; a.vz[s] = uz; }
    if (e2) { const unsigned long long s = base + n0 + n1 + (unsigned)__popcll(m2 & below); a.vx[s] = ux; a.vy[s] = uy; a.vz[s] = uz + 1u; }
  }
  origin = wave_sum(origin);
  if (lane == 0 && origin != 0) atomicAdd(&a.acc[MA_ORIGIN], (unsigned long long)origin);
  __syncthreads();
  if (hist[t] != 0u) atomicAdd(&a.cfg[t], (unsigned long long)hist[t]);
}

// ---- vertex pairs ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double mesh_map(const double* L, int r, double x, double y, double z) {
  return (L[3 * r] * x + L[3 * r + 1] * y) + L[3 * r + 2] * z;
}

__global__ void __launch_bounds__(RAD_TPB) mesh_pair_kernel(const MeshArgs a) {
  __shared__ double jt[3][MS_TILE];
  __shared__ unsigned jc[3][MS_TILE];
  __shared__ double red[(RAD_TPB / 64) * 4];
  if (a.st->flagged) return;
  const unsigned long long V = a.acc[MA_NV];
  const unsigned long long T = (V + MS_TILE - 1ull) / MS_TILE, P = T * (T + 1ull) / 2ull;      // V <= 3 * 2^34: P < 2^63
  const int t = threadIdx.x;
  double m[4] = {0.0, 0.0, 0.0, 0.0};
  for (unsigned long long p = blockIdx.x; p < P; p += gridDim.x) {     // (uniform over the workgroup) p = ti (ti + 1) / 2 + tj, tj <= ti
    unsigned long long ti = (unsigned long long)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while ((ti + 1ull) * (ti + 2ull) / 2ull <= p) ++ti;
    while (ti * (ti + 1ull) / 2ull > p) --ti;
    const unsigned long long tj = p - ti * (ti + 1ull) / 2ull;
    // a lane past the end of the list takes its tile's first vertex again: a pair that is counted anyway
    unsigned long long gi = ti * MS_TILE + t, gj = tj * MS_TILE + t;
    if (gi >= V) gi = ti * MS_TILE;
    if (gj >= V) gj = tj * MS_TILE;
    const unsigned ix = a.vx[gi], iy = a.vy[gi], iz = a.vz[gi];
    const double fx = (double)ix - 1.0, fy = (double)iy - 1.0, fz = (double)iz - 1.0;
    const double t0 = mesh_map(a.L, 0, fx, fy, fz), t1 = mesh_map(a.L, 1, fx, fy, fz), t2 = mesh_map(a.L, 2, fx, fy, fz);
    {
      const unsigned jx = a.vx[gj], jy = a.vy[gj], jz = a.vz[gj];
      const double gx = (double)jx - 1.0, gy = (double)jy - 1.0, gz = (double)jz - 1.0;
      __syncthreads();                                                  // the previous pair's reads of the tile are done
      jc[0][t] = jx; jc[1][t] = jy; jc[2][t] = jz;
      jt[0][t] = mesh_map(a.L, 0, gx, gy, gz); jt[1][t] = mesh_map(a.L, 1, gx, gy, gz); jt[2][t] = mesh_map(a.L, 2, gx, gy, gz);
      __syncthreads();
    }
#pragma unroll 4
    for (int j = 0; j < MS_TILE; ++j) {
      const double d0 = t0 - jt[0][j], d1 = t1 - jt[1][j], d2 = t2 - jt[2][j];
      const double q = (d0 * d0 + d1 * d1) + d2 * d2;
      const double qz = iz == jc[2][j] ? q : 0.0, qy = iy == jc[1][j] ? q : 0.0, qx = ix == jc[0][j] ? q : 0.0;
      m[0] = fmax(m[0], q);                                             // one v_max_f64 each; q >= +0 and never NaN while t is finite
      m[1] = fmax(m[1], qz);
      m[2] = fmax(m[2], qy);
      m[3] = fmax(m[3], qx);
    }
  }
  block_reduce<RAD_TPB / 64>(m, red, Greater{});
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)                                          // non-negative doubles order like their bit patterns
      if (m[k] > 0.0) atomicMax(&a.acc[MA_Q + k], (unsigned long long)__double_as_longlong(m[k]));
  }
}

// ---- the result ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RAD_TPB) mesh_final_kernel(const MeshArgs a) {
  __shared__ double area[256];
  __shared__ unsigned long long ired[RAD_TPB / 64];
  const int t = threadIdx.x;
  if (a.st->flagged) {                                                  // cfg was zeroed by the memset
    if (t == 0) {
      a.out->n_vertices = 0; a.out->n_triangles = 0; a.out->volume48 = 0;
      a.out->area = rad_nan();
      for (int k = 0; k < 4; ++k) a.out->q[k] = rad_nan();
    }
    return;
  }
  double C[9];
  mesh_cofactor(a.L, C);
  const unsigned long long count = a.cfg[t];
  area[t] = (double)count * mesh_cell_area(mesh_tri_dev[t], C);
  unsigned long long ntri = count * (unsigned long long)mesh_tri_dev[t][MMNN_MESH_TRI_ROW - 1];
  unsigned long long local = count * (unsigned long long)(long long)mesh_l48_dev[t];          // modulo 2^64
  ntri = block_reduce<RAD_TPB / 64>(ntri, ired, Sum{});
  local = block_reduce<RAD_TPB / 64>(local, ired, Sum{});
  __syncthreads();
  if (t != 0) return;
  double s = 0.0;
  for (int c = 0; c < 256; ++c) s = s + area[c];                        // index order
  a.out->n_vertices = (long long)a.acc[MA_NV];
  a.out->n_triangles = (long long)ntri;
  a.out->volume48 = (long long)(local + 2ull * a.acc[MA_ORIGIN]);
  a.out->area = s;
  for (int k = 0; k < 4; ++k) a.out->q[k] = __longlong_as_double((long long)a.acc[MA_Q + k]);
}

namespace {

struct MeshLayout { size_t acc, vx, vy, vz, total; unsigned long long cells; };

MeshLayout mesh_layout(int x, int y, int z) {
  MeshLayout M;
  Carver cv;
  M.cells = ((unsigned long long)x + 1ull) * ((unsigned long long)y + 1ull) * ((unsigned long long)z + 1ull);       // x y z < 2^31: below 2^34
  const size_t cap = (size_t)(3ull * M.cells);                         // every cell owns three lattice edges
  M.acc = cv.take((size_t)MS_ACC * 8);
  M.vx = cv.take(cap * 4);
  M.vy = cv.take(cap * 4);
  M.vz = cv.take(cap * 4);
  M.total = cv.cur;
  return M;
}

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_radiomics_mesh_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins) {
  if (rad_validate(x, y, z, max_bins) != 0) return -1;
  return (int64_t)mesh_layout(x, y, z).total;
}

// host only: the table the library was built with
int mmnn_radiomics_mesh_table(int8_t* tri, int32_t* l48, int32_t* nsum) {
  MMNN_REQUIRE(tri && l48 && nsum, "radiomics_mesh_table: null argument");
  for (int c = 0; c < 256; ++c) {
    for (int k = 0; k < MMNN_MESH_TRI_ROW; ++k) tri[c * MMNN_MESH_TRI_ROW + k] = mesh_tri_host[c][k];
    l48[c] = mesh_l48_host[c];
    for (int k = 0; k < 3; ++k) nsum[3 * c + k] = mesh_nsum_host[c][k];
  }
  return 0;
}

int mmnn_radiomics_mesh(const mmnn_radiomics_desc* d, const mmnn_radiomics_result* result, const void* ws, const double* linear,
                        mmnn_radiomics_mesh_result* out, uint64_t* cfg, void* ws4, void* stream_) {
  if (rad_validate_follow("radiomics_mesh", d) != 0) return 1;
  MMNN_REQUIRE(result && ws && linear && out && cfg && ws4, "radiomics_mesh: null argument");
  for (int k = 0; k < 9; ++k) MMNN_REQUIRE(std::isfinite(linear[k]), "radiomics_mesh: linear[%d] is not finite", k);
  MMNN_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)ws4 % 256 == 0 && (uintptr_t)result % 8 == 0 && (uintptr_t)out % 8 == 0 &&
                   (uintptr_t)cfg % 8 == 0,
               "radiomics_mesh: misaligned workspace / result / table");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MeshLayout M = mesh_layout(d->x, d->y, d->z);
  char* w4 = static_cast<char*>(ws4);
  MeshArgs a{};
  static_cast<RadFollow&>(a) = rad_follow(d, ws);
  a.res = result;
  a.cells = M.cells;
  a.cfg = reinterpret_cast<unsigned long long*>(cfg);
  a.acc = reinterpret_cast<unsigned long long*>(w4 + M.acc);
  a.vx = reinterpret_cast<uint32_t*>(w4 + M.vx);
  a.vy = reinterpret_cast<uint32_t*>(w4 + M.vy);
  a.vz = reinterpret_cast<uint32_t*>(w4 + M.vz);
  for (int k = 0; k < 9; ++k) a.L[k] = linear[k];
  a.out = out;
  const unsigned long long cell_groups = (M.cells + RAD_TPB - 1ull) / RAD_TPB;
  const int chunks = cell_groups > (unsigned long long)MS_CELL_CHUNKS ? MS_CELL_CHUNKS : (int)cell_groups;
  // the host-side bound of the tile pairs; the device strides over the pairs its own vertex count gives, surplus workgroups leave
  const unsigned long long tiles = (3ull * M.cells + MS_TILE - 1ull) / MS_TILE;
  const unsigned long long pairs = tiles >= (1ull << 31) ? ~0ull : tiles * (tiles + 1ull) / 2ull;
  const int pair_grid = pairs > (unsigned long long)MS_PAIR_GRID ? MS_PAIR_GRID : (int)pairs;

  MMNN_HIP(hipMemsetAsync(cfg, 0, 256 * 8, stream));
  MMNN_HIP(hipMemsetAsync(w4 + M.acc, 0, (size_t)MS_ACC * 8, stream));
  MMNN_LAUNCH(mesh_cell_kernel, dim3(chunks), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(mesh_pair_kernel, dim3(pair_grid), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(mesh_final_kernel, dim3(1), dim3(RAD_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
