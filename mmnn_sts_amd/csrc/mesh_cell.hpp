// The per-cell arithmetic of the surface mesh (csrc/radiomics_mesh.hip), written once for the device and the host: the configuration
// byte of a cell, the midpoint of a cell edge, a triangle's integer normal and the area of a configuration's triangles under a linear
// map.  The host compiles the same functions (a plain C++ compiler sees no HIP keyword here), which is how the table and the vertex
// enumeration were run under the address and undefined-behaviour sanitizers without a device.
//
// Conventions (the contract above mmnn_radiomics_mesh in include/mmnn_sts.h): corner k of the cell with origin o is
// o + (k & 1, k >> 1 & 1, k >> 2 & 1) in (x, y, z); a corner outside the volume is empty; edge 4 a + p + 2 q runs along axis a at the
// position (p, q) of the two other axes in ascending order; coordinates are doubled, so an edge's midpoint is an integer triple.
#pragma once
#include "mesh_table.hpp"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MMNN_HD __host__ __device__ __forceinline__
#else
#define MMNN_HD inline
#endif

namespace mmnn {

static const int8_t mesh_tri_host[256][MMNN_MESH_TRI_ROW] = MMNN_MESH_TRI_INIT;
static const int32_t mesh_l48_host[256] = MMNN_MESH_L48_INIT;
static const int8_t mesh_nsum_host[256][3] = MMNN_MESH_NSUM_INIT;
#if defined(__HIPCC__)
static __device__ const int8_t mesh_tri_dev[256][MMNN_MESH_TRI_ROW] = MMNN_MESH_TRI_INIT;
static __device__ const int32_t mesh_l48_dev[256] = MMNN_MESH_L48_INIT;
static __device__ const int8_t mesh_nsum_dev[256][3] = MMNN_MESH_NSUM_INIT;
#endif

// bins: [Z][Y][X] uint16, 0 outside the ROI; a value above ng is stale and counts as outside, as in the other radiomics passes.
// Every read is bounds-checked on (x, y, z): the padding layer is never stored and a row or slice end never wraps.
MMNN_HD unsigned mesh_cell_config(const uint16_t* bins, int X, int Y, int Z, unsigned ng, int ox, int oy, int oz) {
  unsigned c = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int px = ox + (k & 1), py = oy + ((k >> 1) & 1), pz = oz + (k >> 2);
    if (px < 0 || px >= X || py < 0 || py >= Y || pz < 0 || pz >= Z) continue;
    const unsigned b = bins[((unsigned)pz * (unsigned)Y + (unsigned)py) * (unsigned)X + (unsigned)px];       // x * y * z < 2^31
    c |= (unsigned)(b != 0u && b <= ng) << k;
  }
  return c;
}

// midpoint of edge e, doubled, relative to the cell origin
MMNN_HD void mesh_edge_point(int e, int p[3]) {
  const int a = e >> 2, r = e & 3;
  const int u = a == 0 ? 1 : 0, w = a == 2 ? 1 : 2;
  p[a] = 1;
  p[u] = 2 * (r & 1);
  p[w] = 2 * (r >> 1);
}

// (b - a) x (c - a) of triangle t of a table row
MMNN_HD void mesh_tri_normal(const int8_t* row, int t, int n[3]) {
  int a[3], b[3], c[3];
  mesh_edge_point(row[3 * t], a);
  mesh_edge_point(row[3 * t + 1], b);
  mesh_edge_point(row[3 * t + 2], c);
  const int ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
  n[0] = uy * vz - uz * vy;
  n[1] = uz * vx - ux * vz;
  n[2] = ux * vy - uy * vx;
}

// cof(L): row r is the cross product of the two other rows of L, so that (L a) x (L b) = cof(L) (a x b)
MMNN_HD void mesh_cofactor(const double* L, double C[9]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
      C[3 * r + c] = L[3 * r1 + c1] * L[3 * r2 + c2] - L[3 * r1 + c2] * L[3 * r2 + c1];
    }
}

// A_c: sum over the row's triangles, in table order, of |cof(L) n| / 8 (half the parallelogram, a quarter for the doubled coordinates)
MMNN_HD double mesh_cell_area(const int8_t* row, const double C[9]) {
  double s = 0.0;
  const int nt = row[MMNN_MESH_TRI_ROW - 1];
  for (int t = 0; t < nt; ++t) {
    int n[3];
    mesh_tri_normal(row, t, n);
    double w[3];
    for (int r = 0; r < 3; ++r) w[r] = (C[3 * r] * (double)n[0] + C[3 * r + 1] * (double)n[1]) + C[3 * r + 2] * (double)n[2];
    s = s + sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) * 0.125;
  }
  return s;
}

}  // namespace mmnn
