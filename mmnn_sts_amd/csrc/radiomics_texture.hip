// The run-length (GLRLM), dependence (GLDM) and neighbouring grey-tone difference (NGTDM) texture classes of one (scan, mask) pair, from
// what `mmnn_radiomics` (csrc/radiomics.hip) left on the device: the uint16 bin volume (0 outside the ROI) in its workspace and Ng, n and
// the flags in the state block there.  The contract is the comment above mmnn_radiomics_texture in include/mmnn_sts.h.  Everything is
// enqueued on the caller's stream behind the extraction; nothing is read back and the host never waits.
//
//   memsets                glrlm, gldm, ngtdm_n, ngtdm_s
//   glrlm_count_kernel     grid (chunks, 13): a lane whose voxel starts a run along the direction walks it and issues one add.  The
//                          direction's matrix (row stride L) is privatised in LDS when Ng * L <= RADT_RUN_WORDS (16384 words = the 64 KiB
//                          of the GLCM kernel), zeroed by the workgroup and flushed once; uint32 atomics on global memory otherwise
//   nbhd_count_kernel      one sweep, 26 two-byte neighbour loads per ROI voxel, for GLDM and both NGTDM tables: Ng * 27 * (8 + 4 + 4) B of
//                          LDS when Ng <= RADT_NBHD_NG (128: 54 KiB), integer LDS atomics and one flush; global integer atomics otherwise
//   tex_features_kernel    15 workgroups: one per GLRLM direction, one for GLDM, one for NGTDM.  Marginals as exact uint64, then the fp64
//                          sums in a fixed order
//   tex_final_kernel       the average over the 13 directions; with a flag set, the NaN block
//
// The 26 neighbour loads go to the cache: a voxel's 27-neighbourhood is shared with the lanes beside it and the rows above and below, so
// the sweep reads the 2-byte volume from HBM about once.  An LDS tile with a halo would save L1 / L2 hits, not memory traffic, at the
// price of a tiling that depends on the extents; it is not built.
//
// Determinism.  The four tables are integers, accumulated exactly.  Every fp64 sum runs over a partition fixed by Ng and the extents: a
// lane adds the rows in ascending order and its columns t, t + 256, ...; a wave folds its lanes by the xor butterfly and the four waves are
// added in index order (block_reduce, reduce.hpp).  No floating-point atomics.  All index arithmetic is 32-bit (x * y * z < 2^31).
#include "ingest_load.hpp"
#include "radiomics.hpp"

#include <cmath>

namespace mmnn {

constexpr int RADT_RUN_WORDS = 16384;       // the run-length matrix in LDS: Ng * L words <= 64 KiB
constexpr int RADT_NBHD_NG = 128;           // the three neighbourhood tables in LDS: 128 * 27 * 16 B = 54 KiB
constexpr int RADT_COLS = MMNN_RADIOMICS_NEIGHBOURS;      // 27: 0..26 neighbours
constexpr int RADT_RUN_CHUNKS = 96;         // workgroups per direction (at most)
constexpr int RADT_NBHD_CHUNKS = 1024;      // workgroups of the neighbourhood sweep (at most)
constexpr int RADT_LDS_L = 4096;            // run-length marginal in LDS up to this L, in the second workspace beyond
constexpr int RADT_NRL = MMNN_RADIOMICS_GLRLM, RADT_NDM = MMNN_RADIOMICS_GLDM, RADT_NGT = MMNN_RADIOMICS_NGTDM;

struct TexArgs : RadFollow {
  int L;
  int max_bins;
  unsigned* glrlm; unsigned* gldm; unsigned* ngn;
  unsigned long long* ngs;
  double* dirf;                             // [13][16]
  unsigned long long* runs;                 // [13][L]: the run-length marginal of a direction when L > RADT_LDS_L
  mmnn_radiomics_texture_result* out;
};

// ---- run counting --------------------------------------------------------------------------------------------------------------------
// grid (chunks, 13); dynamic LDS RADT_RUN_WORDS words.  Workgroup (c, d) walks the voxels c * TPB + t, + chunks * TPB, ... for direction d.
__global__ void __launch_bounds__(RAD_TPB) glrlm_count_kernel(const TexArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned tex_lds[];
  if (a.st->flagged) return;
  const int ng = a.st->n_bins, L = a.L;
  const bool in_lds = (long)ng * L <= RADT_RUN_WORDS;
  const int d = blockIdx.y;
  const int dz = rad_dirs[d][0], dy = rad_dirs[d][1], dx = rad_dirs[d][2];
  unsigned* G = a.glrlm + (size_t)d * a.max_bins * L;
  const int cells = in_lds ? ng * L : 0;
  for (int e = threadIdx.x; e < cells; e += RAD_TPB) tex_lds[e] = 0u;
  if (in_lds) __syncthreads();
  const unsigned X = a.X, XY = (unsigned)a.X * a.Y;
  const unsigned off = (unsigned)((dz * a.Y + dy) * a.X + dx);        // added modulo 2^32: a neighbour inside the volume is below N
  const unsigned stride = gridDim.x * RAD_TPB;
  for (unsigned idx = blockIdx.x * RAD_TPB + threadIdx.x; idx < a.N; idx += stride) {
    const unsigned b = a.bins[idx];
    if (b == 0u || b > (unsigned)ng) continue;
    int x, y, z;
    rad_split(idx, X, XY, x, y, z);
    const int px = x - dx, py = y - dy, pz = z - dz;                    // (dz >= 0: pz < Z)
    if (px >= 0 && px < a.X && py >= 0 && py < a.Y && pz >= 0 && a.bins[idx - off] == b) continue;      // inside a run, not its start
    int len = 1, nx = x + dx, ny = y + dy, nz = z + dz;
    unsigned q = idx + off;
    while (nx >= 0 && nx < a.X && ny >= 0 && ny < a.Y && nz < a.Z && a.bins[q] == b) {      // at most min(extent) - 1 steps
      ++len; nx += dx; ny += dy; nz += dz; q += off;
    }
    const unsigned cell = (b - 1u) * (unsigned)L + (unsigned)(len - 1);
    if (in_lds) atomicAdd(&tex_lds[cell], 1u);
    else atomicAdd(&G[(size_t)(b - 1u) * L + (len - 1)], 1u);
  }
  if (in_lds) {
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += RAD_TPB) {
      const unsigned c = tex_lds[e];
      if (c) atomicAdd(&G[e], c);                                      // (the global rows have the stride L too)
    }
  }
}

// ---- the neighbourhood sweep -----------------------------------------------------------------------------------------------------------
// grid (chunks); dynamic LDS RADT_NBHD_NG * 27 * 16 B: s (uint64), then n and the dependence counts (uint32), each [Ng][27].
__global__ void __launch_bounds__(RAD_TPB) nbhd_count_kernel(const TexArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned tex_lds[];
  if (a.st->flagged) return;
  const int ng = a.st->n_bins;
  const bool in_lds = ng <= RADT_NBHD_NG;
  const int cells = in_lds ? ng * RADT_COLS : 0;
  unsigned long long* ls = reinterpret_cast<unsigned long long*>(tex_lds);
  unsigned* ln = tex_lds + 2 * cells;
  unsigned* ld = ln + cells;
  for (int e = threadIdx.x; e < 4 * cells; e += RAD_TPB) tex_lds[e] = 0u;
  if (in_lds) __syncthreads();
  const unsigned X = a.X, XY = (unsigned)a.X * a.Y;
  const unsigned stride = gridDim.x * RAD_TPB;
  for (unsigned idx = blockIdx.x * RAD_TPB + threadIdx.x; idx < a.N; idx += stride) {
    const unsigned b = a.bins[idx];
    if (b == 0u || b > (unsigned)ng) continue;
    int x, y, z;
    rad_split(idx, X, XY, x, y, z);
    unsigned c = 0, same = 0, B = 0;
#pragma unroll
    for (int ez = -1; ez <= 1; ++ez) {
      const int zz = z + ez;
      if (zz < 0 || zz >= a.Z) continue;
#pragma unroll
      for (int ey = -1; ey <= 1; ++ey) {
        const int yy = y + ey;
        if (yy < 0 || yy >= a.Y) continue;
        const unsigned row = ((unsigned)zz * a.Y + (unsigned)yy) * X;
#pragma unroll
        for (int ex = -1; ex <= 1; ++ex) {
          const int xx = x + ex;
          if ((ez == 0 && ey == 0 && ex == 0) || xx < 0 || xx >= a.X) continue;
          const unsigned v = a.bins[row + (unsigned)xx];
          if (v == 0u) continue;
          ++c; B += v; same += v == b ? 1u : 0u;
        }
      }
    }
    const unsigned ic = b * c;
    const unsigned long long diff = ic > B ? ic - B : B - ic;           // |i * c - B| < 2^15
    const unsigned i27 = (b - 1u) * RADT_COLS;
    if (in_lds) {
      atomicAdd(&ld[i27 + same], 1u);
      atomicAdd(&ln[i27 + c], 1u);
      if (diff) atomicAdd(&ls[i27 + c], diff);
    } else {
      atomicAdd(&a.gldm[i27 + same], 1u);
      atomicAdd(&a.ngn[i27 + c], 1u);
      if (diff) atomicAdd(&a.ngs[i27 + c], diff);
    }
  }
  if (in_lds) {
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += RAD_TPB) {
      const unsigned cd = ld[e], cn = ln[e];
      const unsigned long long cs = ls[e];
      if (cd) atomicAdd(&a.gldm[e], cd);
      if (cn) atomicAdd(&a.ngn[e], cn);
      if (cs) atomicAdd(&a.ngs[e], cs);
    }
  }
}

// ---- features ----------------------------------------------------------------------------------------------------------------------------
// The 16 run-length features of one matrix P[i * stride + j], i < ng (level i + 1), j < J (length or dependence j + 1), in the order of
// MMNN_RADIOMICS_GLRLM; the dependence class takes 14 of them.  pg: ng words of LDS, pr: J words (LDS or global, owned by the calling
// workgroup).  Thread t owns the columns t, t + TPB, ...: pr needs no atomics.  The same f in every thread; all NaN for an empty matrix.
__device__ void tex_matrix_features(const unsigned* P, size_t stride, int ng, int J, double Np, unsigned long long* pg,
                                    unsigned long long* pr, unsigned long long* total, double* red, double (&f)[16]) {
  const int t = threadIdx.x;
  for (int i = t; i < ng; i += RAD_TPB) pg[i] = 0;
  for (int j = t; j < J; j += RAD_TPB) pr[j] = 0;
  if (t == 0) *total = 0;
  __syncthreads();
  unsigned long long own = 0;
  for (int i = 0; i < ng; ++i) {
    unsigned long long rsum = 0;
    for (int j = t; j < J; j += RAD_TPB) {
      const unsigned c = P[(size_t)i * stride + j];
      if (c == 0u) continue;
      rsum += c;
      pr[j] += c;
    }
    if (rsum) { atomicAdd(&pg[i], rsum); own += rsum; }
  }
  if (own) atomicAdd(total, own);
  __syncthreads();
  if (*total == 0ull) {
    for (int k = 0; k < 16; ++k) f[k] = rad_nan();
    return;
  }
  const double Nr = (double)*total;
  double a4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = t; j < J; j += RAD_TPB) {
    const double r = (double)pr[j], jj = (double)(j + 1);
    a4[0] += r / (jj * jj);
    a4[1] += r * (jj * jj);
    a4[2] += r * r;
    a4[3] += jj * (r / Nr);
  }
  block_reduce<RAD_TPB / 64>(a4, red, Sum{});
  double b4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = t; i < ng; i += RAD_TPB) {
    const double g = (double)pg[i], ii = (double)(i + 1);
    b4[0] += g / (ii * ii);
    b4[1] += g * (ii * ii);
    b4[2] += g * g;
    b4[3] += ii * (g / Nr);
  }
  block_reduce<RAD_TPB / 64>(b4, red, Sum{});
  const double mu_r = a4[3], mu_g = b4[3];
  double v2[2] = {0.0, 0.0};
  for (int i = t; i < ng; i += RAD_TPB) { const double c = (double)(i + 1) - mu_g; v2[0] += ((double)pg[i] / Nr) * (c * c); }
  for (int j = t; j < J; j += RAD_TPB) { const double c = (double)(j + 1) - mu_r; v2[1] += ((double)pr[j] / Nr) * (c * c); }
  block_reduce<RAD_TPB / 64>(v2, red, Sum{});
  double m5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < ng; ++i) {
    const double ii = (double)(i + 1) * (double)(i + 1);
    for (int j = t; j < J; j += RAD_TPB) {
      const unsigned c = P[(size_t)i * stride + j];
      if (c == 0u) continue;                                       // (a zero count adds +0.0 to every sum)
      const double cd = (double)c, jj = (double)(j + 1) * (double)(j + 1);
      m5[0] += rad_plogp(cd / Nr);
      m5[1] += cd / (ii * jj);
      m5[2] += cd * ii / jj;
      m5[3] += cd * jj / ii;
      m5[4] += cd * (ii * jj);
    }
  }
  block_reduce<RAD_TPB / 64>(m5, red, Sum{});
  f[0] = a4[0] / Nr;
  f[1] = a4[1] / Nr;
  f[2] = b4[2] / Nr;
  f[3] = b4[2] / (Nr * Nr);
  f[4] = a4[2] / Nr;
  f[5] = a4[2] / (Nr * Nr);
  f[6] = Nr / Np;
  f[7] = v2[0];
  f[8] = v2[1];
  f[9] = -m5[0];
  f[10] = b4[0] / Nr;
  f[11] = b4[1] / Nr;
  f[12] = m5[1] / Nr;
  f[13] = m5[2] / Nr;
  f[14] = m5[3] / Nr;
  f[15] = m5[4] / Nr;
}

// The five NGTDM features from n[i][c] and s[i][c]; all NaN when no ROI voxel has a neighbour in the ROI.
__device__ void tex_ngtdm_features(const unsigned* n, const unsigned long long* s, int ng, unsigned long long* ni, double* si,
                                   unsigned long long* total, unsigned* levels, double* red, double (&f)[5]) {
  const int t = threadIdx.x;
  if (t == 0) { *total = 0; *levels = 0; }
  __syncthreads();
  for (int i = t; i < ng; i += RAD_TPB) {
    unsigned long long c = 0;
    double v = 0.0;
    for (int k = 1; k < RADT_COLS; ++k) {
      c += n[i * RADT_COLS + k];
      v += (double)s[i * RADT_COLS + k] / (double)k;
    }
    ni[i] = c;
    si[i] = v;
    if (c) { atomicAdd(total, c); atomicAdd(levels, 1u); }
  }
  __syncthreads();
  if (*total == 0ull) {
    for (int k = 0; k < 5; ++k) f[k] = rad_nan();
    return;
  }
  const double Nvp = (double)*total, Ngp = (double)*levels;
  double s2[2] = {0.0, 0.0};
  for (int i = t; i < ng; i += RAD_TPB) {
    if (ni[i] == 0ull) continue;
    s2[0] += ((double)ni[i] / Nvp) * si[i];
    s2[1] += si[i];
  }
  block_reduce<RAD_TPB / 64>(s2, red, Sum{});
  double p4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < ng; ++i) {
    if (ni[i] == 0ull) continue;                                   // (uniform over the workgroup)
    const double pi = (double)ni[i] / Nvp, li = (double)(i + 1);
    for (int j = t; j < ng; j += RAD_TPB) {
      if (ni[j] == 0ull) continue;
      const double pj = (double)ni[j] / Nvp, lj = (double)(j + 1), dl = li - lj;
      p4[0] += pi * pj * (dl * dl);
      p4[1] += fabs(li * pi - lj * pj);
      p4[2] += fabs(dl) * (pi * si[i] + pj * si[j]) / (pi + pj);
      p4[3] += (pi + pj) * (dl * dl);
    }
  }
  block_reduce<RAD_TPB / 64>(p4, red, Sum{});
  f[0] = s2[0] == 0.0 ? 1.0e6 : 1.0 / s2[0];
  f[1] = *levels == 1u ? 0.0 : (p4[0] / (Ngp * (Ngp - 1.0))) * (s2[1] / Nvp);
  f[2] = p4[1] == 0.0 ? 0.0 : s2[0] / p4[1];
  f[3] = p4[2] / Nvp;
  f[4] = s2[1] == 0.0 ? 0.0 : p4[3] / s2[1];
}

// grid 15: workgroups 0..12 the run-length directions, 13 the dependence matrix, 14 the NGTDM
__global__ void __launch_bounds__(RAD_TPB) tex_features_kernel(const TexArgs a) {
  __shared__ unsigned long long pg[RAD_MAX_BINS], pr[RADT_LDS_L];
  __shared__ double si[RAD_MAX_BINS];
  __shared__ unsigned long long total;
  __shared__ unsigned levels;
  __shared__ double red[(RAD_TPB / 64) * 8];
  if (a.st->flagged) return;
  const int ng = a.st->n_bins, t = threadIdx.x, w = blockIdx.x;
  const double Np = (double)a.st->n;
  if (w < RAD_DIRS) {
    double f[16];
    tex_matrix_features(a.glrlm + (size_t)w * a.max_bins * a.L, (size_t)a.L, ng, a.L, Np, pg,
                        a.L <= RADT_LDS_L ? pr : a.runs + (size_t)w * a.L, &total, red, f);
    if (t == 0)
      for (int k = 0; k < RADT_NRL; ++k) a.dirf[w * RADT_NRL + k] = f[k];
  } else if (w == RAD_DIRS) {
    double f[16];
    tex_matrix_features(a.gldm, (size_t)RADT_COLS, ng, RADT_COLS, Np, pg, pr, &total, red, f);
    // SmallDependenceEmphasis, LargeDependenceEmphasis, GrayLevelNonUniformity, DependenceNonUniformity, ...Normalized,
    // GrayLevelVariance, DependenceVariance, DependenceEntropy, Low / HighGrayLevelEmphasis, the four joint emphases
    const int from[RADT_NDM] = {0, 1, 2, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    if (t == 0)
      for (int k = 0; k < RADT_NDM; ++k) a.out->gldm[k] = f[from[k]];
  } else {
    double f[5];
    tex_ngtdm_features(a.ngn, a.ngs, ng, pg, si, &total, &levels, red, f);
    if (t == 0)
      for (int k = 0; k < RADT_NGT; ++k) a.out->ngtdm[k] = f[k];
  }
}

// one workgroup: the run-length features averaged over the directions in index order; the NaN block with a flag set
__global__ void __launch_bounds__(64) tex_final_kernel(const TexArgs a) {
  const int t = threadIdx.x;
  if (a.st->flagged) {
    if (t < RADT_NRL) a.out->glrlm[t] = rad_nan();
    if (t < RADT_NDM) a.out->gldm[t] = rad_nan();
    if (t < RADT_NGT) a.out->ngtdm[t] = rad_nan();
    return;
  }
  if (t < RADT_NRL) {
    double s = a.dirf[t];
    for (int d = 1; d < RAD_DIRS; ++d) s += a.dirf[d * RADT_NRL + t];
    a.out->glrlm[t] = s / (double)RAD_DIRS;              // (no direction is empty when n > 0)
  }
}

namespace {

struct TexLayout { size_t dirf, runs, total; };

TexLayout tex_layout(int L) {
  TexLayout T;
  Carver cv;
  T.dirf = cv.take((size_t)RAD_DIRS * RADT_NRL * 8);
  T.runs = cv.take(L > RADT_LDS_L ? (size_t)RAD_DIRS * L * 8 : 0);
  T.total = cv.cur;
  return T;
}

int tex_longest(int x, int y, int z) { return x > y ? (x > z ? x : z) : (y > z ? y : z); }

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_radiomics_texture_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins) {
  if (rad_validate(x, y, z, max_bins) != 0) return -1;
  return (int64_t)tex_layout(tex_longest(x, y, z)).total;
}

int mmnn_radiomics_texture(const mmnn_radiomics_desc* d, const mmnn_radiomics_result* result, const void* ws,
                           mmnn_radiomics_texture_result* out, uint32_t* glrlm, uint32_t* gldm, uint32_t* ngtdm_n, uint64_t* ngtdm_s,
                           void* ws2, void* stream_) {
  if (rad_validate_follow("radiomics_texture", d) != 0) return 1;
  MMNN_REQUIRE(result && ws && out && glrlm && gldm && ngtdm_n && ngtdm_s && ws2, "radiomics_texture: null argument");
  MMNN_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)ws2 % 256 == 0 && (uintptr_t)result % 8 == 0 && (uintptr_t)out % 8 == 0 &&
                   (uintptr_t)glrlm % 4 == 0 && (uintptr_t)gldm % 4 == 0 && (uintptr_t)ngtdm_n % 4 == 0 && (uintptr_t)ngtdm_s % 8 == 0,
               "radiomics_texture: misaligned workspace / result / table");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int L = tex_longest(d->x, d->y, d->z);
  const TexLayout T = tex_layout(L);
  char* ws2b = static_cast<char*>(ws2);
  TexArgs a{};
  static_cast<RadFollow&>(a) = rad_follow(d, ws);
  const long n = (long)a.N;
  a.L = L;
  a.max_bins = d->max_bins;
  a.glrlm = glrlm; a.gldm = gldm; a.ngn = ngtdm_n;
  a.ngs = reinterpret_cast<unsigned long long*>(ngtdm_s);
  a.dirf = reinterpret_cast<double*>(ws2b + T.dirf);
  a.runs = reinterpret_cast<unsigned long long*>(ws2b + T.runs);
  a.out = out;
  const size_t cells = (size_t)d->max_bins * RADT_COLS;
  int run_chunks = cdiv(n, 4 * RAD_TPB), nbhd_chunks = cdiv(n, 4 * RAD_TPB);
  if (run_chunks > RADT_RUN_CHUNKS) run_chunks = RADT_RUN_CHUNKS;
  if (nbhd_chunks > RADT_NBHD_CHUNKS) nbhd_chunks = RADT_NBHD_CHUNKS;

  MMNN_HIP(hipMemsetAsync(glrlm, 0, (size_t)RAD_DIRS * d->max_bins * L * 4, stream));
  MMNN_HIP(hipMemsetAsync(gldm, 0, cells * 4, stream));
  MMNN_HIP(hipMemsetAsync(ngtdm_n, 0, cells * 4, stream));
  MMNN_HIP(hipMemsetAsync(ngtdm_s, 0, cells * 8, stream));
  MMNN_LAUNCH(glrlm_count_kernel, dim3(run_chunks, RAD_DIRS), dim3(RAD_TPB), (size_t)RADT_RUN_WORDS * 4, stream, a);
  MMNN_LAUNCH(nbhd_count_kernel, dim3(nbhd_chunks), dim3(RAD_TPB), (size_t)RADT_NBHD_NG * RADT_COLS * 16, stream, a);
  MMNN_LAUNCH(tex_features_kernel, dim3(RAD_DIRS + 2), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(tex_final_kernel, dim3(1), dim3(64), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
