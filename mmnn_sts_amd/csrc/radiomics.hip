// Radiomic features of one (scan, mask) pair: first-order statistics, the intensity histogram, exact order statistics and the 13
// grey-level co-occurrence matrices with their 23 features (the contract is the comment above mmnn_radiomics in include/mmnn_sts.h).
// Scan and mask are read in their on-disk types through the ingest's typed loads; no float copy of the volume is written.  Everything
// is enqueued on the caller's stream, later kernels read what earlier ones decided (flags, Ng, the mean, the radix prefixes) from a
// small state block in the workspace, and the host never waits.
//
//   memsets               hist, glcm, the radix histograms
//   rad_pass<1>           n, bounding box, index moments, sum v, sum v^2, min, max, the non-finite flag; radix digit 0 (bits 63..48)
//   rad_step<1>           flags, mean, low edge, Ng, the ten ranks; radix prefix after digit 0
//   rad_pass<2>           sum |v - mean|, (v - mean)^2, ^3, ^4; the histogram (privatised in LDS per workgroup); the bin of every voxel as uint16 (0: outside the ROI);
//                         radix digit 1
//   rad_pass<3>, <4>      radix digits 2 and 3, each followed by its rad_step: after the last the prefixes ARE the order statistics
//   glcm_count_kernel     the 13 matrices from the bin volume: uint32 atomics on a matrix privatised in LDS when Ng <= RAD_LDS_NG,
//                         on global memory otherwise
//   rad_pass<5>, <6>      the robust mean absolute deviation: count and sum inside [p10, p90], then sum |v - mean_10-90|
//   glcm_features_kernel  one workgroup per direction: marginals by integer LDS atomics, then the fp64 sums in a fixed order
//   rad_final_kernel      the 17 first-order features, Entropy / Uniformity from the histogram, the direction average
//
// Determinism.  Every integer (counts, moments, histograms, matrices, radix histograms) is accumulated exactly, so the order of the
// atomics does not show.  Every fp64 sum runs over a partition that depends on the extents only: a lane adds its voxels in ascending
// order, a wave folds its lanes by the xor butterfly, the four waves of a workgroup and then the RAD_PARTS workgroups are added in index
// order.  No floating-point atomics anywhere.
#include "ingest_load.hpp"
#include "radiomics.hpp"

#include <cmath>

namespace mmnn {

struct RadArgs {
  const void* scan; const void* mask;
  int X, Y, Z;
  long N;
  int stype, mtype;
  IgScale ss, ms;
  double bw;
  int max_bins;
  int parts;
  mmnn_radiomics_result* res;
  unsigned* hist; unsigned* glcm;
  RadState* st;
  unsigned long long* part;                 // [RAD_SLOTS][RAD_MAX_PARTS]
  unsigned* rhist;                          // [RAD_RANKS][RAD_DIGITS]
  uint16_t* bins;                           // [N]
  double* dirf;                             // [RAD_DIRS][RAD_NF + 1]: the features of a direction, then 1.0 when its matrix is not empty
};

// order-preserving 64-bit key of a double (-0.0 is keyed, and so returned, as +0.0)
__device__ __forceinline__ unsigned long long rad_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v == 0.0 ? 0.0 : v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double rad_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// bin of v: floor((v - low) / bw) + 1 in fp64, held inside 1..65535 (a low edge that rounds above the minimum would give 0)
__device__ __forceinline__ int rad_bin(double v, double low, double bw) {
  const double b = floor((v - low) / bw) + 1.0;
  return b < 1.0 ? 1 : (b > 65535.0 ? 65535 : (int)b);
}

enum { RS_N = 0, RS_LO = 1, RS_HI = 4, RS_MOM = 7, RS_BAD = 16, RS_SUM = 17, RS_SQ = 18, RS_MIN = 19, RS_MAX = 20 };

__device__ __forceinline__ unsigned long long rad_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ unsigned long long rad_bits(long long v) { return (unsigned long long)v; }

// ---- the voxel passes ----------------------------------------------------------------------------------------------------------
// grid a.parts workgroups of RAD_TPB lanes; the volume is flat, group g = VEC consecutive voxels (VEC > 1 only when N % VEC == 0 and both
// buffers are aligned to VEC elements).  Workgroup b takes the groups b * TPB + t, + parts * TPB, ...: the trip count is the same in
// every lane of a workgroup, so the ballots inside rad_count see whole waves.
template <int PHASE, int VEC>
__global__ void __launch_bounds__(RAD_TPB) rad_pass_kernel(const RadArgs a) {
  __shared__ unsigned long long red[(RAD_TPB / 64) * RAD_SLOTS];
  __shared__ unsigned lhist[PHASE == 2 ? RAD_MAX_BINS : 1];          // the workgroup's own histogram: Ng <= max_bins <= RAD_MAX_BINS
  const RadState st = PHASE > 1 ? *a.st : RadState{};
  if (PHASE > 1 && st.flagged) return;
  if (PHASE == 2) {
    for (int b = threadIdx.x; b < st.n_bins; b += RAD_TPB) lhist[b] = 0u;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long G = a.N / VEC;
  const long XY = (long)a.X * a.Y;
  long long cnt = 0, lo[3] = {a.X, a.Y, a.Z}, hi[3] = {-1, -1, -1}, mom[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bad = 0;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  double vmin = INFINITY, vmax = -INFINITY;
  const int shift = PHASE == 1 ? 48 : (PHASE == 2 ? 32 : (PHASE == 3 ? 16 : 0));
  for (long g0 = (long)blockIdx.x * RAD_TPB; g0 < G; g0 += (long)a.parts * RAD_TPB) {
    const long g = g0 + threadIdx.x;
    const bool in = g < G;
    double sv[VEC], mv[VEC];
    if (in) {
      ig_load<VEC>(a.scan, a.stype, g * VEC, sv);
      ig_load<VEC>(a.mask, a.mtype, g * VEC, mv);
    }
    uint16_t bq[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const bool roi = in && !(ig_scaled(mv[k], a.ms) == 0.0);
      const double v = roi ? ig_scaled(sv[k], a.ss) : 0.0;
      const unsigned long long key = rad_key(v);
      bq[k] = 0;
      if (PHASE == 1) {
        if (roi) {
          const long idx = g * VEC + k;
          const long long z = idx / XY, r = idx - z * XY, y = r / a.X, x = r - y * a.X;
          ++cnt;
          lo[0] = x < lo[0] ? x : lo[0]; lo[1] = y < lo[1] ? y : lo[1]; lo[2] = z < lo[2] ? z : lo[2];
          hi[0] = x > hi[0] ? x : hi[0]; hi[1] = y > hi[1] ? y : hi[1]; hi[2] = z > hi[2] ? z : hi[2];
          mom[0] += x; mom[1] += y; mom[2] += z; mom[3] += x * x; mom[4] += y * y; mom[5] += z * z;
          mom[6] += x * y; mom[7] += x * z; mom[8] += y * z;
          if (!isfinite(v)) bad = 1;
          s[0] += v;
          s[1] += v * v;
          vmin = v < vmin ? v : vmin;
          vmax = v > vmax ? v : vmax;
        }
        rad_count(a.rhist, (unsigned)(key >> 48), roi);
      } else if (PHASE <= 4) {
        if (PHASE == 2 && roi) {
          const double d = v - st.mean, d2 = d * d;
          s[0] += fabs(d); s[1] += d2; s[2] += d2 * d; s[3] += d2 * d2;
          const int b = rad_bin(v, st.low, st.bw);
          bq[k] = (uint16_t)(b < st.n_bins ? b : st.n_bins);      // (b <= Ng already: the bin is monotone in v)
        }
        if (PHASE == 2 && roi) atomicAdd(&lhist[bq[k] - 1], 1u);
        const unsigned digit = (unsigned)(key >> shift) & 0xffffu;
        for (int r = 0; r < RAD_RANKS; ++r) {          // (uniform: the state is the same in every lane)
          if (st.rep[r] != r) continue;
          rad_count(a.rhist + (long)r * RAD_DIGITS, digit, roi && (key >> (shift + 16)) == (st.prefix[r] >> (shift + 16)));
        }
      } else if (PHASE == 5) {
        if (roi && v >= st.p10 && v <= st.p90) { ++cnt; s[0] += v; }
      } else {
        if (roi && v >= st.p10 && v <= st.p90) s[0] += fabs(v - st.rob_mean);
      }
    }
    if (PHASE == 2 && in) {
      if constexpr (VEC == 4) {
        IgVec<uint16_t, 4> o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.e[k] = bq[k];
        *reinterpret_cast<IgVec<uint16_t, 4>*>(a.bins + g * 4) = o;
      } else {
        a.bins[g] = bq[0];
      }
    }
  }
  if (PHASE == 3 || PHASE == 4) return;
  if (PHASE == 2) {
    __syncthreads();
    for (int b = threadIdx.x; b < st.n_bins; b += RAD_TPB) {
      const unsigned c = lhist[b];
      if (c) atomicAdd(&a.hist[b], c);
    }
  }
  // workgroup partials: slot q of workgroup b at part[q * RAD_MAX_PARTS + b]
  unsigned long long w[RAD_SLOTS];
  int nq = 0;
  if (PHASE == 1) {
    w[RS_N] = rad_bits(wave_sum(cnt));
    for (int k = 0; k < 3; ++k) { w[RS_LO + k] = rad_bits(wave_reduce(lo[k], Less{})); w[RS_HI + k] = rad_bits(wave_reduce(hi[k], Greater{})); }
    for (int k = 0; k < 9; ++k) w[RS_MOM + k] = rad_bits(wave_sum(mom[k]));
    w[RS_BAD] = rad_bits(wave_reduce(bad, Greater{}));
    w[RS_SUM] = rad_bits(wave_sum(s[0])); w[RS_SQ] = rad_bits(wave_sum(s[1]));
    w[RS_MIN] = rad_bits(wave_reduce(vmin, Less{})); w[RS_MAX] = rad_bits(wave_reduce(vmax, Greater{}));
    nq = 21;
  } else if (PHASE == 2) {
    for (int k = 0; k < 4; ++k) w[k] = rad_bits(wave_sum(s[k]));
    nq = 4;
  } else if (PHASE == 5) {
    w[0] = rad_bits(wave_sum(cnt)); w[1] = rad_bits(wave_sum(s[0]));
    nq = 2;
  } else {
    w[0] = rad_bits(wave_sum(s[0]));
    nq = 1;
  }
  if (lane == 0)
    for (int q = 0; q < nq; ++q) red[wave * RAD_SLOTS + q] = w[q];
  __syncthreads();
  if ((int)threadIdx.x < nq) {
    const int q = threadIdx.x;
    const bool is_int = (PHASE == 1 && q <= RS_BAD) || (PHASE == 5 && q == 0);
    unsigned long long out;
    if (is_int) {
      long long t = (long long)red[q];
      for (int v = 1; v < RAD_TPB / 64; ++v) {
        const long long u = (long long)red[v * RAD_SLOTS + q];
        if (PHASE == 1 && q >= RS_LO && q < RS_HI) t = u < t ? u : t;
        else if (PHASE == 1 && ((q >= RS_HI && q < RS_MOM) || q == RS_BAD)) t = u > t ? u : t;
        else t += u;
      }
      out = (unsigned long long)t;
    } else {
      double t = __longlong_as_double((long long)red[q]);
      for (int v = 1; v < RAD_TPB / 64; ++v) {
        const double u = __longlong_as_double((long long)red[v * RAD_SLOTS + q]);
        if (PHASE == 1 && q == RS_MIN) t = u < t ? u : t;
        else if (PHASE == 1 && q == RS_MAX) t = u > t ? u : t;
        else t += u;
      }
      out = rad_bits(t);
    }
    a.part[(long)q * RAD_MAX_PARTS + blockIdx.x] = out;
  }
}

// ---- the steps between the passes: one workgroup ---------------------------------------------------------------------------------
// slot q of every workgroup, folded in workgroup order
__device__ __forceinline__ long long rad_fold_sum_i(const RadArgs& a, int q) {
  long long t = 0;
  for (int b = 0; b < a.parts; ++b) t += (long long)a.part[(long)q * RAD_MAX_PARTS + b];
  return t;
}
__device__ __forceinline__ double rad_fold_sum_d(const RadArgs& a, int q) {
  double t = __longlong_as_double((long long)a.part[(long)q * RAD_MAX_PARTS]);
  for (int b = 1; b < a.parts; ++b) t += __longlong_as_double((long long)a.part[(long)q * RAD_MAX_PARTS + b]);
  return t;
}

// The radix digit of every rank: in histogram h of RAD_DIGITS counts, the smallest digit d with count(0..d) > k.  All threads call it;
// the result and the count below d are left in lds64[0], lds64[1].  scan: RAD_TPB words of LDS.
__device__ void rad_select_digit(const unsigned* h, unsigned long long k, unsigned long long* scan, unsigned long long* lds64) {
  constexpr int PER = RAD_DIGITS / RAD_TPB;
  const int t = threadIdx.x;
  unsigned long long own = 0;
  for (int i = 0; i < PER; ++i) own += h[t * PER + i];
  __syncthreads();
  scan[t] = own;
  __syncthreads();
  for (int o = 1; o < RAD_TPB; o <<= 1) {
    const unsigned long long add = t >= o ? scan[t - o] : 0ull;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const unsigned long long incl = scan[t], excl = incl - own;
  if (t == 0) { lds64[0] = RAD_DIGITS - 1; lds64[1] = 0; }      // (k beyond the counts cannot happen: k < n; a safe answer all the same)
  __syncthreads();
  if (excl <= k && k < incl) {
    unsigned long long c = excl;
    int d = t * PER;
    for (; d < t * PER + PER - 1; ++d) {
      const unsigned long long e = h[d];
      if (k < c + e) break;
      c += e;
    }
    lds64[0] = (unsigned long long)d;
    lds64[1] = c;
  }
  __syncthreads();
}

template <int PHASE>
__global__ void __launch_bounds__(RAD_TPB) rad_step_kernel(const RadArgs a) {
  __shared__ unsigned long long scan[RAD_TPB];
  __shared__ unsigned long long sel[2];
  __shared__ unsigned long long fold[RAD_SLOTS];
  __shared__ RadState st;
  const int t = threadIdx.x;
  if (PHASE > 1) {
    if (t == 0) st = *a.st;
    __syncthreads();
    if (st.flagged) return;
  }
  if (PHASE == 1) {
    if (t <= RS_MAX) {
      unsigned long long out;
      if (t >= RS_SUM) {
        double v = __longlong_as_double((long long)a.part[(long)t * RAD_MAX_PARTS]);
        for (int b = 1; b < a.parts; ++b) {
          const double u = __longlong_as_double((long long)a.part[(long)t * RAD_MAX_PARTS + b]);
          if (t == RS_MIN) v = u < v ? u : v;
          else if (t == RS_MAX) v = u > v ? u : v;
          else v += u;
        }
        out = rad_bits(v);
      } else {
        long long v = (long long)a.part[(long)t * RAD_MAX_PARTS];
        for (int b = 1; b < a.parts; ++b) {
          const long long u = (long long)a.part[(long)t * RAD_MAX_PARTS + b];
          if (t >= RS_LO && t < RS_HI) v = u < v ? u : v;
          else if ((t >= RS_HI && t < RS_MOM) || t == RS_BAD) v = u > v ? u : v;
          else v += u;
        }
        out = (unsigned long long)v;
      }
      fold[t] = out;
    }
    __syncthreads();
    if (t == 0) {
      mmnn_radiomics_result* r = a.res;
      const long long n = (long long)fold[RS_N];
      const bool empty = n == 0, nonfinite = fold[RS_BAD] != 0;
      RadState s{};
      s.n = n;
      s.bw = a.bw;
      s.sum = __longlong_as_double((long long)fold[RS_SUM]); s.sumsq = __longlong_as_double((long long)fold[RS_SQ]);
      s.vmin = __longlong_as_double((long long)fold[RS_MIN]); s.vmax = __longlong_as_double((long long)fold[RS_MAX]);
      bool overflow = false;
      if (!empty && !nonfinite) {
        s.mean = s.sum / (double)n;
        s.low = floor(s.vmin / a.bw) * a.bw;
        const double ng = floor((s.vmax - s.low) / a.bw) + 1.0;
        overflow = !(ng <= (double)a.max_bins);
        s.n_bins = overflow ? (ng < 2147483647.0 ? (int)ng : 2147483647) : (ng < 1.0 ? 1 : (int)ng);
        const double pct[5] = {10.0, 25.0, 50.0, 75.0, 90.0};
        for (int i = 0; i < 5; ++i) {
          const double h = (double)(n - 1) * pct[i] / 100.0;
          s.rank[2 * i] = (unsigned long long)floor(h);
          s.rank[2 * i + 1] = (unsigned long long)ceil(h);
        }
      }
      s.flagged = empty || nonfinite || overflow;
      r->n = n;
      for (int k = 0; k < 3; ++k) { r->lo[k] = empty ? 0 : (long long)fold[RS_LO + k]; r->hi[k] = empty ? 0 : (long long)fold[RS_HI + k]; }
      for (int k = 0; k < 9; ++k) r->moments[k] = (long long)fold[RS_MOM + k];
      r->n_bins = s.n_bins;
      r->overflow = overflow; r->nonfinite = nonfinite; r->empty = empty;
      const double nan = rad_nan();
      for (int k = 0; k < RAD_RANKS; ++k) r->order[k] = nan;
      for (int k = 0; k < MMNN_RADIOMICS_FIRSTORDER; ++k) r->firstorder[k] = nan;
      for (int k = 0; k < RAD_NF; ++k) r->glcm[k] = nan;
      st = s;
    }
    __syncthreads();
    if (st.flagged) {
      if (t == 0) *a.st = st;
      return;
    }
  } else if (PHASE == 2) {
    if (t < 4) fold[t] = rad_bits(rad_fold_sum_d(a, t));
    __syncthreads();
    if (t == 0)
      for (int k = 0; k < 4; ++k) st.cen[k] = __longlong_as_double((long long)fold[k]);
    __syncthreads();
  } else if (PHASE == 5) {
    if (t == 0) {
      st.rob_n = rad_fold_sum_i(a, 0);
      st.rob_sum = rad_fold_sum_d(a, 1);
      st.rob_mean = st.rob_sum / (double)st.rob_n;
      *a.st = st;
    }
    return;
  } else if (PHASE == 6) {
    if (t == 0) {
      st.rob_abs = rad_fold_sum_d(a, 0);
      *a.st = st;
    }
    return;
  }
  // phases 1..4: one more radix digit for every rank.  Phase 1 filled histogram 0 only (no prefix yet).
  const int shift = PHASE == 1 ? 48 : (PHASE == 2 ? 32 : (PHASE == 3 ? 16 : 0));
  for (int r = 0; r < RAD_RANKS; ++r) {
    const int src = PHASE == 1 ? 0 : st.rep[r];
    // ranks that share a prefix share a histogram but not the rank inside it
    rad_select_digit(a.rhist + (long)src * RAD_DIGITS, st.rank[r], scan, sel);
    if (t == 0) {
      st.prefix[r] |= sel[0] << shift;
      st.rank[r] -= sel[1];
    }
    __syncthreads();
  }
  if (t == 0) {
    for (int r = 0; r < RAD_RANKS; ++r) {
      int rep = r;
      for (int q = 0; q < r; ++q)
        if (st.prefix[q] == st.prefix[r]) { rep = q; break; }
      st.rep[r] = rep;
    }
    if (PHASE == 4) {
      double o[RAD_RANKS];
      for (int r = 0; r < RAD_RANKS; ++r) { o[r] = rad_unkey(st.prefix[r]); a.res->order[r] = o[r]; }
      const double pct[5] = {10.0, 25.0, 50.0, 75.0, 90.0};
      double q[5];
      for (int i = 0; i < 5; ++i) {
        const double h = (double)(st.n - 1) * pct[i] / 100.0;
        q[i] = o[2 * i] + (o[2 * i + 1] - o[2 * i]) * (h - floor(h));
      }
      st.p10 = q[0]; st.p90 = q[4];
      double* f = a.res->firstorder;
      f[10] = q[0]; f[11] = q[4]; f[12] = q[2]; f[13] = q[3] - q[1];
    }
    *a.st = st;
  }
}

// ---- co-occurrence counting -------------------------------------------------------------------------------------------------------
// grid (RAD_GLCM_CHUNKS, 13); dynamic LDS RAD_LDS_NG^2 words.  Workgroup (c, d) walks the voxels c * TPB + t, + CHUNKS * TPB, ... of the
// bin volume for direction d.  Ng is known on the device only, so the choice between the two variants is made here: the LDS matrix
// (row stride Ng, zeroed by the workgroup, its non-zero entries added to the global matrix at the end) or adds on global memory.
__global__ void __launch_bounds__(RAD_TPB) glcm_count_kernel(const RadArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned rad_lds[];
  if (a.st->flagged) return;
  const int ng = a.st->n_bins;
  const bool in_lds = ng <= RAD_LDS_NG;
  const int d = blockIdx.y;
  const int dz = rad_dirs[d][0], dy = rad_dirs[d][1], dx = rad_dirs[d][2];
  unsigned* G = a.glcm + (long)d * a.max_bins * a.max_bins;
  if (in_lds) {
    for (int e = threadIdx.x; e < ng * ng; e += RAD_TPB) rad_lds[e] = 0u;
    __syncthreads();
  }
  const long XY = (long)a.X * a.Y;
  const long off = ((long)dz * a.Y + dy) * a.X + dx;
  for (long idx = (long)blockIdx.x * RAD_TPB + threadIdx.x; idx < a.N; idx += (long)RAD_GLCM_CHUNKS * RAD_TPB) {
    const int ba = a.bins[idx];
    if (ba == 0) continue;
    const long z = idx / XY, r = idx - z * XY, y = r / a.X, x = r - y * a.X;
    const long nx = x + dx, ny = y + dy, nz = z + dz;
    if (nx < 0 || nx >= a.X || ny < 0 || ny >= a.Y || nz >= a.Z) continue;      // (dz >= 0)
    const int bb = a.bins[idx + off];
    if (bb == 0) continue;
    const int i = ba - 1, j = bb - 1;                    // both below ng: the pass that wrote the bins ran only without overflow
    if (i >= ng || j >= ng) continue;
    if (in_lds) {
      atomicAdd(&rad_lds[i * ng + j], 1u);
      atomicAdd(&rad_lds[j * ng + i], 1u);
    } else {
      atomicAdd(&G[(long)i * a.max_bins + j], 1u);
      atomicAdd(&G[(long)j * a.max_bins + i], 1u);
    }
  }
  if (in_lds) {
    __syncthreads();
    for (int e = threadIdx.x; e < ng * ng; e += RAD_TPB) {
      const unsigned c = rad_lds[e];
      if (c) atomicAdd(&G[(long)(e / ng) * a.max_bins + e % ng], c);
    }
  }
}

// ---- co-occurrence features: one workgroup per direction --------------------------------------------------------------------------
__global__ void __launch_bounds__(RAD_TPB) glcm_features_kernel(const RadArgs a) {
  __shared__ unsigned long long row[RAD_MAX_BINS], plus[2 * RAD_MAX_BINS], minus[RAD_MAX_BINS];
  __shared__ unsigned long long total;
  __shared__ unsigned cmax;
  __shared__ double red[(RAD_TPB / 64) * 8];
  if (a.st->flagged) return;
  const int ng = a.st->n_bins, t = threadIdx.x, d = blockIdx.x;
  const unsigned* G = a.glcm + (long)d * a.max_bins * a.max_bins;
  double* out = a.dirf + (long)d * (RAD_NF + 1);
  for (int i = t; i < ng; i += RAD_TPB) { row[i] = 0; minus[i] = 0; }
  for (int i = t; i < 2 * ng; i += RAD_TPB) plus[i] = 0;
  if (t == 0) { total = 0; cmax = 0; }
  __syncthreads();
  // the marginals as integers: exact, whatever the order
  const long E = (long)ng * ng;
  unsigned long long own = 0;
  unsigned omax = 0;
  for (long e = t; e < E; e += RAD_TPB) {
    const int i = (int)(e / ng), j = (int)(e - (long)i * ng);
    const unsigned c = G[(long)i * a.max_bins + j];
    if (c == 0u) continue;
    own += c;
    omax = c > omax ? c : omax;
    atomicAdd(&row[i], (unsigned long long)c);
    atomicAdd(&plus[i + j], (unsigned long long)c);           // k = i + j + 2
    atomicAdd(&minus[i > j ? i - j : j - i], (unsigned long long)c);
  }
  if (own) atomicAdd(&total, own);
  if (omax) atomicMax(&cmax, omax);
  __syncthreads();
  if (total == 0ull) {
    if (t <= RAD_NF) out[t] = 0.0;
    return;
  }
  const double S = (double)total, Ng = (double)ng;
  // the marginal row sums: mu, then sigma^2 and HX
  double m1[1] = {0.0};
  for (int i = t; i < ng; i += RAD_TPB) m1[0] += (double)(i + 1) * ((double)row[i] / S);
  block_reduce<RAD_TPB / 64>(m1, red, Sum{});
  const double mu = m1[0];
  double m2[2] = {0.0, 0.0};
  for (int i = t; i < ng; i += RAD_TPB) {
    const double px = (double)row[i] / S, di = (double)(i + 1) - mu;
    m2[0] += di * di * px;
    m2[1] += rad_plogp(px);
  }
  block_reduce<RAD_TPB / 64>(m2, red, Sum{});
  const double var = m2[0], HX = -m2[1];
  // the matrix: autocorrelation, joint energy, HXY, HXY1, HXY2
  double m5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long e = t; e < E; e += RAD_TPB) {
    const int i = (int)(e / ng), j = (int)(e - (long)i * ng);
    const double p = (double)G[(long)i * a.max_bins + j] / S;
    const double pp = ((double)row[i] / S) * ((double)row[j] / S), lg = log2(pp + RAD_EPS);
    m5[0] += p * (double)(i + 1) * (double)(j + 1);
    m5[1] += p * p;
    m5[2] += rad_plogp(p);
    m5[3] += p * lg;
    m5[4] += pp * lg;
  }
  block_reduce<RAD_TPB / 64>(m5, red, Sum{});
  const double autoc = m5[0], HXY = -m5[2], HXY1 = -m5[3], HXY2 = -m5[4];
  // p+(k), k = 2..2Ng
  double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = t; q < 2 * ng - 1; q += RAD_TPB) {
    const double p = (double)plus[q] / S, k = (double)(q + 2), c = k - 2.0 * mu, c2 = c * c;
    s5[0] += k * p;
    s5[1] += rad_plogp(p);
    s5[2] += c2 * p;
    s5[3] += c2 * c * p;
    s5[4] += c2 * c2 * p;
  }
  block_reduce<RAD_TPB / 64>(s5, red, Sum{});
  // p-(k), k = 0..Ng-1
  double d8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = t; q < ng; q += RAD_TPB) {
    const double p = (double)minus[q] / S, k = (double)q;
    d8[0] += k * p;
    d8[1] += rad_plogp(p);
    d8[2] += k * k * p;
    d8[3] += p / (1.0 + k * k);
    d8[4] += p / (1.0 + k * k / (Ng * Ng));
    d8[5] += p / (1.0 + k);
    d8[6] += p / (1.0 + k / Ng);
    if (q >= 1) d8[7] += p / (k * k);
  }
  block_reduce<RAD_TPB / 64>(d8, red, Sum{});
  const double DA = d8[0];
  double dv[1] = {0.0};
  for (int q = t; q < ng; q += RAD_TPB) {
    const double p = (double)minus[q] / S, c = (double)q - DA;
    dv[0] += c * c * p;
  }
  block_reduce<RAD_TPB / 64>(dv, red, Sum{});
  if (t == 0) {
    out[0] = autoc;
    out[1] = mu;
    out[2] = s5[4];
    out[3] = s5[3];
    out[4] = s5[2];
    out[5] = d8[2];
    out[6] = var == 0.0 ? 1.0 : (autoc - mu * mu) / var;
    out[7] = DA;
    out[8] = -d8[1];
    out[9] = dv[0];
    out[10] = m5[1];
    out[11] = HXY;
    out[12] = HX == 0.0 ? 0.0 : (HXY - HXY1) / HX;
    out[13] = HXY > HXY2 ? 0.0 : sqrt(1.0 - exp(-2.0 * (HXY2 - HXY)));
    out[14] = d8[3];
    out[15] = d8[4];
    out[16] = d8[5];
    out[17] = d8[6];
    out[18] = d8[7];
    out[19] = (double)cmax / S;
    out[20] = s5[0];
    out[21] = -s5[1];
    out[22] = var;
    out[RAD_NF] = 1.0;
  }
}

// ---- the end: one workgroup --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RAD_TPB) rad_final_kernel(const RadArgs a) {
  __shared__ double red[(RAD_TPB / 64) * 2];
  if (a.st->flagged) return;
  const RadState st = *a.st;
  const int t = threadIdx.x;
  const double n = (double)st.n;
  double h2[2] = {0.0, 0.0};
  for (int b = t; b < st.n_bins; b += RAD_TPB) {
    const double p = (double)a.hist[b] / n;
    h2[0] += rad_plogp(p);
    h2[1] += p * p;
  }
  block_reduce<RAD_TPB / 64>(h2, red, Sum{});
  if (t == 0) {
    double* f = a.res->firstorder;
    const double m2 = st.cen[1] / n, m3 = st.cen[2] / n, m4 = st.cen[3] / n;
    f[0] = st.sumsq;
    f[1] = st.vmin;
    f[2] = st.vmax;
    f[3] = st.vmax - st.vmin;
    f[4] = st.mean;
    f[5] = m2;
    f[6] = m2 == 0.0 ? 0.0 : m3 / pow(m2, 1.5);
    f[7] = m2 == 0.0 ? 0.0 : m4 / (m2 * m2);
    f[8] = st.cen[0] / n;
    f[9] = sqrt(st.sumsq / n);
    f[14] = st.rob_abs / (double)st.rob_n;
    f[15] = -h2[0];
    f[16] = h2[1];
  } else if (t >= 64 && t < 64 + RAD_NF) {
    const int k = t - 64;
    double s = 0.0, c = 0.0;
    for (int d = 0; d < RAD_DIRS; ++d) {
      const double* df = a.dirf + (long)d * (RAD_NF + 1);
      if (df[RAD_NF] != 0.0) { s += df[k]; c += 1.0; }
    }
    if (c > 0.0) a.res->glcm[k] = s / c;          // (no direction with a pair: the NaN of rad_step<1> stays)
  }
}

namespace {

template <int PHASE>
void rad_launch_pass(const RadArgs& a, bool vec4, hipStream_t stream) {
  const auto pass = vec4 ? rad_pass_kernel<PHASE, 4> : rad_pass_kernel<PHASE, 1>;
  MMNN_LAUNCH(pass, dim3(a.parts), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(rad_step_kernel<PHASE>, dim3(1), dim3(RAD_TPB), 0, stream, a);
}

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_radiomics_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins) {
  if (rad_validate(x, y, z, max_bins) != 0) return -1;
  return (int64_t)rad_layout((long)x * y * z).total;
}

int mmnn_radiomics(const mmnn_radiomics_desc* d, const void* scan, const void* mask, mmnn_radiomics_result* result, uint32_t* hist,
                   uint32_t* glcm, void* ws, void* stream_) {
  MMNN_REQUIRE(d, "radiomics: null descriptor");
  if (rad_validate(d->x, d->y, d->z, d->max_bins) != 0) return 1;
  const int ssz = ig_type_size(d->scan_type), msz = ig_type_size(d->mask_type);
  MMNN_REQUIRE(ssz != 0, "radiomics: unsupported scan datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->scan_type);
  MMNN_REQUIRE(msz != 0, "radiomics: unsupported mask datatype code %d (2, 4, 8, 16, 64, 256, 512, 768 are)", d->mask_type);
  MMNN_REQUIRE(std::isfinite(d->bin_width) && d->bin_width > 0.0, "radiomics: bin_width must be finite and positive");
  MMNN_REQUIRE(scan && mask && result && hist && glcm && ws, "radiomics: null argument");
  MMNN_REQUIRE((uintptr_t)scan % ssz == 0 && (uintptr_t)mask % msz == 0, "radiomics: scan / mask buffer not aligned to its element size");
  MMNN_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)result % 8 == 0 && (uintptr_t)hist % 4 == 0 && (uintptr_t)glcm % 4 == 0,
               "radiomics: misaligned workspace / result / hist / glcm");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const long n = (long)d->x * d->y * d->z;
  const RadLayout L = rad_layout(n);
  char* wsb = static_cast<char*>(ws);
  RadArgs a{};
  a.scan = scan; a.mask = mask;
  a.X = d->x; a.Y = d->y; a.Z = d->z; a.N = n;
  a.stype = d->scan_type; a.mtype = d->mask_type;
  a.ss = rad_scale(d->scan_slope, d->scan_inter);
  a.ms = rad_scale(d->mask_slope, d->mask_inter);
  a.bw = d->bin_width;
  a.max_bins = d->max_bins;
  a.res = result; a.hist = hist; a.glcm = glcm;
  a.st = reinterpret_cast<RadState*>(wsb + L.state);
  a.part = reinterpret_cast<unsigned long long*>(wsb + L.part);
  a.rhist = reinterpret_cast<unsigned*>(wsb + L.rhist);
  a.dirf = reinterpret_cast<double*>(wsb + L.dirf);
  a.bins = reinterpret_cast<uint16_t*>(wsb + L.bins);
  // 4 voxels per lane when the flat volume divides and both buffers start on a 4-element boundary
  const bool vec4 = n % 4 == 0 && (uintptr_t)scan % (4 * ssz) == 0 && (uintptr_t)mask % (4 * msz) == 0;
  a.parts = cdiv(n / (vec4 ? 4 : 1), 4 * RAD_TPB);
  if (a.parts > RAD_MAX_PARTS) a.parts = RAD_MAX_PARTS;
  if (a.parts < 1) a.parts = 1;
  const size_t rbytes = (size_t)RAD_RANKS * RAD_DIGITS * 4;

  MMNN_HIP(hipMemsetAsync(hist, 0, (size_t)d->max_bins * 4, stream));
  MMNN_HIP(hipMemsetAsync(glcm, 0, (size_t)RAD_DIRS * d->max_bins * d->max_bins * 4, stream));
  MMNN_HIP(hipMemsetAsync(a.rhist, 0, rbytes, stream));
  rad_launch_pass<1>(a, vec4, stream);
  MMNN_HIP(hipMemsetAsync(a.rhist, 0, rbytes, stream));
  rad_launch_pass<2>(a, vec4, stream);
  MMNN_LAUNCH(glcm_count_kernel, dim3(RAD_GLCM_CHUNKS, RAD_DIRS), dim3(RAD_TPB), (size_t)RAD_LDS_NG * RAD_LDS_NG * 4, stream, a);
  MMNN_HIP(hipMemsetAsync(a.rhist, 0, rbytes, stream));
  rad_launch_pass<3>(a, vec4, stream);
  MMNN_HIP(hipMemsetAsync(a.rhist, 0, rbytes, stream));
  rad_launch_pass<4>(a, vec4, stream);
  rad_launch_pass<5>(a, vec4, stream);
  rad_launch_pass<6>(a, vec4, stream);
  MMNN_LAUNCH(glcm_features_kernel, dim3(RAD_DIRS), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(rad_final_kernel, dim3(1), dim3(RAD_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
