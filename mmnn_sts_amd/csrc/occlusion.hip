// Occlusion sensitivity: the occluded batches and the map assembled from the model's scores (the contract is the comment above
// mmnn_occlusion_window_count in include/mmnn_sts.h).
//
//   occlude_windows_kernel<VEC>  the streaming hot path: `count` copies of the input with one window each replaced by the channel's
//                         fill value.  grid.y walks the (sample, channel) pairs, grid.x the rows (z, y) of one of them with LW lanes
//                         each, lanes along w.  The pair is uniform over a block, so the decode of the sample's window (two
//                         divisions, three origins) is scalar work; a thread decodes its row with one 32-bit division, folds the
//                         d / h test into the w range ([lo, hi) is empty for a row the window does not meet) and then walks the row,
//                         where the per-voxel work is one select between the loaded value and the fill.  VEC = 4: one 16-byte load
//                         and one 16-byte store per lane and step (w % 4 == 0, x and out aligned to 16 bytes); VEC = 1: dwords.
//                         LW is the smallest power of two that covers a row (at most 64), so the lanes of a wave cover 64 / LW
//                         consecutive rows: `out` is written without a gap, `x` read the same way.  Values travel as bit patterns
//                         (NaN payloads and -0.0 come through).  No LDS, no atomics.
//   occlusion_map_kernel<STAGED>  one thread = one voxel, lanes along w; the covering windows of a coordinate are the contiguous
//                         index range occ_cover() gives in closed form (prologue arithmetic, no table in memory).  Per class the
//                         thread adds (double)base - (double)score over the range in ascending (a, b, c) order, divides by the count
//                         in fp64 and rounds once.  STAGED: the (Wn, k) score table is copied into LDS first (it fits whenever
//                         Wn * k <= OM_LDS_FLOATS: 343 x 3 at the defaults); otherwise the scores are read from global memory,
//                         where the lanes of a wave read the same or neighbouring windows.
//   channel_partial_kernel<VEC> / channel_final_kernel  the per-channel mean as a two-stage fp64 reduction in a fixed order: a channel
//                         is cut into groups of four consecutive elements, the groups into MMNN_CHANNEL_MEANS_PARTS contiguous parts;
//                         block (part, channel) gives thread t the groups t, t + 256, ... of the part, each added element by element
//                         in ascending order, then a butterfly over the wave, then the four waves in order.  The second stage adds the
//                         64 partials of a channel with the same butterfly, divides by n and rounds once.  The order depends on
//                         (n, the constants) only -- not on the alignment, which merely selects 16-byte (VEC = 4) or dword loads.
#include "../../include/mmnn_sts.h"
#include "common.hpp"
#include "reduce.hpp"

namespace mmnn {

constexpr int OC_TPB = 256;
constexpr int OM_TPB = 256;
constexpr int OM_LDS_FLOATS = 12288;        // 48 KiB of scores
constexpr int CM_TPB = 256;
constexpr int CM_PARTS = MMNN_CHANNEL_MEANS_PARTS;
static_assert(CM_PARTS == 64, "the second stage adds one partial per lane of a wave");

// windows along an axis of length L (window w, stride s; 1 <= s <= w <= L)
__host__ __device__ __forceinline__ int occ_count(int L, int w, int s) { return (L - w + s - 1) / s + 1; }
// first voxel of window i
__host__ __device__ __forceinline__ int occ_origin(int i, int L, int w, int s) { return i * s < L - w ? i * s : L - w; }
// the windows that cover voxel p: lo..hi (contiguous; the last window, clamped to the edge, covers p >= L - w)
__host__ __device__ __forceinline__ void occ_cover(int p, int L, int w, int s, int n, int& lo, int& hi) {
  const int first = p < w ? 0 : (p - w) / s + 1;
  lo = first < n - 1 ? first : n - 1;
  hi = p >= L - w ? n - 1 : p / s;
}

struct OcArgs {
  const unsigned* x;
  const unsigned* fill;
  unsigned* out;
  int samples_x_c;                          // count * c
  int c, d, h, w;                           // w in elements
  int win[3], stride[3], n[3];
  int first, wn;
  int lw_log2;                              // lanes per row = 1 << lw_log2
};

template <int VEC>
__global__ void __launch_bounds__(OC_TPB) occlude_windows_kernel(const OcArgs a) {
  const unsigned slot = blockIdx.x * OC_TPB + threadIdx.x;
  const unsigned zy = slot >> a.lw_log2;                                   // the row inside its (sample, channel) plane stack
  if (zy >= (unsigned)(a.d * a.h)) return;
  const int lane = (int)(slot & ((1u << a.lw_log2) - 1u));
  const int z = (int)(zy / (unsigned)a.h), y = (int)(zy - (unsigned)z * (unsigned)a.h);
  const int step = VEC << a.lw_log2;
  // blockIdx.y = sample * c + channel: uniform over the block, so the window's decode below is scalar work
  for (unsigned sc = blockIdx.y; sc < (unsigned)a.samples_x_c; sc += gridDim.y) {
    const int b = (int)(sc / (unsigned)a.c), ch = (int)(sc - (unsigned)b * (unsigned)a.c);
    int wi = a.first + b;
    if (wi > a.wn - 1) wi = a.wn - 1;
    const int ic = wi % a.n[2]; wi /= a.n[2];
    const int ib = wi % a.n[1];
    const int ia = wi / a.n[1];
    const int oz = occ_origin(ia, a.d, a.win[0], a.stride[0]);
    const int oy = occ_origin(ib, a.h, a.win[1], a.stride[1]);
    const int ox = occ_origin(ic, a.w, a.win[2], a.stride[2]);
    const bool meets = z >= oz && z < oz + a.win[0] && y >= oy && y < oy + a.win[1];
    const int lo = meets ? ox : 0, hi = meets ? ox + a.win[2] : 0;        // the occluded voxels of this row: [lo, hi)
    const unsigned f = a.fill[ch];
    const long src = ((long)ch * (a.d * a.h) + zy) * a.w;
    const long dst = ((long)sc * (a.d * a.h) + zy) * a.w;
    for (int i = lane * VEC; i < a.w; i += step) {
      if (VEC == 4) {
        uint4 v = *reinterpret_cast<const uint4*>(a.x + src + i);
        v.x = (i >= lo && i < hi) ? f : v.x;
        v.y = (i + 1 >= lo && i + 1 < hi) ? f : v.y;
        v.z = (i + 2 >= lo && i + 2 < hi) ? f : v.z;
        v.w = (i + 3 >= lo && i + 3 < hi) ? f : v.w;
        *reinterpret_cast<uint4*>(a.out + dst + i) = v;
      } else {
        const unsigned v = a.x[src + i];
        a.out[dst + i] = (i >= lo && i < hi) ? f : v;
      }
    }
  }
}

struct OmArgs {
  const float* base;
  const float* scores;
  float* out;
  int k, d, h, w;
  int win[3], stride[3], n[3];
  int wn;
};

template <bool STAGED>
__global__ void __launch_bounds__(OM_TPB) occlusion_map_kernel(const OmArgs a) {
  extern __shared__ float lds[];                                           // STAGED: wn * k floats (dynamic, so a small table costs no occupancy)
  if (STAGED) {
    for (int i = threadIdx.x; i < a.wn * a.k; i += OM_TPB) lds[i] = a.scores[i];
    __syncthreads();
  }
  const long vox = (long)a.d * a.h * a.w;
  const long v = (long)blockIdx.x * OM_TPB + threadIdx.x;
  if (v >= vox) return;
  const int x = (int)(v % a.w);
  const int y = (int)((v / a.w) % a.h);
  const int z = (int)(v / ((long)a.w * a.h));
  int a0, a1, b0, b1, c0, c1;
  occ_cover(z, a.d, a.win[0], a.stride[0], a.n[0], a0, a1);
  occ_cover(y, a.h, a.win[1], a.stride[1], a.n[1], b0, b1);
  occ_cover(x, a.w, a.win[2], a.stride[2], a.n[2], c0, c1);
  const double cnt = (double)((long)(a1 - a0 + 1) * (b1 - b0 + 1) * (c1 - c0 + 1));
  for (int kk = 0; kk < a.k; ++kk) {
    const double base = (double)a.base[kk];
    double acc = 0.0;
    for (int ia = a0; ia <= a1; ++ia)
      for (int ib = b0; ib <= b1; ++ib) {
        const long w0 = ((long)ia * a.n[1] + ib) * a.n[2];
        for (int ic = c0; ic <= c1; ++ic) {
          const long at = (w0 + ic) * a.k + kk;
          const float s = STAGED ? lds[at] : a.scores[at];
          acc += base - (double)s;
        }
      }
    a.out[(long)kk * vox + v] = (float)(acc / cnt);
  }
}

template <int VEC>
__global__ void __launch_bounds__(CM_TPB) channel_partial_kernel(const float* x, long n, double* partial) {
  __shared__ double lds[CM_TPB / 64];
  const float* xc = x + (long)blockIdx.y * n;
  const long groups = (n + 3) / 4, per = (groups + CM_PARTS - 1) / CM_PARTS;
  const long g0 = (long)blockIdx.x * per, g1 = g0 + per < groups ? g0 + per : groups;
  double acc = 0.0;
  for (long g = g0 + threadIdx.x; g < g1; g += CM_TPB) {
    const long i = g * 4;
    if (VEC == 4) {                          // n % 4 == 0: every group is whole
      const float4 v = *reinterpret_cast<const float4*>(xc + i);
      acc += (double)v.x; acc += (double)v.y; acc += (double)v.z; acc += (double)v.w;
    } else {
      const int m = n - i < 4 ? (int)(n - i) : 4;
      for (int j = 0; j < m; ++j) acc += (double)xc[i + j];
    }
  }
  const double t = block_reduce<CM_TPB / 64>(acc, lds, Sum{});     // the block's waves in index order
  if (threadIdx.x == 0) partial[(long)blockIdx.y * CM_PARTS + blockIdx.x] = t;
}

__global__ void __launch_bounds__(64) channel_final_kernel(const double* partial, long n, float* out) {
  const double t = wave_sum(partial[(long)blockIdx.x * CM_PARTS + threadIdx.x]);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(t / (double)n);
}

// the shared descriptor checks; `what` names the caller
static int occ_check_desc(const mmnn_occlusion_desc* d, const char* what, int n[3]) {
  MMNN_REQUIRE(d, "%s: null descriptor", what);
  MMNN_REQUIRE(d->c >= 1 && d->d >= 1 && d->h >= 1 && d->w >= 1, "%s: non-positive extent c %d, d %d, h %d, w %d", what, d->c, d->d, d->h, d->w);
  const int L[3] = {d->d, d->h, d->w};
  for (int r = 0; r < 3; ++r) {
    MMNN_REQUIRE(d->win[r] >= 1 && d->win[r] <= L[r], "%s: win[%d] = %d outside 1..%d (the extent)", what, r, d->win[r], L[r]);
    MMNN_REQUIRE(d->stride[r] >= 1 && d->stride[r] <= d->win[r], "%s: stride[%d] = %d outside 1..%d (win: a larger stride leaves holes)", what,
                 r, d->stride[r], d->win[r]);
    n[r] = occ_count(L[r], d->win[r], d->stride[r]);
  }
  MMNN_REQUIRE((double)d->c * d->d * d->h * d->w < 2147483648.0, "%s: extent %d x %d x %d x %d holds 2^31 elements or more", what, d->c, d->d,
               d->h, d->w);
  MMNN_REQUIRE((double)n[0] * n[1] * n[2] < 2147483648.0, "%s: 2^31 windows or more", what);
  return 0;
}

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_occlusion_window_count(const mmnn_occlusion_desc* d, int32_t n_out[3]) {
  int n[3];
  if (occ_check_desc(d, "occlusion_window_count", n)) return -1;
  if (n_out)
    for (int r = 0; r < 3; ++r) n_out[r] = n[r];
  return (int64_t)n[0] * n[1] * n[2];
}

int mmnn_occlude_windows(const mmnn_occlusion_desc* d, const float* x, const float* fill, int32_t first, int32_t count, float* out,
                         void* stream_) {
  int n[3];
  if (occ_check_desc(d, "occlude_windows", n)) return 1;
  const long wn = (long)n[0] * n[1] * n[2];
  MMNN_REQUIRE(x && fill && out, "occlude_windows: null argument");
  MMNN_REQUIRE(count >= 1, "occlude_windows: count = %d is below 1", count);
  MMNN_REQUIRE(first >= 0 && first < wn, "occlude_windows: first = %d outside 0..%ld (Wn - 1)", first, wn - 1);
  const size_t chw = (size_t)d->c * d->d * d->h * d->w;
  MMNN_REQUIRE((double)chw * count < 2147483648.0, "occlude_windows: count = %d samples of %d x %d x %d x %d hold 2^31 elements or more", count,
               d->c, d->d, d->h, d->w);
  MMNN_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)fill % 4 == 0 && (uintptr_t)out % 4 == 0, "occlude_windows: x / fill / out not aligned to 4 bytes");
  const uintptr_t x0 = (uintptr_t)x, x1 = x0 + 4 * chw, o0 = (uintptr_t)out, o1 = o0 + 4 * chw * (size_t)count;
  MMNN_REQUIRE(x1 <= o0 || o1 <= x0, "occlude_windows: x and out overlap");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  OcArgs a{};
  a.x = reinterpret_cast<const unsigned*>(x); a.fill = reinterpret_cast<const unsigned*>(fill); a.out = reinterpret_cast<unsigned*>(out);
  a.samples_x_c = count * d->c;
  a.c = d->c; a.d = d->d; a.h = d->h; a.w = d->w;
  for (int r = 0; r < 3; ++r) { a.win[r] = d->win[r]; a.stride[r] = d->stride[r]; a.n[r] = n[r]; }
  a.first = first; a.wn = (int)wn;
  const bool vec = d->w % 4 == 0 && x0 % 16 == 0 && o0 % 16 == 0;
  const int steps = vec ? d->w / 4 : d->w;                                 // lane steps that cover a row
  a.lw_log2 = 0;
  while (a.lw_log2 < 6 && (1 << a.lw_log2) < steps) ++a.lw_log2;
  const long slots = ((long)d->d * d->h) << a.lw_log2;                     // per (sample, channel); < 2^32: a row holds >= 1 element
  const dim3 grid((unsigned)cdiv(slots, OC_TPB), (unsigned)(a.samples_x_c < 65535 ? a.samples_x_c : 65535));
  if (vec) MMNN_LAUNCH(occlude_windows_kernel<4>, grid, dim3(OC_TPB), 0, stream, a);
  else MMNN_LAUNCH(occlude_windows_kernel<1>, grid, dim3(OC_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int mmnn_occlusion_map(const mmnn_occlusion_desc* d, int32_t k, const float* base, const float* scores, float* out, void* stream_) {
  int n[3];
  if (occ_check_desc(d, "occlusion_map", n)) return 1;
  const long wn = (long)n[0] * n[1] * n[2];
  MMNN_REQUIRE(k >= 1 && k <= MMNN_OCCLUSION_MAX_OUTPUTS, "occlusion_map: k = %d outside 1..%d", k, MMNN_OCCLUSION_MAX_OUTPUTS);
  MMNN_REQUIRE(base && scores && out, "occlusion_map: null argument");
  const size_t vox = (size_t)d->d * d->h * d->w;
  MMNN_REQUIRE((double)vox * k < 2147483648.0, "occlusion_map: k = %d maps of %d x %d x %d hold 2^31 elements or more", k, d->d, d->h, d->w);
  MMNN_REQUIRE((double)wn * k < 2147483648.0, "occlusion_map: %ld windows x k = %d scores are 2^31 or more", wn, k);
  MMNN_REQUIRE((uintptr_t)base % 4 == 0 && (uintptr_t)scores % 4 == 0 && (uintptr_t)out % 4 == 0, "occlusion_map: base / scores / out not aligned to 4 bytes");
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 4 * vox * (size_t)k, s0 = (uintptr_t)scores, s1 = s0 + 4 * (size_t)wn * k,
                  b0 = (uintptr_t)base, b1 = b0 + 4 * (size_t)k;
  MMNN_REQUIRE((s1 <= o0 || o1 <= s0) && (b1 <= o0 || o1 <= b0), "occlusion_map: out overlaps scores or base");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  OmArgs a{};
  a.base = base; a.scores = scores; a.out = out;
  a.k = k; a.d = d->d; a.h = d->h; a.w = d->w;
  for (int r = 0; r < 3; ++r) { a.win[r] = d->win[r]; a.stride[r] = d->stride[r]; a.n[r] = n[r]; }
  a.wn = (int)wn;
  const dim3 grid((unsigned)cdiv((long)vox, OM_TPB));
  if (wn * k <= OM_LDS_FLOATS) MMNN_LAUNCH(occlusion_map_kernel<true>, grid, dim3(OM_TPB), (size_t)(wn * k) * sizeof(float), stream, a);
  else MMNN_LAUNCH(occlusion_map_kernel<false>, grid, dim3(OM_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int mmnn_channel_means(const float* x, int32_t c, int64_t n, float* out, void* ws, void* stream_) {
  MMNN_REQUIRE(x && out && ws, "channel_means: null argument");
  MMNN_REQUIRE(c >= 1 && c <= 65535, "channel_means: c = %d outside 1..65535", c);
  MMNN_REQUIRE(n >= 1, "channel_means: non-positive extent n = %lld", (long long)n);
  MMNN_REQUIRE((double)c * (double)n < 9.0e15, "channel_means: c = %d channels of n = %lld elements are too many", c, (long long)n);
  MMNN_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)out % 4 == 0, "channel_means: x / out not aligned to 4 bytes");
  MMNN_REQUIRE((uintptr_t)ws % 8 == 0, "channel_means: workspace not aligned to 8 bytes");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  double* partial = static_cast<double*>(ws);
  const dim3 grid(CM_PARTS, (unsigned)c);
  if (n % 4 == 0 && (uintptr_t)x % 16 == 0) MMNN_LAUNCH(channel_partial_kernel<4>, grid, dim3(CM_TPB), 0, stream, x, (long)n, partial);
  else MMNN_LAUNCH(channel_partial_kernel<1>, grid, dim3(CM_TPB), 0, stream, x, (long)n, partial);
  MMNN_LAUNCH(channel_final_kernel, dim3((unsigned)c), dim3(64), 0, stream, (const double*)partial, (long)n, out);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
