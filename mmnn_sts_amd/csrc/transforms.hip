// Input transforms of the training / validation path (upstream main.py:64-92: train_transforms, val_transforms) on a batch of
// (C, D, H, W) fp32 volumes, memory-bound passes over whole volumes.  The semantics are the table of DESIGN §11.
//
// Passes, in order; a pass runs only when a stage it carries is present (and, for a random stage, fires for a sample of the group):
//   tf_minmax_kernel     per-sample min / max of the raw input (Normalize and ScaleIntensity are an affine map of the raw voxel
//                        given those two numbers; they are folded into the first pass that reads the input)
//   tf_rotate_kernel     RandRotate (bilinear in the (H, W) plane, border clamp) + RandAxisFlip (an index map), at the input extent
//   tf_area_kernel       RandZoom (area resize to floor(n z), then edge-pad / centre-crop back to n) and Resize (area resize)
//   tf_gauss_kernel      one axis of the separable Gaussian of RandGaussianSmooth / RandGaussianSharpen (zero padding); the last
//                        pass of a sharpen also forms b + alpha (b - G(b))
//   tf_intensity_kernel  RandShiftIntensity, RandAdjustContrast, RandHistogramShift, RandGaussianNoise (point-wise), and the
//                        affine / copy into `out` when no other pass wrote it
// The spatial and Gaussian passes write per-block partial (min, max) of their output beside it, so that a later pass which needs the
// min / max of its input (contrast, histogram shift) reduces at most 256 partials per sample instead of reading the volume again.
// Shift and contrast move the min / max analytically; the kernel tracks them in registers.
//
// Samples travel in groups of TF_G per launch: every per-sample parameter is a kernel argument (no host-to-device copy, no sync).
#include "../../include/mmnn_sts.h"
#include "area.hpp"
#include "common.hpp"
#include "reduce.hpp"

#include <math.h>

namespace mmnn {

constexpr int TF_G = 8;        // samples per launch group
constexpr int TF_TPB = 512;    // threads per block
constexpr int TF_MAXP = 256;   // partial (min, max) pairs per sample
constexpr int TF_NTAP = MMNN_TF_MAX_TAPS;
constexpr int TF_MAXR = (TF_NTAP - 1) / 2;

// Where a kernel finds the min / max of its input: the partials of the pass that wrote it.  With norm / scale set the partials
// describe the raw input and the kernel applies Normalize / ScaleIntensity itself.
struct TfMM {
  const float2* part;   // [TF_G][TF_MAXP]; null: this pass needs neither min / max nor an affine
  int p;                // partials per sample
  int norm, scale;
  float mean, std;
};

struct TfRotArgs {
  const float* src; float* dst; float2* part_out;
  long sstride, dstride;               // floats per sample
  int C, D, H, W, p_out;
  TfMM mm;
  int rot[TF_G], flip[TF_G];           // flip: -1 none, else axis 0 / 1 / 2 = D / H / W
  double cs[TF_G], sn[TF_G];
};

struct TfAreaArgs {
  const float* src; float* dst; float2* part_out;
  long sstride, dstride;
  int C, D, H, W;                      // source extent
  int OD, OH, OW;                      // destination extent
  int p_out;
  TfMM mm;
  int m[TF_G][3], off[TF_G][3];        // intermediate extent and offset per axis: o -> j = clamp(o + off, 0, m - 1) -> window of j
};

struct TfGaussArgs {
  const float* src; float* dst; const float* comb; float2* part_out;   // comb != null: dst = comb + alpha (comb - G(src))
  long stride;
  int C, D, H, W, p_out, axis;
  int rad[TF_G];
  float alpha[TF_G];
  float tap[TF_G][TF_NTAP];
};

struct TfIntArgs {
  const float* src; float* dst;
  long stride;
  int count;                           // C * V
  TfMM mm;
  int flags[TF_G];                     // MMNN_TF_SHIFT / CONTRAST / HIST / NOISE bits
  float shift[TF_G], gamma[TF_G], noise_std[TF_G];
  float fl[TF_G][10];
  uint64_t seed[TF_G];
  int n0;                              // batch index of the group's first sample (noise stream)
};

struct TfMinmaxArgs {
  const float* src; float2* part_out;
  long stride;
  int count, p_out;
};

// ---- block helpers -----------------------------------------------------------------------------------------------------------
// All threads call; every thread returns the block's (min, max).  The LDS of the reduction (TF_MM_LDS floats) is the caller's.
constexpr int TF_MM_LDS = 2 * (TF_TPB / 64);
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* red) {
  float v[2] = {lo, hi};
  block_reduce<TF_TPB / 64>(v, red, FMinMax{});
  lo = v[0]; hi = v[1];
}

__device__ __forceinline__ void store_partial(float2* part_out, int s, float lo, float hi, float* red) {
  block_minmax(lo, hi, red);
  if (part_out && threadIdx.x == 0) part_out[s * TF_MAXP + blockIdx.x] = make_float2(lo, hi);
}

// (min, max) of sample s's input; then, with a pending Normalize / ScaleIntensity, the affine y = A x + B they form and the
// (min, max) of y.  Normalize: (x - mean M) / (std M), M = max(x) (its sign is kept); ScaleIntensity: (y - min) / (max - min), zeros
// when max == min.
__device__ void load_mm(const TfMM& mm, int s, float& lo, float& hi, float& A, float& B, float* red) {
  A = 1.f; B = 0.f; lo = 0.f; hi = 0.f;
  if (!mm.part) return;
  float l = INFINITY, h = -INFINITY;
  if ((int)threadIdx.x < mm.p) { const float2 v = mm.part[s * TF_MAXP + threadIdx.x]; l = v.x; h = v.y; }
  block_minmax(l, h, red);
  lo = l; hi = h;
  if (!mm.norm && !mm.scale) return;
  double a = 1.0, b = 0.0, ylo = l, yhi = h;
  if (mm.norm) {
    const double M = h;
    a = 1.0 / ((double)mm.std * M);
    b = -(double)mm.mean * M * a;
    ylo = a * l + b; yhi = a * h + b;
    if (a < 0.0) { const double t = ylo; ylo = yhi; yhi = t; }
  }
  if (mm.scale) {
    const double r = yhi - ylo;
    if (r == 0.0) { a = 0.0; b = 0.0; ylo = 0.0; yhi = 0.0; }
    else { a = a / r; b = (b - ylo) / r; ylo = 0.0; yhi = 1.0; }
  }
  A = (float)a; B = (float)b; lo = (float)ylo; hi = (float)yhi;
}

// ---- passes ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TF_TPB) tf_minmax_kernel(const TfMinmaxArgs a) {
  __shared__ float red[TF_MM_LDS];
  const int s = blockIdx.y;
  const float* src = a.src + s * a.stride;
  float lo = INFINITY, hi = -INFINITY;
  const int step = gridDim.x * TF_TPB;
  if ((a.count & 3) == 0 && (a.stride & 3) == 0) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (int i = blockIdx.x * TF_TPB + threadIdx.x; i < a.count / 4; i += step) {
      const float4 v = s4[i];
      lo = fminf(lo, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
      hi = fmaxf(hi, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
  } else {
    for (int i = blockIdx.x * TF_TPB + threadIdx.x; i < a.count; i += step) { lo = fminf(lo, src[i]); hi = fmaxf(hi, src[i]); }
  }
  store_partial(a.part_out, s, lo, hi, red);
}

__global__ void __launch_bounds__(TF_TPB) tf_rotate_kernel(const TfRotArgs a) {
  __shared__ float red[TF_MM_LDS];
  const int s = blockIdx.y;
  float lo, hi, A, B;
  load_mm(a.mm, s, lo, hi, A, B, red);
  const float* src = a.src + s * a.sstride;
  float* dst = a.dst + s * a.dstride;
  const int HW = a.H * a.W, V = a.D * HW, count = a.C * V;
  const int rot = a.rot[s], fl = a.flip[s];
  const double cs = a.cs[s], sn = a.sn[s], ch = 0.5 * (a.H - 1), cw = 0.5 * (a.W - 1);
  float olo = INFINITY, ohi = -INFINITY;
  for (int e = blockIdx.x * TF_TPB + threadIdx.x; e < count; e += gridDim.x * TF_TPB) {
    const int c = e / V, v = e - c * V;
    int d = v / HW;
    const int r = v - d * HW;
    int h = r / a.W, w = r - h * a.W;
    // out = Flip(Rotate(x)): output voxel p reads Rotate(x) at Flip(p)
    if (fl == 0) d = a.D - 1 - d;
    else if (fl == 1) h = a.H - 1 - h;
    else if (fl == 2) w = a.W - 1 - w;
    const float* sc = src + (long)c * V + (long)d * HW;
    float val;
    if (rot) {
      const double dh = h - ch, dw = w - cw;
      double sh = cs * dh - sn * dw + ch, sw = sn * dh + cs * dw + cw;
      sh = fmin(fmax(sh, 0.0), (double)(a.H - 1));
      sw = fmin(fmax(sw, 0.0), (double)(a.W - 1));
      const int h0 = (int)sh, w0 = (int)sw;
      const int h1 = min(h0 + 1, a.H - 1), w1 = min(w0 + 1, a.W - 1);
      const float th = (float)(sh - h0), tw = (float)(sw - w0);
      const float v00 = sc[h0 * a.W + w0], v01 = sc[h0 * a.W + w1], v10 = sc[h1 * a.W + w0], v11 = sc[h1 * a.W + w1];
      const float top = v00 + tw * (v01 - v00), bot = v10 + tw * (v11 - v10);
      val = top + th * (bot - top);
    } else {
      val = sc[h * a.W + w];
    }
    val = fmaf(A, val, B);
    dst[e] = val;
    olo = fminf(olo, val); ohi = fmaxf(ohi, val);
  }
  store_partial(a.part_out, s, olo, ohi, red);
}

// (the window rule of the area resize, `area_window`, is csrc/area.hpp: the scan ingest uses the same one)

__global__ void __launch_bounds__(TF_TPB) tf_area_kernel(const TfAreaArgs a) {
  __shared__ float red[TF_MM_LDS];
  const int s = blockIdx.y;
  float lo, hi, A, B;
  load_mm(a.mm, s, lo, hi, A, B, red);
  const float* src = a.src + s * a.sstride;
  float* dst = a.dst + s * a.dstride;
  const int HW = a.H * a.W, V = a.D * HW;
  const int OHW = a.OH * a.OW, OV = a.OD * OHW, count = a.C * OV;
  const int md = a.m[s][0], mh = a.m[s][1], mw = a.m[s][2];
  const int fd = a.off[s][0], fh = a.off[s][1], fw = a.off[s][2];
  float olo = INFINITY, ohi = -INFINITY;
  for (int e = blockIdx.x * TF_TPB + threadIdx.x; e < count; e += gridDim.x * TF_TPB) {
    const int c = e / OV, v = e - c * OV;
    const int od = v / OHW, r = v - od * OHW;
    const int oh = r / a.OW, ow = r - oh * a.OW;
    int d0, d1, h0, h1, w0, w1;
    area_window(od, a.D, md, fd, d0, d1);
    area_window(oh, a.H, mh, fh, h0, h1);
    area_window(ow, a.W, mw, fw, w0, w1);
    const float* sc = src + (long)c * V;
    float sum = 0.f;
    for (int d = d0; d < d1; ++d)
      for (int h = h0; h < h1; ++h) {
        const float* row = sc + (long)d * HW + h * a.W;
        for (int w = w0; w < w1; ++w) sum += row[w];
      }
    const float val = fmaf(A, sum / (float)((d1 - d0) * (h1 - h0) * (w1 - w0)), B);
    dst[e] = val;
    olo = fminf(olo, val); ohi = fmaxf(ohi, val);
  }
  store_partial(a.part_out, s, olo, ohi, red);
}

__global__ void __launch_bounds__(TF_TPB) tf_gauss_kernel(const TfGaussArgs a) {
  __shared__ float red[TF_MM_LDS];
  const int s = blockIdx.y;
  const float* src = a.src + s * a.stride;
  float* dst = a.dst + s * a.stride;
  const float* comb = a.comb ? a.comb + s * a.stride : nullptr;
  const int HW = a.H * a.W, V = a.D * HW, count = a.C * V;
  const int rad = a.rad[s];
  const float alpha = a.alpha[s];
  float k[TF_NTAP];   // the sample's taps in registers: the inner loop below is unrolled over all TF_NTAP slots
#pragma unroll
  for (int j = 0; j < TF_NTAP; ++j) k[j] = a.tap[s][j];
  const int n = a.axis == 0 ? a.D : (a.axis == 1 ? a.H : a.W);
  const int st = a.axis == 0 ? HW : (a.axis == 1 ? a.W : 1);
  float olo = INFINITY, ohi = -INFINITY;
  for (int e = blockIdx.x * TF_TPB + threadIdx.x; e < count; e += gridDim.x * TF_TPB) {
    const int v = e % V;
    const int i = a.axis == 0 ? v / HW : (a.axis == 1 ? (v / a.W) % a.H : v % a.W);
    const int jlo = max(-rad, -i), jhi = min(rad, n - 1 - i);   // zero padding: taps outside the volume contribute nothing
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < TF_NTAP; ++t) {
      const int j = t - rad;
      if (j >= jlo && j <= jhi) acc = fmaf(k[t], src[e + j * st], acc);
    }
    if (comb) { const float b = comb[e]; acc = b + alpha * (b - acc); }
    dst[e] = acc;
    olo = fminf(olo, acc); ohi = fmaxf(ohi, acc);
  }
  if (a.part_out) store_partial(a.part_out, s, olo, ohi, red);
}

// counter-based standard normal for (seed, sample, element): splitmix64, then Box-Muller on two 24-bit uniforms
__device__ __forceinline__ float tf_normal(uint64_t seed, int n, int e) {
  uint64_t x = seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(n + 1));
  x += 0xD1B54A32D192ED03ull * (uint64_t)(uint32_t)e;
  x = mix64(x);
  const float u1 = (float)((x >> 40) + 1) * (1.0f / 16777216.0f);          // (0, 1]
  const float u2 = unit24(x << 32);                                         // [0, 1): bits 8..31
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

__global__ void __launch_bounds__(TF_TPB) tf_intensity_kernel(const TfIntArgs a) {
  __shared__ float red[TF_MM_LDS];
  const int s = blockIdx.y;
  float lo, hi, A, B;
  load_mm(a.mm, s, lo, hi, A, B, red);
  const float* src = a.src + s * a.stride;
  float* dst = a.dst + s * a.stride;
  const int f = a.flags[s];
  const float o = a.shift[s], g = a.gamma[s], sd = a.noise_std[s];
  // min / max after the shift and the contrast (both monotone: the extremes map to the extremes, computed as the voxels are)
  float clo = lo, chi = hi;
  if (f & MMNN_TF_SHIFT) { clo = lo + o; chi = hi + o; }
  const float crange = chi - clo, cden = crange + 1e-7f;
  float hlo = clo, hhi = chi;
  if (f & MMNN_TF_CONTRAST) hhi = powf(fmaxf((chi - clo) / cden, 0.f), g) * crange + clo;
  const float hrange = hhi - hlo;
  const bool hist = (f & MMNN_TF_HIST) && hrange != 0.f;
  float fl[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) fl[k] = a.fl[s][k];
  const uint64_t seed = a.seed[s];
  const int gn = a.n0 + s;
  for (int e = blockIdx.x * TF_TPB + threadIdx.x; e < a.count; e += gridDim.x * TF_TPB) {
    float x = fmaf(A, src[e], B);
    if (f & MMNN_TF_SHIFT) x = x + o;
    if (f & MMNN_TF_CONTRAST) x = powf(fmaxf((x - clo) / cden, 0.f), g) * crange + clo;
    if (hist) {   // np.interp(x, linspace(0,1,10) * range + min, fl * range + min): clamped at both ends
      const float u = fminf(fmaxf((x - hlo) / hrange * 9.f, 0.f), 9.f);
      const int k = min((int)u, 8);
      float f0 = fl[0], f1 = fl[1];
#pragma unroll
      for (int q = 1; q < 9; ++q) if (k == q) { f0 = fl[q]; f1 = fl[q + 1]; }
      x = hlo + hrange * (f0 + (u - (float)k) * (f1 - f0));
    }
    if (f & MMNN_TF_NOISE) x += sd * tf_normal(seed, gn, e);
    dst[e] = x;
  }
}

// ---- host orchestration ------------------------------------------------------------------------------------------------------
namespace {

struct WsLayout {
  size_t part_r, part_s, sp0, sp1, g0, g1, g2, total;
};

WsLayout ws_layout(const mmnn_transform_desc& d) {
  const int g = d.n < TF_G ? d.n : TF_G;
  const size_t vin = (size_t)g * d.c * d.d * d.h * d.w * sizeof(float);
  const size_t vout = (size_t)g * d.c * d.out_d * d.out_h * d.out_w * sizeof(float);
  const size_t part = (size_t)TF_G * TF_MAXP * sizeof(float2);
  const bool spatial = d.stages & (MMNN_TF_ROTATE | MMNN_TF_FLIP | MMNN_TF_ZOOM);
  const int ng = (d.stages & MMNN_TF_SHARPEN) ? 3 : ((d.stages & MMNN_TF_SMOOTH) ? 2 : 0);
  WsLayout L;
  Carver cv;
  L.part_r = cv.take(part);
  L.part_s = cv.take(part);
  L.sp0 = cv.take(spatial ? vin : 0);
  L.sp1 = cv.take(spatial ? vin : 0);
  L.g0 = cv.take(ng >= 1 ? vout : 0);
  L.g1 = cv.take(ng >= 2 ? vout : 0);
  L.g2 = cv.take(ng >= 3 ? vout : 0);
  L.total = cv.cur;
  return L;
}

int validate(const mmnn_transform_desc* d) {
  MMNN_REQUIRE(d, "transform: null descriptor");
  MMNN_REQUIRE(d->n >= 1 && d->c >= 1 && d->d >= 1 && d->h >= 1 && d->w >= 1, "transform: bad batch / extent %d x %d x %d x %d x %d",
               d->n, d->c, d->d, d->h, d->w);
  MMNN_REQUIRE(d->out_d >= 1 && d->out_h >= 1 && d->out_w >= 1, "transform: bad output extent");
  MMNN_REQUIRE((d->stages & ~0xFFF) == 0, "transform: unknown stage bits 0x%x", d->stages);
  MMNN_REQUIRE((d->stages & MMNN_TF_RESIZE) || (d->out_d == d->d && d->out_h == d->h && d->out_w == d->w),
               "transform: the output extent differs from the input extent without a Resize stage");
  MMNN_REQUIRE((long)d->c * d->d * d->h * d->w < (1l << 31) && (long)d->c * d->out_d * d->out_h * d->out_w < (1l << 31),
               "transform: a sample has 2^31 or more voxels");
  MMNN_REQUIRE(!(d->stages & MMNN_TF_NORMALIZE) || d->norm_std != 0.f, "transform: Normalize with std 0");
  return 0;
}

int partials_for(int count, int ng) {
  int p = cdiv(count, TF_TPB * 4);
  const int cap = 2048 / ng;
  if (p > cap) p = cap;
  if (p > TF_MAXP) p = TF_MAXP;
  return p < 1 ? 1 : p;
}

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_transform_workspace_bytes(const mmnn_transform_desc* d) {
  if (validate(d) != 0) return -1;
  return (int64_t)ws_layout(*d).total;
}

int mmnn_transform_volumes(const mmnn_transform_desc* d, const mmnn_transform_params* ps, const float* in, float* out, void* ws,
                           int64_t ws_bytes, void* stream_) {
  if (validate(d) != 0) return 1;
  MMNN_REQUIRE(ps && in && out && ws, "transform: null argument");
  const WsLayout L = ws_layout(*d);
  MMNN_REQUIRE(ws_bytes >= (int64_t)L.total, "transform: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)L.total);
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int st = d->stages, C = d->c;
  const int vin = d->d * d->h * d->w, vout = d->out_d * d->out_h * d->out_w;
  // per-sample checks of what the kernels index with
  for (int i = 0; i < d->n; ++i) {
    const mmnn_transform_params& p = ps[i];
    MMNN_REQUIRE((p.fire & ~st) == 0, "transform: sample %d fires stages 0x%x outside the pipeline 0x%x", i, p.fire, st);
    MMNN_REQUIRE(!(p.fire & MMNN_TF_FLIP) || (p.flip_axis >= 0 && p.flip_axis < 3), "transform: sample %d flip axis %d", i, p.flip_axis);
    const int ext[3] = {d->d, d->h, d->w};
    for (int k = 0; k < 3; ++k) {
      MMNN_REQUIRE(!(p.fire & MMNN_TF_ZOOM) || (p.zoom_m[k] >= 1 && p.zoom_m[k] <= 4 * ext[k]), "transform: sample %d zoom extent %d", i, p.zoom_m[k]);
      MMNN_REQUIRE(!(p.fire & MMNN_TF_SMOOTH) || (p.smooth_r[k] >= 0 && p.smooth_r[k] <= TF_MAXR), "transform: sample %d smooth radius", i);
      MMNN_REQUIRE(!(p.fire & MMNN_TF_SHARPEN) || (p.sharp1_r[k] >= 0 && p.sharp1_r[k] <= TF_MAXR && p.sharp2_r[k] >= 0 && p.sharp2_r[k] <= TF_MAXR),
                   "transform: sample %d sharpen radius", i);
    }
  }
  char* wsb = static_cast<char*>(ws);
  float2* part_r = reinterpret_cast<float2*>(wsb + L.part_r);
  float2* part_s = reinterpret_cast<float2*>(wsb + L.part_s);
  float* spb[2] = {reinterpret_cast<float*>(wsb + L.sp0), reinterpret_cast<float*>(wsb + L.sp1)};
  float* gb[3] = {reinterpret_cast<float*>(wsb + L.g0), reinterpret_cast<float*>(wsb + L.g1), reinterpret_cast<float*>(wsb + L.g2)};
  const long sin_ = (long)C * vin, sout = (long)C * vout;

  for (int g0 = 0; g0 < d->n; g0 += TF_G) {
    const int ng = d->n - g0 < TF_G ? d->n - g0 : TF_G;
    const mmnn_transform_params* P = ps + g0;
    int any = 0;
    for (int s = 0; s < ng; ++s) any |= P[s].fire;
    float* gout = out + g0 * sout;
    // state: current tensor, its extent, a pending affine, and where its (min, max) partials are
    const float* cur = in + g0 * sin_;
    long cur_stride = sin_;
    int ed = d->d, eh = d->h, ew = d->w;
    TfMM pend{};     // the pending Normalize / ScaleIntensity (part = raw partials) or nothing
    pend.mean = d->norm_mean; pend.std = d->norm_std;
    TfMM mm{};       // min / max of `cur` (with `pend` applied by the consumer when pend is active)
    bool have_pend = false;
    auto minmax = [&](const float* src, long stride, int count) -> int {
      TfMinmaxArgs a{src, part_r, stride, count, partials_for(count, ng)};
      MMNN_LAUNCH(tf_minmax_kernel, dim3(a.p_out, ng), dim3(TF_TPB), 0, stream, a);
      mm = TfMM{part_r, a.p_out, 0, 0, d->norm_mean, d->norm_std};
      return 0;
    };
    if (st & (MMNN_TF_NORMALIZE | MMNN_TF_SCALE)) {
      minmax(cur, cur_stride, C * vin);
      pend = mm;
      pend.norm = (st & MMNN_TF_NORMALIZE) != 0;
      pend.scale = (st & MMNN_TF_SCALE) != 0;
      mm = pend;
      have_pend = true;
    }
    // ---- spatial passes at the input extent, then Resize ----
    const bool do_rot = any & (MMNN_TF_ROTATE | MMNN_TF_FLIP);
    const bool do_zoom = any & MMNN_TF_ZOOM;
    const bool do_resize = (st & MMNN_TF_RESIZE) && (d->out_d != d->d || d->out_h != d->h || d->out_w != d->w);
    int sp = 0;
    if (do_rot) {
      float* dst = (!do_zoom && !do_resize) ? gout : spb[sp++];
      TfRotArgs a{};
      a.src = cur; a.dst = dst; a.part_out = part_s; a.sstride = cur_stride; a.dstride = sin_;
      a.C = C; a.D = ed; a.H = eh; a.W = ew; a.p_out = partials_for(C * vin, ng);
      a.mm = have_pend ? pend : TfMM{};
      for (int s = 0; s < TF_G; ++s) {
        const bool on = s < ng && (P[s].fire & MMNN_TF_ROTATE);
        a.rot[s] = on;
        a.cs[s] = on ? cos(P[s].theta) : 1.0;
        a.sn[s] = on ? sin(P[s].theta) : 0.0;
        a.flip[s] = (s < ng && (P[s].fire & MMNN_TF_FLIP)) ? P[s].flip_axis : -1;
      }
      MMNN_LAUNCH(tf_rotate_kernel, dim3(a.p_out, ng), dim3(TF_TPB), 0, stream, a);
      cur = dst; cur_stride = sin_; have_pend = false;
      mm = TfMM{part_s, a.p_out, 0, 0, 0.f, 0.f};
    }
    auto area = [&](float* dst, long dstride, int od, int oh, int ow, bool zoom) {
      TfAreaArgs a{};
      a.src = cur; a.dst = dst; a.part_out = part_s; a.sstride = cur_stride; a.dstride = dstride;
      a.C = C; a.D = ed; a.H = eh; a.W = ew; a.OD = od; a.OH = oh; a.OW = ow;
      a.p_out = partials_for(C * od * oh * ow, ng);
      a.mm = have_pend ? pend : TfMM{};
      const int o3[3] = {od, oh, ow};
      for (int s = 0; s < TF_G; ++s)
        for (int k = 0; k < 3; ++k) {
          const bool z = zoom && s < ng && (P[s].fire & MMNN_TF_ZOOM);
          a.m[s][k] = z ? P[s].zoom_m[k] : o3[k];
          a.off[s][k] = z ? P[s].zoom_off[k] : 0;
        }
      MMNN_LAUNCH(tf_area_kernel, dim3(a.p_out, ng), dim3(TF_TPB), 0, stream, a);
      cur = dst; cur_stride = dstride; have_pend = false; ed = od; eh = oh; ew = ow;
      mm = TfMM{part_s, a.p_out, 0, 0, 0.f, 0.f};
    };
    if (do_zoom) area(do_resize ? spb[sp] : gout, sin_, d->d, d->h, d->w, true);
    if (do_resize) area(gout, sout, d->out_d, d->out_h, d->out_w, false);
    MMNN_HIP(hipGetLastError());
    // ---- intensity and Gaussian passes at the output extent ----
    const int pre = MMNN_TF_SHIFT | MMNN_TF_CONTRAST, post = MMNN_TF_HIST | MMNN_TF_NOISE;
    const bool do_smooth = any & MMNN_TF_SMOOTH, do_sharp = any & MMNN_TF_SHARPEN, gauss = do_smooth || do_sharp;
    auto intensity = [&](int mask) -> int {
      TfIntArgs a{};
      a.src = cur; a.dst = gout; a.stride = sout; a.count = C * vout;
      int need_mm = have_pend;
      for (int s = 0; s < ng; ++s) need_mm |= (P[s].fire & mask & (MMNN_TF_CONTRAST | MMNN_TF_HIST)) != 0;
      if (need_mm && !have_pend && !mm.part) minmax(cur, cur_stride, C * vout);
      a.mm = have_pend ? pend : (need_mm ? mm : TfMM{});
      for (int s = 0; s < ng; ++s) {
        a.flags[s] = P[s].fire & mask;
        a.shift[s] = P[s].shift; a.gamma[s] = P[s].gamma; a.noise_std[s] = P[s].noise_std;
        for (int k = 0; k < 10; ++k) a.fl[s][k] = P[s].hist_fl[k];
        a.seed[s] = P[s].noise_seed;
      }
      a.n0 = g0;
      MMNN_LAUNCH(tf_intensity_kernel, dim3(partials_for(a.count, ng), ng), dim3(TF_TPB), 0, stream, a);
      cur = gout; cur_stride = sout; have_pend = false;
      mm = TfMM{};   // the shift / contrast moved the extremes; nothing downstream of this pass reads them without a new reduction
      return 0;
    };
    if (gauss) {
      if ((any & pre) || have_pend) intensity(pre);
      auto pass = [&](const float* src, float* dst, const float* comb, int axis, int which, bool last) {
        TfGaussArgs a{};
        a.src = src; a.dst = dst; a.comb = comb; a.part_out = last ? part_s : nullptr; a.stride = sout;
        a.C = C; a.D = d->out_d; a.H = d->out_h; a.W = d->out_w; a.p_out = partials_for(C * vout, ng); a.axis = axis;
        for (int s = 0; s < TF_G; ++s) {
          const int bit = which == 0 ? MMNN_TF_SMOOTH : MMNN_TF_SHARPEN;
          const bool on = s < ng && (P[s].fire & bit);
          const int r = !on ? 0 : (which == 0 ? P[s].smooth_r[axis] : (which == 1 ? P[s].sharp1_r[axis] : P[s].sharp2_r[axis]));
          const float* k = !on ? nullptr : (which == 0 ? P[s].smooth_k[axis] : (which == 1 ? P[s].sharp1_k[axis] : P[s].sharp2_k[axis]));
          a.rad[s] = r;
          a.alpha[s] = on ? P[s].alpha : 0.f;
          for (int j = 0; j < TF_NTAP; ++j) a.tap[s][j] = on ? k[j] : (j == 0 ? 1.f : 0.f);
        }
        MMNN_LAUNCH(tf_gauss_kernel, dim3(a.p_out, ng), dim3(TF_TPB), 0, stream, a);
        if (last) mm = TfMM{part_s, a.p_out, 0, 0, 0.f, 0.f};
      };
      const float* src = cur;   // gout, or the input itself when nothing before wrote (no pending affine)
      if (do_smooth) {
        pass(src, gb[0], nullptr, 0, 0, false);
        pass(gb[0], gb[1], nullptr, 1, 0, false);
        pass(gb[1], gout, nullptr, 2, 0, !do_sharp);
        src = gout;
      }
      if (do_sharp) {
        pass(src, gb[0], nullptr, 0, 1, false);
        pass(gb[0], gb[1], nullptr, 1, 1, false);
        pass(gb[1], gb[2], nullptr, 2, 1, false);
        pass(gb[2], gb[0], nullptr, 0, 2, false);
        pass(gb[0], gb[1], nullptr, 1, 2, false);
        pass(gb[1], gout, gb[2], 2, 2, true);
      }
      cur = gout; cur_stride = sout;
      if (any & post) intensity(post);
    } else if (any & (pre | post)) {
      intensity(pre | post);
    }
    if (cur != gout || have_pend) intensity(0);   // copy (or the folded Normalize / ScaleIntensity) into `out`
    MMNN_HIP(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
