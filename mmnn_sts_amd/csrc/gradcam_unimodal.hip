// Batched Grad-CAM of an image-only model (DenseNet family, r3d_18) on the last Conv3d of its encoder: the published Grad-CAM
// (Selvaraju et al.) that upstream obtains from medcam's `gcam` backend (utils/utils.py:451-455), with the rules pinned in
// INTEGRATION.md.  After the eval-mode forward, per sample b:
//   gcu_head_densenet_kernel /      s[b][c]: the gradient scale of the target t_b (sum / one / argmax of the outputs) through the head,
//   gcu_head_sigmoid_kernel         closed form, so that  d t_b / d A[b][c][v] = s[b][c] * mask[b][c][v] / V
//   gcu_count_kernel                per-block partial counts of the mask, per (b, c); the gradient itself when asked
//   gcu_heat_kernel                 alpha = s * count / V^2, heat = ReLU(sum_c alpha * A), per-block partial min / max
//   gcu_normalise_kernel            (heat - min) / (max - min) per sample; 0 where max == min
//   gradcam_upsample_kernel         (gradcam.hip) trilinear up-sampling, one map per sample
// Every kernel is a grid of (voxel chunks[, channel groups], samples); the cross-block reductions go through per-block partials in
// the workspace (no atomics, no initialisation, the same result whatever the arrival order).
#include "gradcam.hpp"

namespace mmnn {

constexpr int GCU_THREADS = 256;
constexpr int GCU_MAX_C = 64;        // channels of the captured layer (DenseNet growth <= 32, r3d_18 16)
constexpr int GCU_CHUNK = 1024;      // voxels of one sample per block
constexpr int GCU_MAX_CHUNKS = 4096;

struct GcuHeadArgs {
  int n, C, K, label, F, w_feat_ld, chan_off;
  const float* w_out; const float* w_feat; const float* gamma; const float* rvar; const float* outputs;
  float eps;
  float* s;                          // [n][C]
};

struct GcuArgs {
  int n, C, V, chunks;
  long act_ns, mask_ns;
  const float* act; const float* mask; const float* s;
  unsigned* part_cnt;                // [n][chunks][C]
  float* part_mm;                    // [n][chunks][2]: min, max
  float* grads;                      // [n][C][V] or null
  float* heat;                       // [n][V]
};

// target of sample b: -1 = every output (a ones mask), otherwise the output index; LABEL_BEST: the first maximum, as torch.argmax
__device__ __forceinline__ int gcu_target(const float* out_b, int K, int label) {
  if (label >= 0) return label;
  if (label == MMNN_GC_LABEL_SUM) return -1;
  int best = 0;
  float top = out_b[0];
  for (int k = 1; k < K; ++k)
    if (out_b[k] > top) { top = out_b[k]; best = k; }
  return best;
}

// s[b][c] = (sum_k l[b][k] sum_f Wcls[k][f] Wfeat[f][c']) * gamma5[c'] / sqrt(var5[c'] + eps),   c' = chan_off + c
__global__ void __launch_bounds__(GCU_MAX_C) gcu_head_densenet_kernel(const GcuHeadArgs a) {
  const int b = blockIdx.x, c = threadIdx.x;
  if (c >= a.C) return;
  const int cc = a.chan_off + c;
  const int t = gcu_target(a.outputs + (long)b * a.K, a.K, a.label);
  const int k0 = t < 0 ? 0 : t, k1 = t < 0 ? a.K : t + 1;
  float s = 0.f;
  for (int k = k0; k < k1; ++k) {
    float u = 0.f;
    for (int f = 0; f < a.F; ++f) u = fmaf(a.w_out[(long)k * a.F + f], a.w_feat[(long)f * a.w_feat_ld + cc], u);
    s += u;
  }
  a.s[(long)b * a.C + c] = s * (a.gamma[cc] / sqrtf(a.rvar[cc] + a.eps));
}

// s[b][c] = sum_k l[b][k] * y[b][k] (1 - y[b][k]) * Wfc[k][c] * gamma[c] / sqrt(var[c] + eps),   y = sigmoid(z) = the model's outputs
__global__ void __launch_bounds__(GCU_MAX_C) gcu_head_sigmoid_kernel(const GcuHeadArgs a) {
  const int b = blockIdx.x, c = threadIdx.x;
  if (c >= a.C) return;
  const int cc = a.chan_off + c;
  const float* y = a.outputs + (long)b * a.K;
  const int t = gcu_target(y, a.K, a.label);
  const int k0 = t < 0 ? 0 : t, k1 = t < 0 ? a.K : t + 1;
  float s = 0.f;
  for (int k = k0; k < k1; ++k) s = fmaf(y[k] * (1.f - y[k]), a.w_out[(long)k * a.C + c], s);
  a.s[(long)b * a.C + c] = s * (a.gamma[cc] / sqrtf(a.rvar[cc] + a.eps));
}

// one wave per channel (grid.y: groups of four channels), lanes along the chunk's voxels: coalesced 256-byte rows, four loads in flight
// per lane before the first is used (the chunk is a latency chain otherwise: one wave per 8 channels took 18 us)
__global__ void __launch_bounds__(GCU_THREADS) gcu_count_kernel(const GcuArgs a) {
  const int chunk = blockIdx.x, b = blockIdx.z;
  const int lane = threadIdx.x & 63, c = blockIdx.y * (GCU_THREADS / 64) + (threadIdx.x >> 6);
  if (c >= a.C) return;
  const int v0 = chunk * GCU_CHUNK, v1 = min(a.V, v0 + GCU_CHUNK);
  const float* m = a.mask + (long)b * a.mask_ns + (long)c * a.V;
  float* g = a.grads ? a.grads + ((long)b * a.C + c) * a.V : nullptr;
  const float gs = a.s[(long)b * a.C + c] / (float)a.V;
  unsigned n = 0;
  for (int v = v0 + lane; v < v1; v += 256) {
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = v + 64 * e < v1 ? m[v + 64 * e] : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool on = x[e] > 0.f;
      n += on ? 1u : 0u;
      if (g && v + 64 * e < v1) g[v + 64 * e] = on ? gs : 0.f;
    }
  }
  n = wave_sum(n);
  if (lane == 0) a.part_cnt[((long)b * a.chunks + chunk) * a.C + c] = n;
}

// thread per voxel: heat = ReLU(sum_c alpha[c] * A[c][v]) with alpha = s * count / V / V (the mean over the voxels of s * mask / V)
__global__ void __launch_bounds__(GCU_THREADS) gcu_heat_kernel(const GcuArgs a) {
  __shared__ float alpha[GCU_MAX_C];
  __shared__ float red[2 * GCU_THREADS / 64];
  const int chunk = blockIdx.x, b = blockIdx.y;
  const float fv = (float)a.V;
  for (int c = threadIdx.x; c < a.C; c += GCU_THREADS) {
    const unsigned* pc = a.part_cnt + (long)b * a.chunks * a.C + c;
    unsigned n = 0;
    for (int k = 0; k < a.chunks; ++k) n += pc[(long)k * a.C];
    alpha[c] = a.s[(long)b * a.C + c] * (float)n / fv / fv;
  }
  __syncthreads();
  const int v0 = chunk * GCU_CHUNK, v1 = min(a.V, v0 + GCU_CHUNK);
  const float* x = a.act + (long)b * a.act_ns;
  float* hb = a.heat + (long)b * a.V;
  float mm[2] = {3.4e38f, -3.4e38f};     // min, max
  for (int v = v0 + threadIdx.x; v < v1; v += GCU_THREADS) {
    float m = 0.f;
    for (int c = 0; c < a.C; ++c) m = fmaf(alpha[c], x[(long)c * a.V + v], m);
    m = m > 0.f ? m : 0.f;
    hb[v] = m;
    mm[0] = fminf(mm[0], m); mm[1] = fmaxf(mm[1], m);
  }
  block_reduce<GCU_THREADS / 64>(mm, red, FMinMax{});
  if (threadIdx.x == 0) {
    float* pm = a.part_mm + ((long)b * a.chunks + chunk) * 2;
    pm[0] = mm[0]; pm[1] = mm[1];
  }
}

__global__ void __launch_bounds__(GCU_THREADS) gcu_normalise_kernel(const GcuArgs a) {
  const int chunk = blockIdx.x, b = blockIdx.y;
  const float* pm = a.part_mm + (long)b * a.chunks * 2;
  float lo = pm[0], hi = pm[1];
  for (int k = 1; k < a.chunks; ++k) { lo = fminf(lo, pm[2 * k]); hi = fmaxf(hi, pm[2 * k + 1]); }
  const float range = hi - lo;
  const int v0 = chunk * GCU_CHUNK, v1 = min(a.V, v0 + GCU_CHUNK);
  float* hb = a.heat + (long)b * a.V;
  for (int v = v0 + threadIdx.x; v < v1; v += GCU_THREADS) hb[v] = range > 0.f ? (hb[v] - lo) / range : 0.f;
}

struct GcuLayout {
  long chunks, s_off, cnt_off, mm_off, bytes;
};

static GcuLayout gcu_layout(const mmnn_gradcam_unimodal_desc* d) {
  GcuLayout l;
  const long v = (long)d->d * d->h * d->w, n = d->n, c = d->channels;
  l.chunks = (v + GCU_CHUNK - 1) / GCU_CHUNK;
  Carver cv;
  l.s_off = (long)cv.take(4 * n * c);
  l.cnt_off = (long)cv.take(4 * n * l.chunks * c);
  l.mm_off = (long)cv.take(4 * n * l.chunks * 2);
  l.bytes = (long)cv.cur;
  return l;
}

}  // namespace mmnn

using namespace mmnn;

extern "C" int64_t mmnn_gradcam_unimodal_workspace_bytes(const mmnn_gradcam_unimodal_desc* d) {
  if (!d || d->n < 1 || d->channels < 1 || d->d < 1 || d->h < 1 || d->w < 1) return -1;
  return gcu_layout(d).bytes;
}

extern "C" int mmnn_gradcam_unimodal(const mmnn_gradcam_unimodal_desc* d, const mmnn_gradcam_head* head, const float* act,
                                     const float* mask_src, float* grads, float* heat, float* maps, void* ws, int64_t ws_bytes,
                                     void* stream) {
  MMNN_REQUIRE(d && head && act && mask_src && heat && maps && ws, "gradcam_unimodal: null argument");
  MMNN_REQUIRE(head->w_out && head->gamma && head->running_var && head->outputs, "gradcam_unimodal: null head tensor");
  MMNN_REQUIRE(head->kind == MMNN_GC_HEAD_DENSENET || head->kind == MMNN_GC_HEAD_SIGMOID, "gradcam_unimodal: unknown head kind %d", head->kind);
  MMNN_REQUIRE(d->n >= 1 && d->n <= 65535, "gradcam_unimodal: %d samples not in 1..65535", d->n);
  MMNN_REQUIRE(d->channels >= 1 && d->channels <= GCU_MAX_C, "gradcam_unimodal: captured layer width %d not in 1..%d", d->channels, GCU_MAX_C);
  MMNN_REQUIRE(d->d >= 1 && d->h >= 1 && d->w >= 1 && d->out_d >= 1 && d->out_h >= 1 && d->out_w >= 1, "gradcam_unimodal: bad extent");
  MMNN_REQUIRE(d->classes >= 1, "gradcam_unimodal: %d classes", d->classes);
  MMNN_REQUIRE(d->label == MMNN_GC_LABEL_SUM || d->label == MMNN_GC_LABEL_BEST || (d->label >= 0 && d->label < d->classes),
               "gradcam_unimodal: label %d is neither an output index below %d nor SUM / BEST", d->label, d->classes);
  const long v = (long)d->d * d->h * d->w;
  const GcuLayout l = gcu_layout(d);
  MMNN_REQUIRE(l.chunks <= GCU_MAX_CHUNKS, "gradcam_unimodal: captured layer of %ld voxels larger than %d", v, GCU_MAX_CHUNKS * GCU_CHUNK);
  MMNN_REQUIRE(d->act_ns >= (long)d->channels * v && d->mask_ns >= (long)d->channels * v, "gradcam_unimodal: sample stride below channels x voxels");
  MMNN_REQUIRE(ws_bytes >= l.bytes, "gradcam_unimodal: workspace of %lld bytes, %ld needed", (long long)ws_bytes, l.bytes);
  if (head->kind == MMNN_GC_HEAD_DENSENET) {
    MMNN_REQUIRE(head->w_feat && head->features >= 1, "gradcam_unimodal: DenseNet head without feature layer");
    MMNN_REQUIRE(head->chan_off >= 0 && head->chan_off + d->channels <= head->w_feat_ld,
                 "gradcam_unimodal: captured channels [%d, %d) outside the %d columns of the feature layer", head->chan_off,
                 head->chan_off + d->channels, head->w_feat_ld);
  } else {
    MMNN_REQUIRE(head->chan_off >= 0, "gradcam_unimodal: negative channel offset");
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(ws);
  float* s = reinterpret_cast<float*>(w + l.s_off);

  GcuHeadArgs h;
  h.n = d->n; h.C = d->channels; h.K = d->classes; h.label = d->label; h.F = head->features; h.w_feat_ld = head->w_feat_ld;
  h.chan_off = head->chan_off; h.w_out = head->w_out; h.w_feat = head->w_feat; h.gamma = head->gamma; h.rvar = head->running_var;
  h.outputs = head->outputs; h.eps = head->eps; h.s = s;
  if (head->kind == MMNN_GC_HEAD_DENSENET) {
    MMNN_LAUNCH(gcu_head_densenet_kernel, dim3(d->n), dim3(GCU_MAX_C), 0, st, h);
  } else {
    MMNN_LAUNCH(gcu_head_sigmoid_kernel, dim3(d->n), dim3(GCU_MAX_C), 0, st, h);
  }
  MMNN_HIP(hipGetLastError());

  GcuArgs a;
  a.n = d->n; a.C = d->channels; a.V = (int)v; a.chunks = (int)l.chunks; a.act_ns = d->act_ns; a.mask_ns = d->mask_ns;
  a.act = act; a.mask = mask_src; a.s = s;
  a.part_cnt = reinterpret_cast<unsigned*>(w + l.cnt_off); a.part_mm = reinterpret_cast<float*>(w + l.mm_off);
  a.grads = grads; a.heat = heat;
  const dim3 grid((unsigned)l.chunks, (unsigned)d->n);
  MMNN_LAUNCH(gcu_count_kernel, dim3((unsigned)l.chunks, (unsigned)((d->channels + 3) / 4), (unsigned)d->n), dim3(GCU_THREADS), 0, st, a);
  MMNN_HIP(hipGetLastError());
  MMNN_LAUNCH(gcu_heat_kernel, grid, dim3(GCU_THREADS), 0, st, a);
  MMNN_HIP(hipGetLastError());
  MMNN_LAUNCH(gcu_normalise_kernel, grid, dim3(GCU_THREADS), 0, st, a);
  MMNN_HIP(hipGetLastError());
  return launch_gradcam_upsample(d->d, d->h, d->w, d->out_d, d->out_h, d->out_w, d->n, heat, maps, st);
}
