// Learning-rate range test (upstream utils/find_lr.py -> torch-lr-finder's LRFinder.range_test) on the device:
//   * softmax cross entropy (nn.CrossEntropyLoss: index targets with ignore_index, or probability targets) and its adjoint;
//   * the sweep's bookkeeping (loss accumulation, exponential smoothing, best loss, divergence stop) in a small device struct;
//   * the SGD update with its learning rate read from a device table and switched off by the struct's `live` flag
//     (elementwise.hip: the same per-element code as mmnn_sgd_step / mmnn_sgd_step_multi).
// Nothing here waits on the host: a whole sweep is enqueued up front and its history read back once.
#include "../../include/mmnn_sts.h"
#include "common.hpp"
#include "elementwise.hpp"
#include "reduce.hpp"

namespace mmnn {

// =====================================================================================================================
// cross entropy.  One block of 4 wavefronts; wave w owns rows w, w + 4, ...; a row's classes are spread over the 64 lanes.
// Row arithmetic is fp64 (exp / log of the max-shifted logits), rounded to fp32 once per output.  The reduction over rows is
// a fixed order (each wave sums its rows in row order, then the 4 wave sums in wave order): two calls are bit-identical.
// =====================================================================================================================
constexpr int CE_THREADS = 256;
constexpr int CE_WAVES = CE_THREADS / 64;

struct CeRow {
  double lse;      // log-sum-exp of the row
  double mass;     // sum_k y_k (index targets: 1)
  double loss;     // row loss (NaN for an out-of-range index)
  int kept;        // 0: ignored row (index == ignore_index)
  long y;          // index target (kind 0)
};

// every lane returns the same CeRow
__device__ CeRow ce_row(const float* z, const void* target, int kind, long ignore_index, int c, long r, int lane) {
  CeRow o;
  float m = -INFINITY;
  for (int k = lane; k < c; k += 64) m = fmaxf(m, z[k]);   // fmaxf drops NaN; a NaN logit still poisons the sum below
  m = wave_reduce(m, FMax{});
  const double md = (double)m;
  double s = 0.0;
  for (int k = lane; k < c; k += 64) s += exp((double)z[k] - md);
  s = wave_sum(s);
  o.lse = md + log(s);
  if (kind == 0) {
    const long y = static_cast<const long long*>(target)[r];
    o.y = y;
    o.mass = 1.0;
    o.kept = y != ignore_index;
    if (!o.kept) o.loss = 0.0;
    else if (y < 0 || y >= c) o.loss = __longlong_as_double(0x7ff8000000000000ll);   // out-of-range class: NaN, never an address
    else o.loss = o.lse - (double)z[y];
  } else {
    const float* yr = static_cast<const float*>(target) + r * (long)c;
    double mass = 0.0, yz = 0.0;
    for (int k = lane; k < c; k += 64) {
      const double yk = (double)yr[k];
      mass += yk;
      if (yk != 0.0) yz += yk * (double)z[k];     // a zero weight takes no part, whatever the logit (-inf included)
    }
    o.mass = wave_sum(mass);
    o.loss = o.lse * o.mass - wave_sum(yz);
    o.kept = 1;
    o.y = 0;
  }
  return o;
}

__global__ void __launch_bounds__(CE_THREADS) ce_kernel(int n, int c, const float* logits, const void* target, int kind, long ignore_index,
                                                        int reduction, float* loss, float* dsaved) {
  __shared__ double wsum[CE_WAVES];
  __shared__ int wcnt[CE_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  int cnt = 0;
  for (long r = wave; r < n; r += CE_WAVES) {
    const CeRow o = ce_row(logits + r * (long)c, target, kind, ignore_index, c, r, lane);
    acc += o.loss;
    cnt += o.kept;
    if (reduction == 0 && lane == 0) loss[r] = (float)o.loss;
  }
  if (lane == 0) { wsum[wave] = acc; wcnt[wave] = cnt; }
  __syncthreads();
  double total = 0.0;
  int kept = 0;
  for (int w = 0; w < CE_WAVES; ++w) { total += wsum[w]; kept += wcnt[w]; }
  // mean: index targets divide by the rows kept (0 -> NaN, as torch), probability targets by n
  const double div = reduction == 2 ? (kind == 0 ? (double)kept : (double)n) : 1.0;
  if (reduction != 0 && threadIdx.x == 0) loss[0] = (float)(reduction == 2 ? total / div : total);
  if (!dsaved) return;
  for (long r = wave; r < n; r += CE_WAVES) {
    const float* z = logits + r * (long)c;
    const CeRow o = ce_row(z, target, kind, ignore_index, c, r, lane);
    float* g = dsaved + r * (long)c;
    const bool bad = kind == 0 && o.kept && (o.y < 0 || o.y >= c);
    for (int k = lane; k < c; k += 64) {
      double v;
      if (!o.kept) v = 0.0;
      else if (bad) v = __longlong_as_double(0x7ff8000000000000ll);
      else {
        const double yk = kind == 0 ? (k == o.y ? 1.0 : 0.0) : (double)static_cast<const float*>(target)[r * (long)c + k];
        v = (exp((double)z[k] - o.lse) * o.mass - yk) / div;
      }
      g[k] = (float)v;
    }
  }
}

__global__ void __launch_bounds__(256) ce_backward_kernel(long total, int c, const float* saved, const float* dloss, int per_row, float* out) {
  for (long e = blockIdx.x * 256l + threadIdx.x; e < total; e += (long)gridDim.x * 256) out[e] = saved[e] * dloss[per_row ? e / c : 0];
}

// =====================================================================================================================
// sweep state.  Byte layout (also read by mmnn_sts_amd/utils/find_lr.py):
//   0 float total | 4 int live | 8 int stop_iter | 12 int iters_done | 16 int num_iter | 20 pad | 24 double best | 32 double prev
//   40 double hist[num_iter]
// One thread does every step, in the order and the roundings of torch-lr-finder's Python (fp32 loss sum, fp64 smoothing).
// =====================================================================================================================
struct LrRangeState {
  float total;
  int live, stop_iter, iters_done, num_iter, pad;
  double best, prev;
  double hist[1];
};
static_assert(offsetof(LrRangeState, best) == 24 && offsetof(LrRangeState, hist) == 40, "lr range state layout");

__global__ void lr_range_init_kernel(LrRangeState* s, int num_iter) {
  for (int i = threadIdx.x; i < num_iter; i += blockDim.x) s->hist[i] = 0.0;
  if (threadIdx.x == 0) {
    s->total = 0.f;
    s->live = 1; s->stop_iter = -1; s->iters_done = 0; s->num_iter = num_iter; s->pad = 0;
    s->best = 0.0; s->prev = 0.0;
  }
}

__global__ void lr_range_accumulate_kernel(LrRangeState* s, const float* loss, float steps, int first) {
  if (threadIdx.x != 0 || !s->live) return;
  const float l = __fdiv_rn(loss[0], steps);            // loss /= accumulation_steps (steps == 1: unchanged)
  s->total = first ? l : __fadd_rn(s->total, l);        // total_loss += loss
}

__global__ void lr_range_update_kernel(LrRangeState* s, int iter, double smooth_f, double one_minus_smooth_f, double diverge_th) {
  if (threadIdx.x != 0 || !s->live || iter < 0 || iter >= s->num_iter) return;
  const double raw = (double)s->total;
  double v;
  if (iter == 0) {
    s->best = raw;
    v = raw;
  } else {
    v = smooth_f > 0.0 ? __dadd_rn(__dmul_rn(smooth_f, raw), __dmul_rn(one_minus_smooth_f, s->prev)) : raw;
    if (v < s->best) s->best = v;                       // NaN compares false: never the best
  }
  s->hist[iter] = v;
  s->prev = v;
  s->iters_done = iter + 1;
  if (v > __dmul_rn(diverge_th, s->best)) {             // NaN compares false: never a stop
    s->live = 0;
    s->stop_iter = iter;
  }
}

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int mmnn_cross_entropy(int32_t n, int32_t c, const float* logits, const void* target, int32_t target_kind, int64_t ignore_index,
                       int32_t reduction, float* loss, float* dlogits_saved, void* stream) {
  MMNN_REQUIRE(n >= 1 && c >= 1 && c <= 1024, "cross_entropy: need n >= 1 and 1 <= c <= 1024, got n=%d c=%d", n, c);
  MMNN_REQUIRE(target_kind == 0 || target_kind == 1, "cross_entropy: target_kind must be 0 (int64 index) or 1 (fp32 probabilities)");
  MMNN_REQUIRE(reduction >= 0 && reduction <= 2, "cross_entropy: reduction must be 0 (none), 1 (sum) or 2 (mean)");
  MMNN_REQUIRE(logits && target && loss, "cross_entropy: null pointer");
  MMNN_LAUNCH(ce_kernel, dim3(1), dim3(CE_THREADS), 0, static_cast<hipStream_t>(stream), (int)n, (int)c, logits, target, (int)target_kind,
              (long)ignore_index, (int)reduction, loss, dlogits_saved);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int mmnn_cross_entropy_backward(int32_t n, int32_t c, int32_t reduction, const float* dlogits_saved, const float* dloss, float* dlogits,
                                void* stream) {
  MMNN_REQUIRE(n >= 1 && c >= 1 && c <= 1024, "cross_entropy_backward: need n >= 1 and 1 <= c <= 1024, got n=%d c=%d", n, c);
  MMNN_REQUIRE(reduction >= 0 && reduction <= 2, "cross_entropy_backward: reduction must be 0, 1 or 2");
  MMNN_REQUIRE(dlogits_saved && dloss && dlogits, "cross_entropy_backward: null pointer");
  const long total = (long)n * c;
  const int blocks = (int)std::min<long>(1024, (total + 255) / 256);
  MMNN_LAUNCH(ce_backward_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), total, (int)c, dlogits_saved, dloss,
              reduction == 0 ? 1 : 0, dlogits);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int64_t mmnn_lr_range_state_bytes(int32_t num_iter) {
  if (num_iter < 1) return -1;
  return (int64_t)offsetof(LrRangeState, hist) + 8 * (int64_t)num_iter;
}

int mmnn_lr_range_init(void* state, int32_t num_iter, void* stream) {
  MMNN_REQUIRE(state && num_iter >= 1, "lr_range_init: need a state buffer and num_iter >= 1");
  MMNN_REQUIRE(((uintptr_t)state & 7) == 0, "lr_range_init: the state buffer must be 8-byte aligned");
  MMNN_LAUNCH(lr_range_init_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<LrRangeState*>(state), (int)num_iter);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int mmnn_lr_range_accumulate(void* state, const float* loss, float steps_or_1, int32_t first, void* stream) {
  MMNN_REQUIRE(state && loss, "lr_range_accumulate: null pointer");
  MMNN_LAUNCH(lr_range_accumulate_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<LrRangeState*>(state), loss,
              steps_or_1, (int)first);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int mmnn_lr_range_update(void* state, int32_t iter, double smooth_f, double one_minus_smooth_f, double diverge_th, void* stream) {
  MMNN_REQUIRE(state && iter >= 0, "lr_range_update: null state or negative iteration");
  MMNN_LAUNCH(lr_range_update_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<LrRangeState*>(state), (int)iter,
              smooth_f, one_minus_smooth_f, diverge_th);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int mmnn_sgd_step_dev(float* params, const float* grads, float* momentum_buf, int64_t n, const float* lr, const int32_t* live, float momentum,
                      float weight_decay, int32_t nesterov, int32_t first_step, void* stream) {
  return launch_sgd_dev(params, grads, momentum_buf, n, lr, live, momentum, weight_decay, nesterov, first_step, static_cast<hipStream_t>(stream));
}

int mmnn_sgd_step_multi_dev(const mmnn_tensor_ref* refs, int32_t n, float* momentum_buf, const float* lr, const int32_t* live, float momentum,
                            float weight_decay, int32_t nesterov, void* stream) {
  return launch_sgd_multi_dev(refs, n, momentum_buf, lr, live, momentum, weight_decay, nesterov, static_cast<hipStream_t>(stream));
}

}  // extern "C"
