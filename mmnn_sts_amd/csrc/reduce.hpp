// Wave and workgroup reductions: the one copy of the lane butterfly and of its workgroup follow-up.
//
// Order.  wave_reduce folds the 64 lanes by the xor butterfly, offsets 32, 16, ... 1, as v = op(v, other lane's v): every lane ends with
// the same value.  block_reduce then folds the waves' values in wave-index order, left-associated from wave 0:
// op(... op(op(w0, w1), w2) ..., w_last).  Both orders are fixed, so a floating-point sum is the same bits on every call.
//
// Operator.  The functor is how a call site says which combine it means.  Sum adds.  Less / Greater compare (`b < a ? b : a`): a NaN in
// `a` stays, +0 and -0 are equal.  FMin / FMax / FMinMax call fminf / fmaxf (fmin / fmax for double): a NaN operand is dropped.  The two
// families differ on NaN and on the sign of zero, and no site is moved from one to the other.  block_reduce hands the functor the index k
// of the value as a third argument, so that one call can fold values with different operators (FMinMax: [0] is a minimum, [1] a maximum).
//
// block_reduce<WAVES>(v, lds, op): every thread of a one-dimensional workgroup of WAVES * 64 threads calls it, with K values each and
// the same `lds` of WAVES * K elements; on return v holds the workgroup's results in EVERY thread.  Its two barriers:
//   (1) before the LDS writes: every thread has finished reading `lds` -- the combine loop of an earlier call on the same buffer, or
//       whatever else the caller keeps there.  This is what makes two calls in a row on one buffer safe;
//   (2) between the writes and the reads: the reads see this call's values.  Every word read was written after (1) in this call (each
//       wave's lane 0 writes its K words), so nothing depends on what LDS held before.
// There is no barrier after the reads: a caller that writes `lds` itself after the call needs its own.
#pragma once
#include "common.hpp"

namespace mmnn {

#if defined(__HIPCC__)
struct Sum {
  template <class T> __device__ __forceinline__ T operator()(T a, T b, int = 0) const { return a + b; }
};
struct Less {
  template <class T> __device__ __forceinline__ T operator()(T a, T b, int = 0) const { return b < a ? b : a; }
};
struct Greater {
  template <class T> __device__ __forceinline__ T operator()(T a, T b, int = 0) const { return b > a ? b : a; }
};
struct FMin {
  __device__ __forceinline__ float operator()(float a, float b, int = 0) const { return fminf(a, b); }
};
struct FMax {
  __device__ __forceinline__ float operator()(float a, float b, int = 0) const { return fmaxf(a, b); }
};
struct FMinMax {   // value 0: minimum, value 1: maximum
  __device__ __forceinline__ float operator()(float a, float b, int k) const { return k ? fmaxf(a, b) : fminf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b, int k) const { return k ? fmax(a, b) : fmin(a, b); }
};

template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, Sum{}); }

template <int WAVES, int K, class T, class Op>
__device__ __forceinline__ void block_reduce(T (&v)[K], T* lds, Op op) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_reduce(v[k], [&](T a, T b) { return op(a, b, k); });
  __syncthreads();   // (1)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) lds[wave * K + k] = v[k];
  }
  __syncthreads();   // (2)
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T t = lds[k];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t = op(t, lds[w * K + k], k);
    v[k] = t;
  }
}

template <int WAVES, class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* lds, Op op) {
  T a[1] = {v};
  block_reduce<WAVES>(a, lds, op);
  return a[0];
}

// block_exclusive_scan<WAVES>(v, lds, total): every thread of a one-dimensional workgroup of WAVES * 64 threads calls it with one value
// and the same `lds` of WAVES elements.  It returns the sum of the values of the threads in front of the caller, in thread-index order,
// and sets `total` to the sum of all of them in every thread.  Integer sums in mind: the lanes fold by the shift-up ladder (offsets
// 1, 2, ... 32), the waves in wave-index order.  Its two barriers are block_reduce's (1) and (2), with the same consequences.
template <int WAVES, class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* lds, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  __syncthreads();   // (1)
  if (lane == 63) lds[wave] = s;
  __syncthreads();   // (2)
  T before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const T t = lds[w];
    if (w < wave) before += t;
    total += t;
  }
  return before + s - v;
}
#endif  // __HIPCC__

}  // namespace mmnn
