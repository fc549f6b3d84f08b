// The workgroup side of what the compressed-series kernels share (csrc/dicom_rle.hip, csrc/dicom_jpegll.hip): filling the LDS window
// from an untrusted payload, and resolving the chunk's successor chain by pointer doubling (csrc/stream_core.hpp: chain_hop).  Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "stream_core.hpp"

namespace mmnn {

// lds[0, WINDOW) = payload[base, base + WINDOW), zeros behind the payload's end.  `base` is a multiple of 16 and `payload` aligned
// to 16 bytes: aligned 16-byte loads, the payload's ragged end by bytes.  No barrier: the caller's next one publishes the window.
template <int WINDOW, int TPB>
__device__ __forceinline__ void window_fill(uint8_t* lds, const uint8_t* payload, long payload_bytes, long base, int tid) {
  static_assert(WINDOW % 16 == 0, "whole 16-byte cells");
  for (int v = tid; v < WINDOW / 16; v += TPB) {
    const long g = base + 16l * v;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (g + 16 <= payload_bytes) {
      q = *reinterpret_cast<const uint4*>(payload + g);
    } else if (g < payload_bytes) {          // the payload's ragged end
      unsigned w[4] = {0u, 0u, 0u, 0u};
      for (int i = 0; i < 16 && g + i < payload_bytes; ++i) w[i >> 2] |= (unsigned)payload[g + i] << (8 * (i & 3));
      q = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(lds + 16 * v) = q;
  }
}

// Marks the members of the chain that enters a chunk of N positions at `entry`: hop[p] = successor(p) for every p, mark[entry] = 1,
// then at most ROUNDS rounds of chain_hop<N> with two barriers each, fewer when the steps are long (the rounds stop once the entry's
// pointer has left the chunk).  Lanes along the positions (thread t has t, t + TPB, ...), so that neighbouring lanes read
// neighbouring entries.
// The barrier contract: EVERY thread of the block calls it, with `entry` and `enters` the same in every thread (`enters` false: the
// entry is no position of the chain, nothing is marked and no round runs); `mark` is all zero and published before the call, and
// nobody else writes `hop` or `mark` until it returns.  It returns behind a barrier: hop and mark are final and visible to all, and
// whatever the callers wrote to other shared words in front of the call (one writer per word) is visible too.
template <int N, int TPB, int ROUNDS, typename Successor>
__device__ __forceinline__ void chain_resolve(uint16_t* hop, uint8_t* mark, int entry, bool enters, int tid, Successor successor) {
  constexpr int PER = N / TPB;
  static_assert(N % TPB == 0 && (1 << ROUNDS) >= N, "positions per thread, rounds of pointer doubling");
#pragma unroll
  for (int i = 0; i < PER; ++i) hop[i * TPB + tid] = (uint16_t)successor(i * TPB + tid);
  if (tid == 0 && enters) mark[entry] = 1;
  __syncthreads();
  for (int k = 0; k < ROUNDS && enters; ++k) {
    uint16_t on[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) on[i] = chain_hop<N>(hop, mark, i * TPB + tid);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) hop[i * TPB + tid] = on[i];
    __syncthreads();
    if (hop[entry] >= N) break;              // (the same word in every thread; the next write of hop lies behind the next barrier)
  }
}

}  // namespace mmnn
