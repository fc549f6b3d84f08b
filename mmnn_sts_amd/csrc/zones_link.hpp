// Union-find on a parent array, for the connected-component labelling of csrc/radiomics_zones.hip.  The routines are __host__ __device__
// so that the same text runs on the CPU (one thread or several) as on the device.
//
// The invariant.  parent[v] == v at the start for every voxel, and every later write to `parent` is an atomic minimum with a smaller
// index.  So parent[v] <= v holds at all times and a slot's value only ever decreases.
//   * zone_find walks v -> parent[v] while the value read is smaller than v: the index strictly decreases, so the walk ends after at most
//     v steps whatever other threads write meanwhile (a stale read is an older, larger ancestor: the walk is longer, never wrong).
//   * zone_link: every turn of its loop either returns or replaces the larger of its two indices by a smaller one (the value the atomic
//     returned, below the slot's index), and the finds in between only decrease them: a + b strictly decreases, so it ends.
//   * Connectivity is kept: the atomic minimum on slot a with value b found a either a root (old == a: a now hangs under b, done) or
//     hanging under `old`.  In the second case a now hangs under min(old, b) and the thread goes on to link `old` with b, so a, old and
//     b still end in one tree whichever of the two the slot kept.
//   * The root of a finished tree is the smallest index of its set: a root is only ever hung under a smaller index.  That is the
//     canonical label, independent of the order of the merges.
//   * zone_compress hangs v under the root it found: an ancestor, smaller than the value it replaces, by the same atomic minimum.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MMNN_ZONES_HD __host__ __device__ __forceinline__
#else
#define MMNN_ZONES_HD inline
#endif

namespace mmnn {

MMNN_ZONES_HD uint32_t zone_load(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

// parent[slot] = min(parent[slot], v); returns what the slot held
MMNN_ZONES_HD uint32_t zone_min(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicMin(p, v);
#else
  uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
#endif
}

MMNN_ZONES_HD uint32_t zone_find(const uint32_t* parent, uint32_t v) {
  uint32_t p;
  while ((p = zone_load(parent + v)) < v) v = p;
  return v;
}

MMNN_ZONES_HD void zone_link(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = zone_find(parent, a);
    b = zone_find(parent, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = zone_min(parent + a, b);
    if (old >= a) return;               // a was a root and hangs under b now
    a = old;                            // a hung under `old` already: `old` and b are what is left to join
  }
}

MMNN_ZONES_HD void zone_compress(uint32_t* parent, uint32_t v) {
  const uint32_t r = zone_find(parent, v);
  if (zone_load(parent + v) > r) zone_min(parent + v, r);
}

}  // namespace mmnn
