// The grey-level size-zone matrix (GLSZM) of one (scan, mask) pair, from what `mmnn_radiomics` (csrc/radiomics.hip) left on the device:
// the uint16 bin volume (0 outside the ROI) in its workspace and Ng, n and the flags in the state block there.  The contract is the
// comment above mmnn_radiomics_zones in include/mmnn_sts.h.  Everything is enqueued on the caller's stream behind the extraction; nothing
// is read back and the host never waits.
//
//   memsets                labels, sizes, levels; the two hash tables and the integer accumulators in ws3
//   zones_init_kernel      parent[v] = v
//   zones_link_kernel      an ROI voxel links itself to each of its 13 earlier neighbours (the directions of radiomics.hpp, negated) that
//                          lies in the volume and shares its bin: union-find by atomic minimum (zones_link.hpp states the invariant that
//                          bounds every walk and retry), then hangs itself under the root it finds
//   zones_label_kernel     labels[v] = 1 + root; one count at sizes[root], the lanes of a wave that agree on the root folded into one add
//   zones_insert_kernel    a root (sizes[v] > 0) of level i and size j puts the key (i, j) into the open-addressing table of the joint
//                          counts: the slot's count += 1, its owner = min(owner, v).  Lanes of a wave with the same key send one add; the
//                          probe reads before it swaps and the owner is only lowered when the slot holds a larger one, so a key that is
//                          already there costs one atomic
//   zones_marginal_kernel  a sweep over the table's slots: levels[i - 1] += P, key j into the table of ps(j) (count += P, owner = min),
//                          nz and sum j^2 as integers
//   zones_features_kernel  a fixed-partition sweep: a root that owns its key adds that key's terms; per-workgroup partial sums
//   zones_final_kernel     one workgroup: the partials, the sums over the levels, the result block; the NaN block with a flag
//
// The tables cannot fill.  Level i holds at most sqrt(2 n_i) distinct sizes (1 + 2 + ... + d <= n_i), so by Cauchy-Schwarz the matrix has
// at most sqrt(2 n Ng) <= sqrt(2 x y z max_bins) distinct (i, j); the table has the next power of two above twice that many slots, the one
// keyed by j alone the same from sqrt(2 x y z).  A probe therefore always meets its key or a free slot.  Both tables live in ws3 (global
// memory) at every Ng: there is no LDS variant and no threshold.
//
// Determinism.  labels, sizes, levels, the slots' counts and owners and the six integers are exact and independent of the order of the
// atomics (minimum and integer add).  Every fp64 sum runs over the distinct keys, each met at its owner voxel: a lane adds its voxels in
// ascending order, a wave folds its lanes by the xor butterfly and the four waves are added in index order (block_reduce, reduce.hpp);
// the workgroups' sums are folded the same way by the last kernel, one lane per workgroup.  The partition is fixed by the extents.
// No floating-point atomics.  All index arithmetic is 32-bit (x * y * z < 2^31).
#include "ingest_load.hpp"
#include "radiomics.hpp"
#include "zones_link.hpp"

#include <cmath>

namespace mmnn {

constexpr int ZN_CHUNKS = 1024;             // workgroups of the labelling passes (at most)
constexpr int ZN_SLOTS = 8;                 // fp64 partial sums per workgroup of the feature sweep (seven used)
constexpr int ZN_ACC = 8;                   // integer accumulators: nz, sum j^2, sum ps^2, n_keys, max_size
constexpr int ZN_NF = MMNN_RADIOMICS_GLSZM;
static_assert(RAD_TPB >= RAD_MAX_PARTS, "zones_final_kernel holds one workgroup of the feature sweep per lane");
enum { ZA_NZ = 0, ZA_J2 = 1, ZA_PS2 = 2, ZA_KEYS = 3, ZA_MAX = 4 };
enum { ZS_SAE = 0, ZS_ZV = 1, ZS_ENT = 2, ZS_SALG = 3, ZS_SAHG = 4, ZS_LALG = 5, ZS_LAHG = 6 };

struct ZoneArgs : RadFollow {
  int max_bins, parts;
  uint32_t* labels; uint32_t* sizes; uint32_t* levels;
  uint32_t* parent;                         // [N]
  unsigned long long* keys;                 // [kmask + 1]: (i << 32) | j, 0 = free
  uint32_t* kcnt; uint32_t* kown;
  uint32_t* jkeys; uint32_t* jcnt; uint32_t* jown;      // [jmask + 1]: j, 0 = free
  unsigned kmask, jmask;
  unsigned long long* acc;                  // [ZN_ACC]
  double* part;                             // [parts][ZN_SLOTS]
  mmnn_radiomics_zones_result* out;
};

__global__ void __launch_bounds__(RAD_TPB) zones_init_kernel(const ZoneArgs a) {
  const unsigned stride = gridDim.x * RAD_TPB;
  for (unsigned idx = blockIdx.x * RAD_TPB + threadIdx.x; idx < a.N; idx += stride) a.parent[idx] = idx;
}

// ---- labelling -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RAD_TPB) zones_link_kernel(const ZoneArgs a) {
  if (a.st->flagged) return;
  const unsigned ng = (unsigned)a.st->n_bins;
  const unsigned X = a.X, XY = (unsigned)a.X * a.Y;
  const unsigned stride = gridDim.x * RAD_TPB;
  for (unsigned idx = blockIdx.x * RAD_TPB + threadIdx.x; idx < a.N; idx += stride) {
    const unsigned b = a.bins[idx];
    if (b == 0u || b > ng) continue;
    int x, y, z;
    rad_split(idx, X, XY, x, y, z);
    bool linked = false;
    for (int d = 0; d < RAD_DIRS; ++d) {
      const int dz = rad_dirs[d][0], dy = rad_dirs[d][1], dx = rad_dirs[d][2];
      const int px = x - dx, py = y - dy, pz = z - dz;                  // the test is made on (x, y, z): no wrap over a row or slice end
      if (px < 0 || px >= a.X || py < 0 || py >= a.Y || pz < 0) continue;      // (dz >= 0: pz < Z)
      const unsigned q = idx - (unsigned)((dz * a.Y + dy) * a.X + dx);         // in the volume: 0 <= q < idx
      if (a.bins[q] != b) continue;
      zone_link(a.parent, idx, q);
      linked = true;
    }
    if (linked) zone_compress(a.parent, idx);
  }
}

// Every lane of a workgroup makes the same number of trips, so the ballots inside rad_count see whole waves.
__global__ void __launch_bounds__(RAD_TPB) zones_label_kernel(const ZoneArgs a) {
  if (a.st->flagged) return;
  const unsigned ng = (unsigned)a.st->n_bins;
  const unsigned stride = gridDim.x * RAD_TPB;
  const unsigned trips = (a.N + stride - 1u) / stride;
  unsigned idx = blockIdx.x * RAD_TPB + threadIdx.x;
  for (unsigned t = 0; t < trips; ++t, idx += stride) {                 // idx < N + stride < 2^32
    unsigned b = 0u;
    if (idx < a.N) b = a.bins[idx];
    const bool roi = b != 0u && b <= ng;
    unsigned root = 0u;
    if (roi) {
      root = zone_find(a.parent, idx);
      a.labels[idx] = root + 1u;
    }
    rad_count(a.sizes, root, roi);
  }
}

// ---- the joint count ---------------------------------------------------------------------------------------------------------------------
// Keys are written once (0 -> key) and owners only decrease, so a read that is behind the other lanes' atomics only costs the atomic
// it would have saved: a key read as free goes to the swap, an owner read too large goes to the minimum.
__device__ __forceinline__ void zone_insert(const ZoneArgs& a, unsigned long long key, unsigned count, unsigned v) {
  unsigned slot = (unsigned)mix64(key) & a.kmask;
  for (;;) {                                                            // the table is never more than half full: ends at the key or a free slot
    unsigned long long prev = __hip_atomic_load(&a.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == 0ull) prev = atomicCAS(&a.keys[slot], 0ull, key);
    if (prev == 0ull || prev == key) break;
    slot = (slot + 1u) & a.kmask;
  }
  atomicAdd(&a.kcnt[slot], count);
  if (__hip_atomic_load(&a.kown[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(&a.kown[slot], v);
}

__device__ __forceinline__ void zone_insert_size(const ZoneArgs& a, unsigned j, unsigned count, unsigned v) {
  unsigned slot = (unsigned)mix64((unsigned long long)j) & a.jmask;
  for (;;) {
    const unsigned prev = atomicCAS(&a.jkeys[slot], 0u, j);
    if (prev == 0u || prev == j) break;
    slot = (slot + 1u) & a.jmask;
  }
  atomicAdd(&a.jcnt[slot], count);
  atomicMin(&a.jown[slot], v);
}

__global__ void __launch_bounds__(RAD_TPB) zones_insert_kernel(const ZoneArgs a) {
  if (a.st->flagged) return;
  const unsigned stride = gridDim.x * RAD_TPB;
  const unsigned trips = (a.N + stride - 1u) / stride;
  const int lane = threadIdx.x & 63;
  unsigned idx = blockIdx.x * RAD_TPB + threadIdx.x;
  for (unsigned t = 0; t < trips; ++t, idx += stride) {                 // every lane makes the same trips: the ballots see whole waves
    unsigned j = 0u, i = 0u;
    if (idx < a.N) j = a.sizes[idx];
    const bool root = j != 0u;
    if (root) i = a.bins[idx];
    // the lanes that share a key send one add.  A wave's voxel indices ascend with the lane, so the first lane of a group holds the
    // group's smallest index: it is the one that inserts
    const unsigned long long key = ((unsigned long long)i << 32) | j;
    unsigned long long todo = __ballot(root);
    while (todo) {                                                      // (uniform over the wave)
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned long long k0 = __shfl(key, leader, 64);
      const unsigned long long m = __ballot(root && key == k0);
      if (lane == leader) zone_insert(a, key, (unsigned)__popcll(m), idx);
      todo &= ~m;
    }
  }
}

// grid-stride over the slots of the joint table: at most sqrt(2 n Ng) of them are taken
__global__ void __launch_bounds__(RAD_TPB) zones_marginal_kernel(const ZoneArgs a) {
  if (a.st->flagged) return;
  const unsigned stride = gridDim.x * RAD_TPB;
  unsigned long long nz = 0ull, j2 = 0ull;
  for (unsigned slot = blockIdx.x * RAD_TPB + threadIdx.x; slot <= a.kmask; slot += stride) {
    const unsigned long long key = a.keys[slot];
    if (key == 0ull) continue;
    const unsigned i = (unsigned)(key >> 32), j = (unsigned)key, c = a.kcnt[slot];
    atomicAdd(&a.levels[i - 1u], c);
    zone_insert_size(a, j, c, a.kown[slot]);
    nz += c;
    j2 += (unsigned long long)c * j * j;
  }
  const int lane = threadIdx.x & 63;
  nz = wave_sum(nz);
  j2 = wave_sum(j2);
  if (lane == 0 && nz) {
    atomicAdd(&a.acc[ZA_NZ], nz);
    atomicAdd(&a.acc[ZA_J2], j2);
  }
}

// ---- features ----------------------------------------------------------------------------------------------------------------------------
// grid a.parts workgroups.  Workgroup b takes the voxels b * TPB + t, + parts * TPB, ...
__global__ void __launch_bounds__(RAD_TPB) zones_features_kernel(const ZoneArgs a) {
  __shared__ double red[(RAD_TPB / 64) * ZN_SLOTS];
  if (a.st->flagged) return;
  const double Nz = (double)a.acc[ZA_NZ], mu_j = (double)a.st->n / Nz;      // mu_j = sum_j j ps(j) / Nz = n / Nz
  const unsigned stride = gridDim.x * RAD_TPB;
  double s[ZN_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned long long ps2 = 0ull, nk = 0ull, mx = 0ull;
  for (unsigned idx = blockIdx.x * RAD_TPB + threadIdx.x; idx < a.N; idx += stride) {
    const unsigned j = a.sizes[idx];
    if (j == 0u) continue;
    const unsigned i = a.bins[idx];
    const double jd = (double)j, jj = jd * jd;
    unsigned slot = (unsigned)mix64((unsigned long long)j) & a.jmask;
    while (a.jkeys[slot] != j) slot = (slot + 1u) & a.jmask;            // the key was inserted: the probe meets it before a free slot
    if (a.jown[slot] == idx) {
      const unsigned long long c = a.jcnt[slot];
      const double ps = (double)c, cj = jd - mu_j;
      s[ZS_SAE] += ps / jj;
      s[ZS_ZV] += (ps / Nz) * (cj * cj);
      ps2 += c * c;
      mx = j > mx ? j : mx;
    }
    const unsigned long long key = ((unsigned long long)i << 32) | j;
    slot = (unsigned)mix64(key) & a.kmask;
    while (a.keys[slot] != key) slot = (slot + 1u) & a.kmask;
    if (a.kown[slot] == idx) {
      const double P = (double)a.kcnt[slot], ii = (double)i * (double)i;
      s[ZS_ENT] += rad_plogp(P / Nz);
      s[ZS_SALG] += P / (ii * jj);
      s[ZS_SAHG] += P * ii / jj;
      s[ZS_LALG] += P * jj / ii;
      s[ZS_LAHG] += P * (ii * jj);
      nk += 1ull;
    }
  }
  block_reduce<RAD_TPB / 64>(s, red, Sum{});
  if (threadIdx.x < ZN_SLOTS) a.part[blockIdx.x * ZN_SLOTS + threadIdx.x] = s[threadIdx.x];
  ps2 = wave_sum(ps2);
  nk = wave_sum(nk);
  mx = wave_reduce(mx, Greater{});
  if ((threadIdx.x & 63) == 0 && nk + ps2) {
    atomicAdd(&a.acc[ZA_PS2], ps2);
    atomicAdd(&a.acc[ZA_KEYS], nk);
    atomicMax(&a.acc[ZA_MAX], mx);
  }
}

// one workgroup of RAD_TPB >= RAD_MAX_PARTS lanes
__global__ void __launch_bounds__(RAD_TPB) zones_final_kernel(const ZoneArgs a) {
  __shared__ double red[(RAD_TPB / 64) * ZN_SLOTS];
  __shared__ unsigned long long ired[RAD_TPB / 64];
  const int t = threadIdx.x;
  long long* oi = reinterpret_cast<long long*>(a.out);                  // nz, n_keys, max_size, sum_pg2, sum_ps2, sum_j2
  if (a.st->flagged) {
    if (t < 6) oi[t] = 0;
    if (t < ZN_NF) a.out->glszm[t] = rad_nan();
    return;
  }
  const int ng = a.st->n_bins;
  const double Nz = (double)a.acc[ZA_NZ], Np = (double)a.st->n;
  unsigned long long g2 = 0ull;
  double b3[3] = {0.0, 0.0, 0.0};
  for (int i = t; i < ng; i += RAD_TPB) {
    const unsigned long long c = a.levels[i];
    const double g = (double)c, ii = (double)(i + 1);
    g2 += c * c;
    b3[0] += g / (ii * ii);
    b3[1] += g * (ii * ii);
    b3[2] += ii * (g / Nz);
  }
  block_reduce<RAD_TPB / 64>(b3, red, Sum{});
  g2 = block_reduce<RAD_TPB / 64>(g2, ired, Sum{});
  const double mu_i = b3[2];
  double glv = 0.0;
  for (int i = t; i < ng; i += RAD_TPB) { const double c = (double)(i + 1) - mu_i; glv += ((double)a.levels[i] / Nz) * (c * c); }
  glv = block_reduce<RAD_TPB / 64>(glv, red, Sum{});
  double s[ZN_SLOTS];                                                   // lane p holds the sums of workgroup p of the feature sweep
  for (int k = 0; k < ZN_SLOTS; ++k) s[k] = t < a.parts ? a.part[t * ZN_SLOTS + k] : 0.0;
  block_reduce<RAD_TPB / 64>(s, red, Sum{});
  if (t != 0) return;
  const unsigned long long j2 = a.acc[ZA_J2], ps2 = a.acc[ZA_PS2];
  oi[0] = (long long)a.acc[ZA_NZ];
  oi[1] = (long long)a.acc[ZA_KEYS];
  oi[2] = (long long)a.acc[ZA_MAX];
  oi[3] = (long long)g2;
  oi[4] = (long long)ps2;
  oi[5] = (long long)j2;
  double* f = a.out->glszm;
  f[0] = s[ZS_SAE] / Nz;
  f[1] = (double)j2 / Nz;
  f[2] = (double)g2 / Nz;
  f[3] = (double)g2 / (Nz * Nz);
  f[4] = (double)ps2 / Nz;
  f[5] = (double)ps2 / (Nz * Nz);
  f[6] = Nz / Np;
  f[7] = glv;
  f[8] = s[ZS_ZV];
  f[9] = -s[ZS_ENT];
  f[10] = b3[0] / Nz;
  f[11] = b3[1] / Nz;
  f[12] = s[ZS_SALG] / Nz;
  f[13] = s[ZS_SAHG] / Nz;
  f[14] = s[ZS_LALG] / Nz;
  f[15] = s[ZS_LAHG] / Nz;
}

namespace {

struct ZoneLayout { size_t parent, keys, kcnt, jkeys, jcnt, acc, kown, jown, part, total; unsigned kslots, jslots; };

// the next power of two above twice ceil(sqrt(v))
unsigned zone_slots(double v) {
  const unsigned long long need = 2ull * (unsigned long long)std::ceil(std::sqrt(v));
  unsigned s = 1u;
  while (s <= need) s <<= 1;                                           // v <= 2^42: s <= 2^23
  return s;
}

ZoneLayout zone_layout(long n, int max_bins) {
  ZoneLayout Z;
  Carver cv;
  Z.kslots = zone_slots(2.0 * (double)n * max_bins);
  Z.jslots = zone_slots(2.0 * (double)n);
  Z.parent = cv.take((size_t)n * 4);
  Z.keys = cv.take((size_t)Z.kslots * 8);                               // keys .. acc are zeroed by one memset
  Z.kcnt = cv.take((size_t)Z.kslots * 4);
  Z.jkeys = cv.take((size_t)Z.jslots * 4);
  Z.jcnt = cv.take((size_t)Z.jslots * 4);
  Z.acc = cv.take((size_t)ZN_ACC * 8);
  Z.kown = cv.take((size_t)Z.kslots * 4);                               // the owners start from 0xffffffff, by one memset
  Z.jown = cv.take((size_t)Z.jslots * 4);
  Z.part = cv.take((size_t)RAD_MAX_PARTS * ZN_SLOTS * 8);
  Z.total = cv.cur;
  return Z;
}

}  // namespace

}  // namespace mmnn

using namespace mmnn;

extern "C" {

int64_t mmnn_radiomics_zones_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins) {
  if (rad_validate(x, y, z, max_bins) != 0) return -1;
  return (int64_t)zone_layout((long)x * y * z, max_bins).total;
}

int mmnn_radiomics_zones(const mmnn_radiomics_desc* d, const mmnn_radiomics_result* result, const void* ws,
                         mmnn_radiomics_zones_result* out, uint32_t* labels, uint32_t* sizes, uint32_t* levels, void* ws3,
                         void* stream_) {
  if (rad_validate_follow("radiomics_zones", d) != 0) return 1;
  MMNN_REQUIRE(result && ws && out && labels && sizes && levels && ws3, "radiomics_zones: null argument");
  MMNN_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)ws3 % 256 == 0 && (uintptr_t)result % 8 == 0 && (uintptr_t)out % 8 == 0 &&
                   (uintptr_t)labels % 4 == 0 && (uintptr_t)sizes % 4 == 0 && (uintptr_t)levels % 4 == 0,
               "radiomics_zones: misaligned workspace / result / table");
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  ZoneArgs a{};
  static_cast<RadFollow&>(a) = rad_follow(d, ws);
  const long n = (long)a.N;
  const ZoneLayout Z = zone_layout(n, d->max_bins);
  char* w3 = static_cast<char*>(ws3);
  a.max_bins = d->max_bins;
  a.labels = labels; a.sizes = sizes; a.levels = levels;
  a.parent = reinterpret_cast<uint32_t*>(w3 + Z.parent);
  a.keys = reinterpret_cast<unsigned long long*>(w3 + Z.keys);
  a.kcnt = reinterpret_cast<uint32_t*>(w3 + Z.kcnt);
  a.kown = reinterpret_cast<uint32_t*>(w3 + Z.kown);
  a.jkeys = reinterpret_cast<uint32_t*>(w3 + Z.jkeys);
  a.jcnt = reinterpret_cast<uint32_t*>(w3 + Z.jcnt);
  a.jown = reinterpret_cast<uint32_t*>(w3 + Z.jown);
  a.kmask = Z.kslots - 1u; a.jmask = Z.jslots - 1u;
  a.acc = reinterpret_cast<unsigned long long*>(w3 + Z.acc);
  a.part = reinterpret_cast<double*>(w3 + Z.part);
  a.out = out;
  int chunks = cdiv(n, RAD_TPB);
  a.parts = chunks > RAD_MAX_PARTS ? RAD_MAX_PARTS : chunks;
  if (chunks > ZN_CHUNKS) chunks = ZN_CHUNKS;

  MMNN_HIP(hipMemsetAsync(labels, 0, (size_t)n * 4, stream));
  MMNN_HIP(hipMemsetAsync(sizes, 0, (size_t)n * 4, stream));
  MMNN_HIP(hipMemsetAsync(levels, 0, (size_t)d->max_bins * 4, stream));
  MMNN_HIP(hipMemsetAsync(w3 + Z.keys, 0, Z.kown - Z.keys, stream));
  MMNN_HIP(hipMemsetAsync(w3 + Z.kown, 0xFF, Z.part - Z.kown, stream));
  MMNN_LAUNCH(zones_init_kernel, dim3(chunks), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(zones_link_kernel, dim3(chunks), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(zones_label_kernel, dim3(chunks), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(zones_insert_kernel, dim3(chunks), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(zones_marginal_kernel, dim3(cdiv(Z.kslots, RAD_TPB) > ZN_CHUNKS ? ZN_CHUNKS : cdiv(Z.kslots, RAD_TPB)), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(zones_features_kernel, dim3(a.parts), dim3(RAD_TPB), 0, stream, a);
  MMNN_LAUNCH(zones_final_kernel, dim3(1), dim3(RAD_TPB), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
