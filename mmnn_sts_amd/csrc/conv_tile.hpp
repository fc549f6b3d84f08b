// Building blocks of the fp32-MFMA convolution family: fprop_kernel (fprop.hpp), conv1_dgrad_resident_kernel (conv1_dgrad.hip), the
// epilogue of conv3_dgrad_bf16x3_kernel (conv3_bf16x3.hip).  Their numerical contract -- the order of the sums, the mask formula, the fp64
// atomics -- is stated HERE, once: a kernel that calls these computes fprop_kernel's bits by construction (floating-point contraction is
// off: a sum written the same way is the same sum).  Included by fprop.hpp behind FpropArgs.
#pragma once

namespace mmnn {

// Cross-workgroup K-split hand-off (fprop_kernel, "cross-block K-split").  0: the fence-free form measured valid on gfx950 / ROCm 7.2
// (MI355X_MICROARCH.md, inter-workgroup visibility, table row "ONE lane of each storing workgroup ... an agent-scope atomic add / the
// workgroup whose add came last"): partial tiles leave with write-through `sc1` stores, every storing wave drains `vmcnt(0)`, a workgroup
// barrier, ONE lane's agent-scope ticket; the last arriver reads them with `sc1` loads behind a workgroup barrier.  That is a property of
// this chip's cache policy, not of the HIP memory model, so it is the default ONLY for gfx950; any other target -- or -DMMNN_KZ_FENCED=1
// (`MMNN_KZ_FENCED=1 python -m mmnn_sts_amd.build` builds libmmnn_sts_fenced.so) -- gets the portable form: plain stores, an agent-scope
// RELEASE fence before the ticket, an agent-scope ACQUIRE fence in every reading wave after it.  tests/test_kz_handoff_gpu.py stresses
// whichever library is loaded; tests/test_host_cpu.py::test_kz_handoff_isa checks that the emitted gfx950 code really carries `sc1`.
#if !defined(MMNN_KZ_FENCED)
#if defined(__gfx950__) || !defined(__HIP_DEVICE_COMPILE__)
#define MMNN_KZ_FENCED 0
#else
#define MMNN_KZ_FENCED 1
#endif
#endif

#if defined(__HIPCC__)

// ---- tile-local voxel index -> position ------------------------------------------------------------------------------------------
// Origin of a workgroup's voxel tile: (d0, h0, w0) for the 3x3x3 kernels, the linear voxel v0 for the 1x1x1 kernels.
struct TileAt { int d0, h0, w0, v0; };

// Voxel t of a TD x TH x TW tile, W fastest.
template <int TH, int TW>
__device__ __forceinline__ void tile_local(int t, int& wx, int& hy, int& dz) {
  wx = t % TW, hy = (t / TW) % TH, dz = t / (TW * TH);
}

// Global voxel of tile-local index t, and whether it lies inside the volume (`vox` of a voxel outside is not to be used as an address).
template <int TAPS, int TD, int TH, int TW>
__device__ __forceinline__ bool tile_voxel(const TileAt& o, int D, int H, int W, int V, int t, int& vox) {
  if (TAPS == 27) {
    int wx, hy, dz;
    tile_local<TH, TW>(t, wx, hy, dz);
    const int d = o.d0 + dz, h = o.h0 + hy, w = o.w0 + wx;
    vox = (d * H + h) * W + w;
    return d < D && h < H && w < W;
  }
  vox = o.v0 + t;
  return vox < V;
}

// The same index as a position in the staged activation tile: rows of RS floats with the interior at column 4 (the tap offset adds
// -1 .. +1, hence + 3), HS rows per plane.  1x1x1: the tile is staged as it lies.
template <int TAPS, int TH, int TW, int HS, int RS>
__device__ __forceinline__ int tile_lds_pos(int t) {
  if (TAPS == 27) {
    int wx, hy, dz;
    tile_local<TH, TW>(t, wx, hy, dz);
    return (dz * HS + hy) * RS + wx + 3;
  }
  return t;
}

// ---- ReLU-mask element of the data-gradient epilogues ------------------------------------------------------------------------------
// x: the pre-activation tensor's element, val: the convolution's; (ea, eb) the affine form of the norm in front of the ReLU, (mu, rs) its
// mean and reciprocal deviation.  z = val where the ReLU was on; xh = xhat, the factor of z in the dgamma sum.
__device__ __forceinline__ void mask_elem(float ea, float eb, float mu, float rs, float x, float val, float& z, float& xh) {
  const float pre = fmaf(ea, x, eb);
  z = pre > 0.f ? val : 0.f;
  xh = (x - mu) * rs;
}

// ---- per-row epilogue coefficients ------------------------------------------------------------------------------------------------
// One row of the table [a, b, mean, rstd, gamma, dropscale][STRIDE] in LDS (conv1_dgrad.hip keeps the first five).  `e` = &table[row].
template <int STRIDE>
struct EpiRow {
  float* e;
  __device__ __forceinline__ float a() const { return e[0]; }
  __device__ __forceinline__ float b() const { return e[STRIDE]; }
  __device__ __forceinline__ float mean() const { return e[2 * STRIDE]; }
  __device__ __forceinline__ float rstd() const { return e[3 * STRIDE]; }
  __device__ __forceinline__ float gamma() const { return e[4 * STRIDE]; }
  __device__ __forceinline__ float dropscale() const { return e[5 * STRIDE]; }
  __device__ __forceinline__ void put(float ea, float eb, float mu, float rs, float g) const {
    e[0] = ea; e[STRIDE] = eb; e[2 * STRIDE] = mu; e[3 * STRIDE] = rs; e[4 * STRIDE] = g;
  }
  __device__ __forceinline__ void put_dropscale(float ds) const { e[5 * STRIDE] = ds; }
  // fast: from the statistics that bn_fwd_issue loaded into `raw` (row clamped there); else loads and arithmetic in one go, row m of the
  // statistics.  A row past the tensor's last one, or of an epilogue without a mask (!valid), is zero.
  __device__ __forceinline__ void fill(bool fast, const BnFwd& s, BnFwdRaw& raw, int m, bool valid) const {
    float ea = 0.f, eb = 0.f, mu = 0.f, rs = 0.f, g = 0.f;
    if (valid && fast) { bn_fwd_finish(s, raw, ea, eb, mu, rs); g = raw.g; }
    if (valid && !fast) { bn_fwd_coef(s, m, ea, eb, mu, rs); g = s.gamma[m]; }
    put(ea, eb, mu, rs, g);
  }
};

// ---- per-channel prologue coefficients (pro_apply reads them): rows [cpad] of `coef`, zero for a padding channel (!ok).  fast: from the
// statistics that bn_fwd_issue / bn_bwd_issue loaded into `raw` (c clamped there); else loads and arithmetic in one go. ----
// PRO_BNRELU: a, b of ReLU(a x + b)
__device__ __forceinline__ void pro_coef(float* coef, int cpad, int c, bool ok, bool fast, const BnFwd& s, BnFwdRaw& raw) {
  float ca = 0.f, cb = 0.f, mu, rs;
  if (fast) bn_fwd_finish(s, raw, ca, cb, mu, rs);
  else if (ok) bn_fwd_coef(s, c, ca, cb, mu, rs);
  coef[c] = ok ? ca : 0.f; coef[cpad + c] = ok ? cb : 0.f;
}
// PRO_GRAD: p, q, r of BN-backward p G + q X + r, times sc, the channel-dropout scale of (n, c)
__device__ __forceinline__ void pro_coef(float* coef, int cpad, int c, bool ok, bool fast, const BnBwd& s, BnBwdRaw& raw, float sc) {
  float p = 0.f, q = 0.f, r = 0.f;
  if (fast) bn_bwd_finish(s, raw, p, q, r);
  else if (ok) bn_bwd_coef(s, c, p, q, r);
  coef[c] = ok ? p * sc : 0.f; coef[cpad + c] = ok ? q * sc : 0.f; coef[2 * cpad + c] = ok ? r * sc : 0.f;
}

// ---- cross-workgroup K-split hand-off (see MMNN_KZ_FENCED above) -------------------------------------------------------------------
__device__ __forceinline__ void kz_store(float* dst, float v) {
#if MMNN_KZ_FENCED
  *dst = v;
#else
  __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // global_store_dword ... sc1
#endif
}
__device__ __forceinline__ float kz_load(const float* src) {
#if MMNN_KZ_FENCED
  return *src;
#else
  return __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // global_load_dword ... sc1
#endif
}

// Partial tiles of one (voxel, row) tile: [kz slices][nslot accumulator tiles][16 rows][64 lanes] floats.  Rows row0 .. row0 + RP - 1 of
// tile `slot`, slice z, this lane's elements (v[q]: a register array or an accumulator vector).
template <int RP, class T>
__device__ __forceinline__ void kz_publish_rows(float* part, int nslot, int slot, int row0, int lane, int z, const T& v) {
#pragma unroll
  for (int q = 0; q < RP; ++q) kz_store(part + (((long)z * nslot + slot) * 16 + row0 + q) * 64 + lane, v[q]);
}

// Called by EVERY thread of the workgroup once its kz_store()s are issued; true in the workgroup whose ticket came last of the tile's
// `kz` (workgroup-uniform: the others are done and return).  No spinning.  Hand-off without fences (MI355X_MICROARCH.md, inter-workgroup
// visibility, "valid forms"): every partial is written with write-through (`sc1`) stores, drained with vmcnt(0) before the workgroup's
// agent-scope ticket; the last arriver reads the partials with `sc1` loads, which bypass its own XCD's L2.  An agent-scope release fence
// instead writes back the XCD's whole dirty L2 -- 3-6 us per kernel in the phase trace, as long as the K loop of the 8^3 / 4^3 layers
// itself.  `cnt`: the tile's arrival counter (zero on entry, zero again on exit), `ticket`: a word of LDS, `after`: called by every
// thread behind the second barrier (the kernel's phase stamp).
template <class After>
__device__ __forceinline__ bool kz_arrive(unsigned* cnt, int kz, unsigned* ticket, int tid, After after) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every storing wave drains its stores before the barrier
  __syncthreads();
  if (tid == 0) {
#if MMNN_KZ_FENCED
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // cumulative over the barrier: publishes the whole workgroup's stores
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the compiler may drop the wait after buffer_wbl2: MI355X_MICROARCH.md, compiler hazard)
#endif
    *ticket = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  after();
  const unsigned arrived = *ticket;
  if (arrived != (unsigned)(kz - 1)) return false;       // not the last slice of this tile
  // Ready for the next launch: nobody else touches this tile's counter any more in THIS launch (all kz slices have arrived), and the
  // kernel boundary orders the store before the next launch's first add.
  if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#if MMNN_KZ_FENCED
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");     // every reading wave: drops this CU's stale L1 lines of the partial tiles
#endif
  return true;
}

// out[q] = sum over the kz slices, in slice order from zero, of row `row0 + q` of accumulator tile `slot` (NSLOT tiles of 16 x 64 floats
// per slice), this lane's element.  ZB slices' loads are in flight at once (slices past kz re-read the last one and add an exact zero):
// one memory round trip per ZB slices instead of one per slice.
template <int RP, int ZB = (RP <= 4) ? 8 : 4>   // slices in flight: at most 32 loads per lane
__device__ __forceinline__ void kz_sum_slices(const float* part, int nslot, int slot, int row0, int lane, int kz, float (&out)[RP]) {
#pragma unroll
  for (int q = 0; q < RP; ++q) out[q] = 0.f;
  for (int z0 = 0; z0 < kz; z0 += ZB) {
    float pz[ZB][RP];
#pragma unroll
    for (int z = 0; z < ZB; ++z) {
      const int zc = min(z0 + z, kz - 1);
#pragma unroll
      for (int q = 0; q < RP; ++q) pz[z][q] = kz_load(part + (((long)zc * nslot + slot) * 16 + row0 + q) * 64 + lane);
    }
#pragma unroll
    for (int z = 0; z < ZB; ++z)
#pragma unroll
      for (int q = 0; q < RP; ++q) out[q] += (z0 + z < kz) ? pz[z][q] : 0.f;
  }
}

// ---- row sums ---------------------------------------------------------------------------------------------------------------------
// 16-byte epilogue: a row's 32 voxels lie in the 8 lanes lane ^ 1, ^ 2, ^ 4, four each, already summed within the lane.  Both sums
// together, lane ^ 1 first; every lane of the eight ends with the totals.
__device__ __forceinline__ void quad_row_sum(float& r0, float& r1) {
  r0 += swz_xor<1>(r0); r1 += swz_xor<1>(r1);
  r0 += swz_xor<2>(r0); r1 += swz_xor<2>(r1);
  r0 += swz_xor<4>(r0); r1 += swz_xor<4>(r1);
}

// One output row's sums leave the workgroup: its WN per-wave partials (red0[j * stride], red1[j * stride]: one writer per slot, no LDS
// atomics -- reproducible) are added in fp64 in wave order from zero, then one fp64 atomic per sum onto replica `rep`.  EPI_STORE_STATS:
// sum / sum of squares for the consumer's batch statistics.  Mask epilogues: dbeta / dgamma, and (EPI_MASK_ACCUM) gamma times each onto
// the S1 / S2 sums of the tensor the gradient accumulates into.  `m`: the row in the tensor, `gamma`: read by EPI_MASK_ACCUM only.
template <int EPI, int WN>
__device__ __forceinline__ void flush_row_sums(const FpropArgs& a, int rep, int m, const float* red0, const float* red1, int stride, float gamma) {
  double v0d = 0.0, v1d = 0.0;
#pragma unroll
  for (int j = 0; j < WN; ++j) { v0d += (double)red0[j * stride]; v1d += (double)red1[j * stride]; }
  if (EPI == EPI_STORE_STATS) {
    atomicAdd(a.st_out.sum + (long)rep * a.st_out.stride + a.st_out.off + m, v0d);
    atomicAdd(a.st_out.sq + (long)rep * a.st_out.stride + a.st_out.off + m, v1d);
  } else {
    atomicAdd(a.dbeta + (long)rep * a.M + m, v0d);
    atomicAdd(a.dgamma + (long)rep * a.M + m, v1d);
    if (EPI == EPI_MASK_ACCUM) {
      const double g = (double)gamma;
      atomicAdd(a.s_acc.sum + (long)rep * a.s_acc.stride + a.s_acc.off + m, g * v0d);
      atomicAdd(a.s_acc.sq + (long)rep * a.s_acc.stride + a.s_acc.off + m, g * v1d);
    }
  }
}

// ---- next-launch weight prefetch (FpropArgs::pf_ptr) --------------------------------------------------------------------------------
// One dword per 128-byte line of the NEXT launch's weights, at most two lines per thread, addresses clamped instead of guarded
// and the values consumed only at the very end of the kernel (prefetch_sink): nothing ever waits for these loads.  Issue them after the
// first chunk's loads and the coefficient loads (memory returns in order: a cold weight line ahead of them would hold them back).
// `lin`: the workgroup's place in dispatch order (XCD = lin & 7) of `nblocks`.
__device__ __forceinline__ void prefetch_weight_lines(const FpropArgs& a, unsigned lin, unsigned nblocks, unsigned nthreads, unsigned tid, float& s0, float& s1) {
  const unsigned lines = a.pf_bytes >> 7;
  if (a.pf_ptr == nullptr || lines == 0) return;
  const unsigned per_xcd = (nblocks + 7u) >> 3;
  const unsigned ln0 = (lin >> 3) * nthreads + tid, ln1 = ln0 + per_xcd * nthreads;
  s0 = a.pf_ptr[(size_t)min(ln0, lines - 1) * 32];
  s1 = a.pf_ptr[(size_t)min(ln1, lines - 1) * 32];
}
__device__ __forceinline__ void prefetch_sink(const FpropArgs& a, float s0, float s1) {
  if (s0 + s1 == 1.2345678e-33f) a.out[0] = s0;     // never true in practice: the prefetched values are not used
}

#endif  // __HIPCC__
}  // namespace mmnn
