// Building blocks of the weight-gradient family: wgrad3_body / wgrad1_body (wgrad.hpp) and stem_wgrad_kernel (stem.hip).  All three compute
//
//     dW[m][j] = sum over voxels k of  dOut[m][k] * f(in)[j][k],      dOut = BN-backward(G, X) = p G + q X + r  (pro_elem<PRO_GRAD>)
//
// into per-split slabs.  Their numerical contract is stated HERE, once (floating-point contraction is off: a sum written the same way is
// the same sum): a block walks the tiles [begin, end) of split_range in ascending order; inside a tile mfma_ksteps adds k-step after
// k-step, lanes 0-31 voxel s and lanes 32-63 voxel s + 32 of each step, onto ONE accumulator chain per (A tile, B tile) pair that is never
// reset between tiles; a padding row, channel or voxel is staged as an exact zero; the dropout scale of sample n multiplies p, q, r
// (rescale_rows / rescale_row) before they meet G and X, and is refreshed when a block's range crosses into the next sample.
#pragma once
#include "fprop.hpp"   // Pro, pro_apply, pro_coef (conv_tile.hpp)

namespace mmnn {
#if defined(__HIPCC__)

// Pointers read from a device-resident argument table (the batched kernels) are "generic" to the compiler, and every access
// through them becomes a FLAT instruction -- which counts on the LDS counter (lgkmcnt) as well as on vmcnt, so a wait for an LDS
// operand inside the MFMA loop also waits for the global loads in flight.  The tile loops therefore load through pointers that
// are explicitly in the global address space (kernel arguments passed by value get this automatically).
#define MMNN_GLOBAL __attribute__((address_space(1)))
typedef const MMNN_GLOBAL float* gcf;
// ldg(base, off): base + a 32-bit BYTE offset, `global_load_dword v, v_off, s[base]` when base is wave-uniform.  A function object, declared
// where it is used (`const Ldg ldg;`): called as a free function, stem_wgrad_kernel's per-item offsets end up in scratch memory (32 bytes per
// lane in the gfx950 code object) instead of registers.
struct Ldg {
  __device__ __forceinline__ float operator()(gcf base, unsigned byte_off) const { return *(gcf)((const MMNN_GLOBAL char*)base + byte_off); }
};

// ---- the k-step loop ---------------------------------------------------------------------------------------------------------------
// STEPS k-steps (two voxels each) of v_mfma_f32_32x32x2_f32 over NA A tiles x NB B tiles: acc[i * NB + j] += A_i(s) x B_j(s), s ascending,
// one chain per accumulator.  rd_a(s, av) / rd_b(s, bv) read step s's operands from LDS; the reads of step s + 1 are issued before the MFMAs
// of step s (two register sets), the operand with the single tile first.  The sched_group_barrier pairs pin that order: NA + NB DS reads,
// then NA * NB MFMAs.  filler(s) is called once per k-step, after the MFMAs of step s: the caller's staging work for the NEXT tile issues
// in the shadow of this wave's own MFMAs -- the matrix pipe is busy 64 cycles per instruction, an in-order wave has nothing else to issue
// meanwhile.  Accumulators are passed by reference so that they stay in registers in every instantiation.
template <int STEPS, int NA, int NB, int NACC, class RdA, class RdB, class F>
__device__ __forceinline__ void mfma_ksteps(f32x16 (&acc)[NACC], RdA&& rd_a, RdB&& rd_b, F&& filler) {
  static_assert(STEPS % 2 == 0 && NA * NB <= NACC && (NA == 1 || NB == 1), "mfma_ksteps: even step count, one operand with a single tile");
  float a0[NA], a1[NA], b0[NB], b1[NB];
  auto rd = [&](int s, float (&av)[NA], float (&bv)[NB]) {
    if (NA == 1) { rd_a(s, av); rd_b(s, bv); } else { rd_b(s, bv); rd_a(s, av); }
  };
  auto mm = [&](const float (&av)[NA], const float (&bv)[NB]) {
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[i * NB + j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i * NB + j], 0, 0, 0);
  };
  rd(0, a0, b0);
#pragma unroll
  for (int s = 0; s < STEPS; s += 2) {
    rd(s + 1, a1, b1);
    __builtin_amdgcn_sched_group_barrier(0x100, NA + NB, 0);
    mm(a0, b0);
    __builtin_amdgcn_sched_group_barrier(0x008, NA * NB, 0);
    filler(s);
    if (s + 2 < STEPS) rd(s + 2, a0, b0);
    __builtin_amdgcn_sched_group_barrier(0x100, NA + NB, 0);
    mm(a1, b1);
    __builtin_amdgcn_sched_group_barrier(0x008, NA * NB, 0);
    filler(s + 1);
  }
}
struct NoFiller { __device__ __forceinline__ void operator()(int) const {} };

// ---- prologue element and its coefficient tables ------------------------------------------------------------------------------------
// pro_apply (fprop.hpp) with the coefficients already in registers (the pipelined 3x3x3 staging keeps them there): PRO_BNRELU
// max(c0 x0 + c1, 0), PRO_GRAD c0 x0 + (c1 x1 + c2) -- the inner fma first --, PRO_NONE x0.
template <int PRO>
__device__ __forceinline__ float pro_elem(float c0, float c1, float c2, float x0, float x1) {
  if (PRO == PRO_BNRELU) return fmaxf(fmaf(c0, x0, c1), 0.f);
  if (PRO == PRO_GRAD) return fmaf(c0, x0, fmaf(c1, x1, c2));
  return x0;
}

// pro_coef (conv_tile.hpp) indexes its table by the channel; the weight-gradient tables are indexed by the block-local row `row` of
// channel c = first channel of the block + row, so the table is entered at row - c.  Statistics loaded and reduced in one go (fast = false).
// PRO_BNRELU rows [a, b][stride]; zero for a channel past the tensor's last one or a PRO_NONE operand (!ok).
__device__ __forceinline__ void pro_coef_row(float* table, int stride, int row, int c, bool ok, const BnFwd& s) {
  BnFwdRaw raw;
  pro_coef(table + (row - c), stride, c, ok, false, s, raw);
}
// PRO_GRAD rows [p, q, r][stride] BEFORE the dropout scale (sc = 1: p * 1.f is p)
__device__ __forceinline__ void pro_coef_row(float* table, int stride, int row, int c, bool ok, const BnBwd& s) {
  BnBwdRaw raw;
  pro_coef(table + (row - c), stride, c, ok, false, s, raw, 1.f);
}

// Channel dropout: sample n's p, q, r of one dOut row = the unscaled ones times sc = drop_scale(drop, n, channel of the row).
__device__ __forceinline__ void rescale_row(float sc, float bp, float bq, float br, float& p, float& q, float& r) {
  p = bp * sc; q = bq * sc; r = br * sc;
}
// The same for `rows` rows of the LDS tables [p, q, r][rows], row m = channel row0 + m, dealt over the block's nthreads threads.  No barrier
// in here: the caller separates it from the readers of `scaled` before it and from its own reads after it.
__device__ __forceinline__ void rescale_rows(const float* base, float* scaled, int rows, int row0, int n, const DropCfg& drop, int tid, int nthreads) {
  for (int m = tid; m < rows; m += nthreads)
    rescale_row(drop_scale(drop, n, row0 + m), base[m], base[rows + m], base[2 * rows + m], scaled[m], scaled[rows + m], scaled[2 * rows + m]);
}

// ---- tile walk, split range, slab store ----------------------------------------------------------------------------------------------
// Split `split` of nsplit owns the tiles (1x1x1: 64-voxel chunks) [begin, end) of `total`, samples outermost: contiguous, in ascending order.
__device__ __forceinline__ void split_range(int total, int split, int nsplit, int& begin, int& end) {
  begin = (int)((long)total * split / nsplit); end = (int)((long)total * (split + 1) / nsplit);
}

// TD x TH x TW tiles over a D x H x W volume, linear tile index W fastest, then H, D, sample.
template <int TD, int TH, int TW>
struct TileGrid {
  int nw, nh, nd;
  __device__ __forceinline__ TileGrid(int D, int H, int W) : nw((W + TW - 1) / TW), nh((H + TH - 1) / TH), nd((D + TD - 1) / TD) {}
  __device__ __forceinline__ int per_sample() const { return nw * nh * nd; }
  __device__ __forceinline__ void origin(int tile, int& n, int& d0, int& h0, int& w0) const {
    int b = tile;
    w0 = (b % nw) * TW; b /= nw;
    h0 = (b % nh) * TH; b /= nh;
    d0 = (b % nd) * TD; b /= nd;
    n = b;
  }
};

// One 32 x 32 accumulator tile into a slab: register r is row row0 + acc_row(r, half); dst[row * ld] for the rows below M, where dst
// already points at this lane's column (col_ok: the column exists).  One writer per word, no atomics: the finaliser sums the slabs.
__device__ __forceinline__ void store_acc_tile(const f32x16& acc, float* dst, long ld, int row0, int M, int half, bool col_ok) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = row0 + acc_row(r, half);
    if (m < M && col_ok) dst[(long)m * ld] = acc[r];
  }
}

// ---- phase trace (developer builds, MMNN_PHASE_TRACE; tools/phase_trace.py) ----------------------------------------------------------
// Shader-clock time between successive lap(k) calls of ONE thread, summed per k over the block's tiles; finish() writes the sums to words
// 0-5 of the block's 16-word record, the tile count to word 6 and the launch's tag / grid to words 10 / 11.  Empty when the macro is off.
struct PhaseTrace {
#if defined(MMNN_PHASE_TRACE)
  bool on;
  unsigned long long tr[6] = {0, 0, 0, 0, 0, 0}, tprev;
  __device__ __forceinline__ PhaseTrace(bool on_) : on(on_), tprev(on_ ? __builtin_amdgcn_s_memtime() : 0) {}
  __device__ __forceinline__ void lap(int k) { if (on) { const unsigned long long t = __builtin_amdgcn_s_memtime(); tr[k] += t - tprev; tprev = t; } }
  __device__ __forceinline__ void finish(unsigned long long* trace, int split, int taps, int M, int Cin, int count) const {
    if (!on) return;
    for (int k = 0; k < 6; ++k) trace[split * 16 + k] = tr[k];
    trace[split * 16 + 6] = (unsigned long long)count;
    trace[10] = ((unsigned long long)taps << 48) | (9ull << 40) | ((unsigned long long)M << 16) | (unsigned long long)Cin;
    trace[11] = ((unsigned long long)gridDim.x << 32) | ((unsigned long long)gridDim.y << 16) | gridDim.z;
  }
#else
  __device__ __forceinline__ PhaseTrace(bool) {}
  __device__ __forceinline__ void lap(int) {}
  __device__ __forceinline__ void finish(unsigned long long*, int, int, int, int, int) const {}
#endif
};

#endif  // __HIPCC__
}  // namespace mmnn
