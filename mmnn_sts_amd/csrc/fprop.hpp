// Implicit-GEMM "forward-shaped" convolution on fp32 MFMA for NCDHW tensors (stride 1, "same" padding).
//
//     out[n][m][v] = sum_{c < Cin} sum_{tap < TAPS}  w[(c*TAPS + tap)][m] * f(in[n][c][v + off(tap)])
//
// TAPS = 1 (1x1x1) or 27 (3x3x3).  One kernel template serves four reference ops (models/densenet.py:76-82 and
// their autograd adjoints, main.py:469):
//   conv1 forward   : f = ReLU(BN(x))        (PRO_BNRELU)  epilogue: store + batch statistics      (EPI_STORE_STATS)
//   conv2 forward   : same, 27 taps, zero padding applied AFTER BN+ReLU
//   conv2 data-grad : f = BN-backward(G, Y)   (PRO_GRAD)    epilogue: ReLU mask, dgamma/dbeta sums  (EPI_MASK_STORE)
//   conv1 data-grad : f = BN-backward(dZ, T)  (PRO_GRAD)    epilogue: ReLU mask, G += gamma*z, sums (EPI_MASK_ACCUM)
//
// MFMA mapping (v_mfma_f32_32x32x2_f32): A = weights (i = output row m, k = input channel parity), B = activations
// (k = channel parity, j = voxel), so the 32 lanes of a half read 32 CONSECUTIVE voxels of one channel from LDS
// (conflict-free ds_read_b32) and the accumulator tile comes out as rows = m, lanes = voxels: every store
// instruction writes 128-byte runs of one output channel.  Lanes 0-31 take channel 2k, lanes 32-63 channel 2k+1.
#pragma once
#include "common.hpp"

namespace mmnn {

enum Pro { PRO_NONE = 0, PRO_BNRELU = 1, PRO_GRAD = 2 };
enum Epi { EPI_STORE = 0, EPI_STORE_STATS = 1, EPI_MASK_STORE = 2, EPI_MASK_ACCUM = 3 };

struct FpropArgs {
  int N, D, H, W;
  int Cin, M;
  const float* in0; long in0_ns; int in0_coff;   // in0[n*in0_ns + (in0_coff + c)*V + v]
  const float* in1; long in1_ns; int in1_coff;   // PRO_GRAD: the normalised tensor (in0 is its upstream G)
  BnFwd bn_in;
  BnBwd gr_in;
  DropCfg drop_in;
  const float* w; int w_ld;                      // w[(c*TAPS + tap)*w_ld + m]
  float* out; long out_ns; int out_coff;
  DropCfg drop_out;
  StatPtr st_out;
  const float* ex; long ex_ns; int ex_coff;
  BnFwd ebn;
  double* dgamma; double* dbeta;                 // [NREP][M]
  StatPtr s_acc;
  int nrep;                                      // replicas this launch's epilogue spreads its fp64 atomics over (0: NREP); see StatPtr::nrep
  int conv1_dgrad_resident;                      // plan option of the same name (conv1_dgrad.hip): 0 never, 1 where it measured faster, 2 wherever it can run
  // cross-block K-split (gridDim.z slices of the channel axis): partial tiles + per-tile arrival counters (zero on entry)
  float* kz_part; unsigned* kz_cnt;
  size_t kz_part_bytes; unsigned kz_cnt_entries;   // capacity of kz_part / kz_cnt as provided by the caller (the split is skipped when it would not fit)
  // Weights of the NEXT launch on this stream (may be null): every layer's weights are read exactly once per pass, i.e. always
  // cold, and the first chunk's weight load is the longest single wait of the small-extent kernels.  Each XCD's workgroups touch
  // one dword per 128-byte line of [pf_ptr, pf_ptr + pf_bytes) while their own first chunk is in flight, which pulls the range
  // into that XCD's L2 before the next kernel starts.
  const float* pf_ptr; unsigned pf_bytes;
  // Three-piece bf16 kernels only (conv3_bf16x3.hip, bf16x3.hpp): the pre-split weight panel (pack kind 5 / 6, replaces `w` there) and
  // the scratch its split pass writes the operand planes to, [3][N][Cin/8][V] 16-byte entries, `x3_bytes` long.  Null everywhere else.
  const void* w3; void* x3; size_t x3_bytes;
  // Filled in by launch_cfg (callers leave them zero): ceil(2^32 / d) for the divisors of the workgroup -> tile decomposition
  // (3x3x3: tiles along W, H, D; 1x1x1: tiles per sample), 0 when d == 1.  q = mulhi(b, magic) is exact for b * d < 2^32 and is two
  // scalar instructions; the compiler's sequence for a run-time divisor is ~25 dependent ones, three times over, ahead of the first load.
  unsigned mg_w, mg_h, mg_d;
  // developer aid (tools/phase_trace.py): when non-null, thread 0 of the first 64 blocks of the launch stores shader-clock stamps
  // of its phases to trace[block * 16 + k]; null in normal operation
  unsigned long long* trace;
};

int launch_fprop(const FpropArgs& a, int taps, int pro, int epi, hipStream_t stream);
// conv3_bf16x3.hip: which conv2 launches run on the three-piece bf16 kernels (they need FpropArgs::w3 / x3), and the plane scratch they need
bool conv3_fwd_bf16x3_eligible(const FpropArgs& a);
bool conv3_dgrad_bf16x3_eligible(const FpropArgs& a);
size_t conv3_bf16x3_plane_bytes(const FpropArgs& a);
// conv1_dgrad.hip: the dense-layer conv1 data gradient (1x1x1, PRO_GRAD, EPI_MASK_ACCUM) with the normalised operand tile resident in LDS
bool conv1_dgrad_resident_shape_ok(int mode, int N, long V, int Cin, int M, int w_ld);
bool conv1_dgrad_resident_eligible(const FpropArgs& a);
int launch_conv1_dgrad_resident(const FpropArgs& a, hipStream_t stream);

}  // namespace mmnn

#include "conv_tile.hpp"   // the building blocks of the kernels below and of their siblings (they take FpropArgs)

namespace mmnn {
#if defined(__HIPCC__)

template <int TAPS, int PRO, int EPI, int WM, int WN, int KS, int MT, int NT, int KC, int TD, int TH, int TW, bool SPEC = false>
struct FpropCfg {
  static constexpr int NWAVES = WM * WN * KS;          // KS wave groups split the channel (reduction) axis of every chunk
  // SPEC: wave specialisation -- a second set of NWAVES "loader" waves stages chunk k+1 into the other LDS buffer while
  // the compute waves run the MFMAs of chunk k (one loader + one compute wave per SIMD: VALU/LDS-write beside the matrix pipe)
  static constexpr int NCOMPUTE = NWAVES * 64;
  static constexpr int NTHREADS = NCOMPUTE * (SPEC ? 2 : 1);
  static constexpr int M_B = WM * MT * 32;
  static constexpr int V_B = WN * NT * 32;
  static constexpr int RS = (TAPS == 27) ? TW + 8 : TW;
  static constexpr int HS = (TAPS == 27) ? TH + 2 : 1;
  static constexpr int DS = (TAPS == 27) ? TD + 2 : 1;
  static constexpr int XS = DS * HS * RS;
  static constexpr int NCOEF = (PRO == PRO_BNRELU) ? 2 : (PRO == PRO_GRAD ? 3 : 0);
  static constexpr int ECOEF = 6 + 2 * WN;   // per output row: a, b, mean, rstd, gamma, dropscale, then per-wave partial sums
  static_assert(TD * TH * TW == V_B, "tile volume must equal the block's voxel count");
  static_assert(KC % 2 == 0 && (KC / 2) % KS == 0, "channel-pair count of a chunk must be a multiple of the K-split");
  static constexpr int STAGE = KC * XS + KC * TAPS * M_B;                       // floats: activations + weights of a chunk
  // small tiles (one accumulator per wave, K split over wave groups): every group keeps 16 / KS rows of the tile from the in-block
  // reduction to the stores (fprop_kernel, "distributed tail"); all KS groups' tiles pass through LDS
  static constexpr bool DIST = (MT * NT == 1) && KS > 1 && !SPEC;
  static constexpr int REDN = (DIST ? KS : KS - 1) * WM * WN * MT * NT * 1024;   // floats: cross-group accumulator reduction
  static constexpr int BUF0 = ((SPEC ? 2 : 1) * STAGE) > REDN ? ((SPEC ? 2 : 1) * STAGE) : REDN;
  // wide mask epilogue (see fprop_kernel): one 32 x 36 float transposition tile per wave, in the staging area after the K loop
  // (forward 3x3x3 tiles with two epilogue waves -- the 16^3 layers -- measured 1.8 us slower in the wide form: direct form kept)
  static constexpr bool WIDE = (EPI == EPI_MASK_STORE || EPI == EPI_MASK_ACCUM || (EPI == EPI_STORE_STATS && !(TAPS == 27 && WM * WN > 1))) && !SPEC;
  static constexpr int TSTRIDE = 36;
  static constexpr int TRANS = WIDE ? WM * WN * 32 * TSTRIDE : 0;
  static constexpr int BUF = BUF0 > TRANS ? BUF0 : TRANS;
  static size_t smem_bytes(int Cin) {
    int cpad = ((Cin + KC - 1) / KC) * KC;
    size_t ncoef = ((size_t)NCOEF * cpad + 3) & ~(size_t)3;   // keep the staging buffers 16-byte aligned
    return sizeof(float) * (ncoef + (size_t)BUF + (size_t)ECOEF * M_B + 4);   // + arrival ticket of the cross-block K-split
  }
};

template <int PRO>
__device__ __forceinline__ float pro_apply(const float* coef, int cpad, int c, float x0, float x1) {
  if (PRO == PRO_BNRELU) return fmaxf(fmaf(coef[c], x0, coef[cpad + c]), 0.f);
  if (PRO == PRO_GRAD) return fmaf(coef[c], x0, fmaf(coef[cpad + c], x1, coef[2 * cpad + c]));
  return x0;
}

// Sum each of R (2, 4 or 8) per-lane values over the 32 lanes of a wave half (half_reduce16 for fewer registers): log2(R) exchange-and-halve
// steps, then plain butterflies.  On return every lane of a half holds the total of register index (l31 >> (5 - log2 R)).
template <int R>
__device__ __forceinline__ float half_reduce_n(const float (&v)[R], int lane) {
  static_assert(R == 2 || R == 4 || R == 8, "half_reduce_n: 2, 4 or 8 registers");
  float w[R];
#pragma unroll
  for (int r = 0; r < R; ++r) w[r] = v[r];
  if (R >= 8) {
    const bool b = lane & 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) { const float send = b ? w[r] : w[r + 4], keep = b ? w[r + 4] : w[r]; w[r] = keep + swz_xor<16>(send); }
  }
  if (R >= 4) {
    constexpr int X = (R == 8) ? 8 : 16;
    const bool b = lane & X;
#pragma unroll
    for (int r = 0; r < 2; ++r) { const float send = b ? w[r] : w[r + 2], keep = b ? w[r + 2] : w[r]; w[r] = keep + swz_xor<X>(send); }
  }
  {
    constexpr int X = (R == 8) ? 4 : (R == 4 ? 8 : 16);
    const bool b = lane & X;
    const float send = b ? w[0] : w[1], keep = b ? w[1] : w[0];
    w[0] = keep + swz_xor<X>(send);
  }
  float t = w[0];
  if (R <= 2) t += swz_xor<8>(t);
  if (R <= 4) t += swz_xor<4>(t);
  t += swz_xor<2>(t);
  t += swz_xor<1>(t);
  return t;
}

// ---- the tails of fprop_kernel: what happens to a workgroup's accumulators after the K loop, as the stages the kernel calls.  The
// members are what every tail needs of the kernel's state: the extents of the launch (by value: a bound read through the argument
// struct inside a condition keeps the compiler from flattening it), the tile (rows from m0, voxels from `at`), this lane's place in it
// (wave (wm, wn) of K-split group kg), the sample's output / mask-operand tensors, and the LDS areas: the per-row epilogue coefficients,
// the per-wave row sums ([WN][M_B] each, one writer per slot) and the staging area, free after the last barrier of the K loop. ----
template <int TAPS, int PRO, int EPI, int WM, int WN, int KS, int MT, int NT, int KC, int TD, int TH, int TW, bool SPEC>
struct FpropTail {
  using C = FpropCfg<TAPS, PRO, EPI, WM, WN, KS, MT, NT, KC, TD, TH, TW, SPEC>;
  static constexpr int M_B = C::M_B, RP = 16 / KS, NSLOT = WM * WN * MT * NT;      // RP: accumulator rows per K-split wave group
  static constexpr bool MASK = (EPI == EPI_MASK_STORE || EPI == EPI_MASK_ACCUM);
  int D, H, W, V, M;
  TileAt at;
  int m0, wm, wn, kg, half, l31, lane;
  float* outn;
  const float* exn;
  float* ecoef; float* red0; float* red1; float* Xs;
  bool want_sums;
  __device__ __forceinline__ int slot() const { return (wm * WN + wn) * MT * NT; }      // this wave's first accumulator tile
  __device__ __forceinline__ bool voxel(int idx, int& vox) const { return tile_voxel<TAPS, TD, TH, TW>(at, D, H, W, V, idx, vox); }

  // ================= distributed tail of the small tiles (r03).  One accumulator tile per wave, the K axis split over KS wave
  // groups.  The r02 tail funnelled everything through the group-0 waves: they summed (KS - 1) x 16 rows from LDS, published 16 rows,
  // summed the K-split slices and ran the whole epilogue while seven of eight waves waited (phase trace: 1.3k + 3.4k + 2.2k + 3.7k
  // cycles of a 23k-cycle 8^3 launch).  Here every group keeps 16 / KS rows of its tile from the in-block reduction through the
  // cross-workgroup hand-off to the stores; sums are taken in the same order as before (group order, then slice order). =======
  // In-block reduction: my[q] = row kg * RP + q of the wave's tile, summed over the KS groups in group order.
  __device__ __forceinline__ void dist_reduce(const f32x16& acc, float (&my)[RP]) const {
    float* rbuf = Xs;
    const int slot = this->slot();
#pragma unroll
    for (int r = 0; r < 16; ++r) rbuf[((kg * NSLOT + slot) * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RP; ++q) {
      float s = rbuf[((0 * NSLOT + slot) * 16 + kg * RP + q) * 64 + lane];
#pragma unroll
      for (int g = 1; g < KS; ++g) s += rbuf[((g * NSLOT + slot) * 16 + kg * RP + q) * 64 + lane];
      my[q] = s;
    }
  }

  // Epilogue of this wave's rows: register q holds row acc_row(kg * RP + q, half) of tile (wm, wn), voxel l31.
  __device__ __forceinline__ void dist_epilogue(const float (&my)[RP]) const {
    int vox;
    const bool vok = voxel(wn * 32 + l31, vox);
    int ml[RP]; bool ok[RP]; unsigned off[RP];
    float xe[MASK ? RP : 1], go[(EPI == EPI_MASK_ACCUM) ? RP : 1];
#pragma unroll
    for (int q = 0; q < RP; ++q) {
      ml[q] = wm * 32 + acc_row(kg * RP + q, half);
      ok[q] = vok && (m0 + ml[q]) < M;
      off[q] = ok[q] ? (unsigned)(m0 + ml[q]) * (unsigned)V + (unsigned)vox : 0u;     // unconditional loads (clamped), before any store (aliasing)
      if (MASK) xe[MASK ? q : 0] = exn[off[q]];
      if (EPI == EPI_MASK_ACCUM) go[(EPI == EPI_MASK_ACCUM) ? q : 0] = outn[off[q]];
    }
    float s0[RP], s1[RP];
#pragma unroll
    for (int q = 0; q < RP; ++q) {
      const EpiRow<M_B> e{ecoef + ml[q]};
      float val = my[q], t0 = 0.f, t1 = 0.f;
      if (EPI == EPI_STORE) {
        if (ok[q]) outn[off[q]] = val;
      } else if (EPI == EPI_STORE_STATS) {
        val *= e.dropscale();
        if (ok[q]) { outn[off[q]] = val; t0 = val; t1 = val * val; }
      } else {
        if (ok[q]) {
          float z, xh;
          mask_elem(e.a(), e.b(), e.mean(), e.rstd(), xe[MASK ? q : 0], val, z, xh);
          t0 = z; t1 = z * xh;
          if (EPI == EPI_MASK_STORE) outn[off[q]] = z;
          else outn[off[q]] = go[(EPI == EPI_MASK_ACCUM) ? q : 0] + e.gamma() * z;
        }
      }
      s0[q] = t0; s1[q] = t1;
    }
    if (want_sums) {
      const float r0 = half_reduce_n<RP>(s0, lane), r1 = half_reduce_n<RP>(s1, lane);
      constexpr int SH = (RP == 8) ? 2 : (RP == 4 ? 3 : 4);      // lanes l31 >> SH share a total: the first of each group writes it
      if ((l31 & ((1 << SH) - 1)) == 0) {
        const int mrow = wm * 32 + acc_row(kg * RP + (l31 >> SH), half);
        red0[wn * M_B + mrow] = r0;
        red1[wn * M_B + mrow] = r1;
      }
    }
  }

  // ================= cross-group reduction of the accumulators (in-block K-split): group 0 adds its partners' tiles in group order =====
  __device__ __forceinline__ void group_reduce(bool loader, f32x16 (&acc)[MT][NT]) const {
    float* rbuf = Xs;   // staging buffers are free after the last barrier
    const int slot = this->slot();
    if (kg > 0 && !loader) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) rbuf[(((kg - 1) * NSLOT + slot + i * NT + j) * 16 + r) * 64 + lane] = acc[i][j][r];
    }
    __syncthreads();
    if (kg == 0 && !loader) {
#pragma unroll
      for (int g = 1; g < KS; ++g)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] += rbuf[(((g - 1) * NSLOT + slot + i * NT + j) * 16 + r) * 64 + lane];
    }
  }

  // The last arriver of the cross-block K-split: the group-0 waves' accumulators <- the sum of all kz slices, in slice order from zero
  // (bit-reproducible).
  __device__ __forceinline__ void kz_collect(const float* part, int kz, bool loader, f32x16 (&acc)[MT][NT]) const {
    const int slot = this->slot();
    if constexpr (KS > 1) {
      // Every wave group takes 16 / KS accumulator rows of each tile and has ALL slices' loads in flight at once (slices past kz
      // re-read the last one and add an exact zero): one memory round trip instead of kz / 2 dependent ones by the group-0 waves
      // alone (phase "kz sum": 3.7k of a 27k-cycle launch at kz = 8).  Summed in slice order as before -- same bits -- and handed to
      // the epilogue waves through the staging area, which is free since the barriers above.
      float* xbuf = Xs;
      if (!loader) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            float sacc[RP];
            kz_sum_slices<RP>(part, NSLOT, slot + i * NT + j, kg * RP, lane, kz, sacc);
#pragma unroll
            for (int q = 0; q < RP; ++q) xbuf[((slot + i * NT + j) * 16 + kg * RP + q) * 64 + lane] = sacc[q];
          }
      }
      __syncthreads();
      if (kg == 0 && !loader) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = xbuf[((slot + i * NT + j) * 16 + r) * 64 + lane];
      }
    } else {
      if (kg == 0 && !loader) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
            // kz is 2, 4 or 8: two slices' loads are in flight together (one memory round trip per pair), summed in slice order
            for (int z = 0; z < kz; z += 2) {
              float p0[16], p1[16];
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                p0[r] = kz_load(part + (((long)z * NSLOT + slot + i * NT + j) * 16 + r) * 64 + lane);
                p1[r] = kz_load(part + (((long)(z + 1) * NSLOT + slot + i * NT + j) * 16 + r) * 64 + lane);
              }
#pragma unroll
              for (int r = 0; r < 16; ++r) acc[i][j][r] = (acc[i][j][r] + p0[r]) + p1[r];
            }
          }
      }
    }
  }

  // ================= epilogues of the group-0 waves =================
  // The mask epilogues read one (ex) or two (ex, out) tensors per element.  Their loads are issued BEFORE the stores: `out` may
  // alias `ex` as far as the compiler knows, so a load placed after a store is never hoisted above it and every accumulator row
  // would pay a full memory round trip of its own (phase trace r02: 34 us of a 126 us block in block 1's data gradient).  One
  // tensor (MASK_STORE): the whole tile's loads go out together; two tensors (MASK_ACCUM): one 32-row slab at a time (register
  // budget: the big tiles of block 1 must stay at two waves per SIMD).  Element offsets are 32-bit (host check: M * V < 2^31),
  // so an address costs one register beside the uniform base pointer.
  // Wide form (big tiles, 16-byte aligned tensors): an MFMA accumulator holds ONE voxel per lane and row, so the direct form below
  // moves 4 bytes per lane and instruction -- 128..192 memory instructions per thread, and the address coalescer, not HBM, bounds
  // the epilogue (phase trace r02: 33k of a block's 85k cycles in block 1's conv1 data gradient, 40k of 290k in conv2's).  Each
  // 32 x 32 accumulator tile is therefore transposed through LDS (wave-private, the staging buffers are free) so that a lane holds
  // 4 consecutive voxels of 4 rows: every global access becomes a dwordx4 -- a quarter of the memory instructions.
  __device__ __forceinline__ void epilogue_wide(const f32x16 (&acc)[MT][NT]) const {
    float* tb = Xs + (wm * WN + wn) * (32 * C::TSTRIDE);
    const int q4 = 4 * (lane & 7), rl = lane >> 3;            // this lane's voxel quad and first row within a tile
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      f32x4 vt[NT][4], xq[MASK ? NT : 1][4], gq[(EPI == EPI_MASK_ACCUM) ? NT : 1][4];
      unsigned off[NT][4];
      bool okq[NT][4];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        // voxel quad of this lane in tile j
        int vq;
        const bool vk = voxel((wn * NT + j) * 32 + q4, vq);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();        // the previous tile's reads precede these writes (LDS executes a wave's accesses in order)
#pragma unroll
        for (int r = 0; r < 16; ++r) tb[acc_row(r, half) * C::TSTRIDE + l31] = acc[i][j][r];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int ml = wm * MT * 32 + i * 32 + rl + 8 * k;
          vt[j][k] = *reinterpret_cast<const f32x4*>(tb + (rl + 8 * k) * C::TSTRIDE + q4);
          okq[j][k] = vk && (m0 + ml) < M;
          off[j][k] = okq[j][k] ? (unsigned)(m0 + ml) * (unsigned)V + (unsigned)vq : 0u;      // unconditional loads (clamped)
        }
      }
      // all loads of the slab before its stores (see the note on aliasing above)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (MASK) xq[MASK ? j : 0][k] = *reinterpret_cast<const f32x4*>(exn + off[j][k]);
          if (EPI == EPI_MASK_ACCUM) gq[(EPI == EPI_MASK_ACCUM) ? j : 0][k] = *reinterpret_cast<const f32x4*>(outn + off[j][k]);
        }
      float s0[4], s1[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ml = wm * MT * 32 + i * 32 + rl + 8 * k;
        const EpiRow<M_B> e{ecoef + ml};
        const float ea = e.a(), eb = e.b(), mu = e.mean(), rs = e.rstd(), gm = e.gamma(), ds = e.dropscale();
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          if (okq[j][k]) {
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              if (MASK) {
                float z, xh;
                mask_elem(ea, eb, mu, rs, xq[MASK ? j : 0][k][c], vt[j][k][c], z, xh);
                t0 += z;
                t1 += z * xh;
                o[c] = (EPI == EPI_MASK_STORE) ? z : gq[(EPI == EPI_MASK_ACCUM) ? j : 0][k][c] + gm * z;
              } else {     // EPI_STORE_STATS: channel dropout scale, sums for the consumer's batch statistics
                const float val = vt[j][k][c] * ds;
                t0 += val;
                t1 += val * val;
                o[c] = val;
              }
            }
            *reinterpret_cast<f32x4*>(outn + off[j][k]) = o;
          }
        }
        s0[k] = t0; s1[k] = t1;
      }
      if (want_sums) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float r0 = s0[k], r1 = s1[k];
          quad_row_sum(r0, r1);
          if ((lane & 7) == 0) {
            const int ml = wm * MT * 32 + i * 32 + rl + 8 * k;
            red0[wn * M_B + ml] = r0;
            red1[wn * M_B + ml] = r1;
          }
        }
      }
    }
  }

  // Direct form: a lane stores the one voxel per row that its accumulator registers hold.  EPI_MASK_STORE: the epilogue's operand, the
  // pre-activation tensor `ex`, is loaded for the whole tile at once.  (Loading it before the last chunk's MFMAs measured slower: its
  // registers stay live across the chunk)
  __device__ __forceinline__ void epilogue_direct(const f32x16 (&acc)[MT][NT]) const {
    constexpr bool ALL_ROWS = (EPI == EPI_MASK_STORE);
    int vox[NT];      // (computed here, not ahead of the K loop: kept live across it these cost the small-tile kernels their last registers)
    bool vok[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) vok[j] = voxel((wn * NT + j) * 32 + l31, vox[j]);
    float xall[ALL_ROWS ? MT : 1][ALL_ROWS ? 16 : 1][NT];
    if (ALL_ROWS) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int ml = wm * MT * 32 + i * 32 + acc_row(q, half);
          const bool mok = (m0 + ml) < M;
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            const unsigned o = (mok && vok[j]) ? (unsigned)(m0 + ml) * (unsigned)V + (unsigned)vox[j] : 0u;   // unconditional loads (clamped)
            xall[ALL_ROWS ? i : 0][ALL_ROWS ? q : 0][j] = exn[o];
          }
        }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float s0[16], s1[16];
      float xe[(MASK && !ALL_ROWS) ? 16 : 1][NT], go[(EPI == EPI_MASK_ACCUM) ? 16 : 1][NT];
      if (MASK && !ALL_ROWS) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int ml = wm * MT * 32 + i * 32 + acc_row(q, half);
          const bool mok = (m0 + ml) < M;
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            const unsigned o = (mok && vok[j]) ? (unsigned)(m0 + ml) * (unsigned)V + (unsigned)vox[j] : 0u;
            xe[(MASK && !ALL_ROWS) ? q : 0][j] = exn[o];
            if (EPI == EPI_MASK_ACCUM) go[(EPI == EPI_MASK_ACCUM) ? q : 0][j] = outn[o];
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ml = wm * MT * 32 + i * 32 + acc_row(r, half);
        const EpiRow<M_B> e{ecoef + ml};
        const bool mok = (m0 + ml) < M;
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const bool ok = mok && vok[j];
          const unsigned o = (unsigned)(m0 + ml) * (unsigned)V + (unsigned)vox[j];
          float val = acc[i][j][r];
          if (EPI == EPI_STORE) {
            if (ok) outn[o] = val;
          } else if (EPI == EPI_STORE_STATS) {
            val *= e.dropscale();
            if (ok) {
              outn[o] = val;
              t0 += val;
              t1 += val * val;
            }
          } else {
            if (ok) {
              float z, xh;
              mask_elem(e.a(), e.b(), e.mean(), e.rstd(), ALL_ROWS ? xall[ALL_ROWS ? i : 0][ALL_ROWS ? r : 0][j] : xe[(MASK && !ALL_ROWS) ? r : 0][j], val, z, xh);
              t0 += z;
              t1 += z * xh;
              if (EPI == EPI_MASK_STORE) outn[o] = z;
              else outn[o] = go[(EPI == EPI_MASK_ACCUM) ? r : 0][j] + e.gamma() * z;
            }
          }
        }
        s0[r] = t0;
        s1[r] = t1;
      }
      if (want_sums) {
        const float r0 = half_reduce16(s0, lane), r1 = half_reduce16(s1, lane);
        if ((lane & 1) == 0) {
          const int ml = wm * MT * 32 + i * 32 + acc_row((l31 >> 1) & 15, half);
          red0[wn * M_B + ml] = r0;
          red1[wn * M_B + ml] = r1;
        }
      }
    }
  }
};

template <int TAPS, int PRO, int EPI, int WM, int WN, int KS, int MT, int NT, int KC, int TD, int TH, int TW, bool SPEC = false>
__global__ void __launch_bounds__(WM* WN* KS * 64 * (SPEC ? 2 : 1)) fprop_kernel(const FpropArgs a) {
  using C = FpropCfg<TAPS, PRO, EPI, WM, WN, KS, MT, NT, KC, TD, TH, TW, SPEC>;
  constexpr int NL = C::NCOMPUTE;                         // threads that take part in staging (fast path)
  constexpr int NTHREADS = C::NTHREADS, M_B = C::M_B, V_B = C::V_B, RS = C::RS, HS = C::HS, DS = C::DS, XS = C::XS;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
#if defined(MMNN_PHASE_TRACE)   // developer builds only (MMNN_PHASE_TRACE=1 python -m mmnn_sts_amd.build): costs ~11 registers
  const bool tracing = a.trace != nullptr && tid == 0 && blockIdx.x < 64 && blockIdx.y == 0;
#else
  constexpr bool tracing = false;
#endif
  auto stamp = [&](int k) {
    if (tracing) a.trace[(blockIdx.x * (gridDim.z > 1 ? 2 : 1) + (blockIdx.z ? 1 : 0)) % 64 * 16 + k] = __builtin_amdgcn_s_memtime();
  };
  stamp(0);
  kernarg_warm<sizeof(FpropArgs)>();
  stamp(13);
  float pf_sink = 0.f, pf_sink2 = 0.f;                   // keep the prefetch loads alive (see FpropArgs::pf_ptr)
  const bool loader = SPEC && tid >= NL;                 // wave-uniform role
  const int ltid = loader ? tid - NL : tid;              // index within the role's thread set
  const int wave = ltid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int kg = wave / (WM * WN);                      // K-split group of this wave
  const int wm = (wave % (WM * WN)) / WN, wn = wave % WN;
  const int V = a.D * a.H * a.W;
  const int cpad = ((a.Cin + KC - 1) / KC) * KC;

  float* coef = smem;
  float* Xs = coef + ((C::NCOEF * cpad + 3) & ~3);
  float* Ws = Xs + KC * XS;                              // buffer 0; buffer 1 (SPEC) follows at + C::STAGE
  float* ecoef = Xs + C::BUF;

  // ---- which tile ----
  int n, d0 = 0, h0 = 0, w0 = 0, v0_ = 0;
  {
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (blockIdx.x & 7 = XCD), each with an L2 of its own.
    // Giving XCD x the x-th CONTIGUOUS eighth of the tile sequence makes neighbouring tiles -- which share halo rows and, for
    // the 1x1x1 kernels, nothing -- meet in the same L2 instead of each pulling the halo from HBM / the Infinity Cache again.
    int b = blockIdx.x;
    // (Applying the same order to the 1x1x1 kernels, so that producer and consumer tiles share an XCD, measured no gain: r02.)
    if (TAPS == 27 && (gridDim.x & 7) == 0) b = (b & 7) * (int)(gridDim.x >> 3) + (b >> 3);
    auto divmod = [](int& x, int d, unsigned magic) {      // x <- x / d, returns x % d
      const int q = magic ? (int)__umulhi((unsigned)x, magic) : x;
      const int r = x - q * d;
      x = q;
      return r;
    };
    if (TAPS == 27) {
      const int nw = (a.W + TW - 1) / TW, nh = (a.H + TH - 1) / TH, nd = (a.D + TD - 1) / TD;
      w0 = divmod(b, nw, a.mg_w) * TW;
      h0 = divmod(b, nh, a.mg_h) * TH;
      d0 = divmod(b, nd, a.mg_d) * TD;
      n = b;
    } else {
      const int nt = (V + V_B - 1) / V_B;
      v0_ = divmod(b, nt, a.mg_w) * V_B;
      n = b;
    }
  }
  const int m0 = blockIdx.y * M_B;
  const int rep = blockIdx.x & ((a.nrep > 0 ? a.nrep : NREP) - 1);
  // channel slice of this block (cross-block K-split): whole chunks [c_begin, c_end)
  // (kz is a power of two -- launch_cfg doubles it -- so the slice bounds are shifts: the 64-bit run-time division this used to be
  // is ~100 dependent instructions, twice, ahead of the first load of every launch)
  const int kz = gridDim.z, nch_all = (a.Cin + KC - 1) / KC;
  const int kz_sh = __builtin_ctz((unsigned)kz);
  const int c_begin = ((nch_all * (int)blockIdx.z) >> kz_sh) * KC;
  const int c_end = min(a.Cin, ((nch_all * ((int)blockIdx.z + 1)) >> kz_sh) * KC);

  // ---- small tiles: the loads the coefficients need go out FIRST (a handful per thread), the first chunks' operand loads follow,
  // and the coefficient arithmetic (prologue_fast below) runs when the statistics are back -- memory returns in order, so it no
  // longer waits behind the 50-110 KB of operands, and the operands no longer wait for it: one memory round trip where the phase
  // trace of r03 showed three (tools/phase_trace.py: "prologue" 3.6k + "1st store" 3.3k cycles of a 27k-cycle 8^3 launch). ----
  constexpr bool EARLY_K = (MT * NT == 1) || (TAPS == 27 && TW <= 16);          // the latency-bound tile shapes (see EARLY below)
  constexpr bool MASK_E = (EPI == EPI_MASK_STORE || EPI == EPI_MASK_ACCUM);
  static_assert(!EARLY_K || M_B <= NTHREADS, "one epilogue row per thread");
  const int c_hi = min(cpad, c_begin + ((c_end - c_begin + KC - 1) / KC) * KC);   // end of this slice's coefficient range
  bool fastp = EARLY_K && (c_hi - c_begin) <= NTHREADS;
  if (PRO == PRO_BNRELU) fastp = fastp && a.bn_in.training && a.bn_in.st.nrep <= 2;
  if (PRO == PRO_GRAD) fastp = fastp && a.gr_in.st.nrep <= 2 && a.gr_in.s.nrep <= 2;
  if (MASK_E) fastp = fastp && a.ebn.training && a.ebn.st.nrep <= 2;
  BnFwdRaw raw_in, raw_e;
  BnBwdRaw raw_gr;
  if (EARLY_K && fastp) {
    // Only the waves that own a channel / a row load (a slice is 16-128 channels of a 512-thread block): memory returns in order, and
    // eight waves' worth of redundant statistic loads ahead of the operand loads cost more than they hide.  Indices clamped inside a
    // wave, values of padding channels discarded in prologue_fast.
    const int pc = max(0, min(c_begin + tid, a.Cin - 1)), pm = max(0, min(m0 + tid, a.M - 1));
    if (PRO != PRO_NONE && c_begin + (tid & ~63) < c_hi) {
      if (PRO == PRO_BNRELU) bn_fwd_issue(a.bn_in, pc, raw_in);
      if (PRO == PRO_GRAD) bn_bwd_issue(a.gr_in, pc, raw_gr);
    }
    if (MASK_E && (tid & ~63) < M_B) bn_fwd_issue(a.ebn, pm, raw_e);
  }
  stamp(14);
  // one channel's prologue coefficients, one row's epilogue coefficients (`fast`: from the statistics issued above)
  auto pro_row = [&](int c, bool fast) {
    if (PRO == PRO_BNRELU) pro_coef(coef, cpad, c, c < a.Cin, fast, a.bn_in, raw_in);
    if (PRO == PRO_GRAD) pro_coef(coef, cpad, c, c < a.Cin, fast, a.gr_in, raw_gr, drop_scale(a.drop_in, n, c));
  };
  auto epi_row = [&](int m, bool fast) {
    const EpiRow<M_B> e{ecoef + m};
    const bool valid = m0 + m < a.M;
    e.fill(fast, a.ebn, raw_e, m0 + m, MASK_E && valid);
    e.put_dropscale((EPI == EPI_STORE_STATS && valid) ? drop_scale(a.drop_out, n, m0 + m) : 1.f);
  };
  auto prologue_fast = [&]() {
    if (c_begin + tid < c_hi) pro_row(c_begin + tid, true);
    if (tid < M_B) epi_row(tid, true);
    __syncthreads();
  };

  // ---- per-channel prologue coefficients, per-row epilogue coefficients.  Called AFTER the first chunk's global loads have
  // been issued (fast path): the coefficients cost a memory round trip of their own (fp64 statistics) and are only needed when
  // the chunk is written to LDS, so the two latencies overlap instead of adding up -- the small-extent layers are a chain of
  // such latencies and little else. ----
  auto prologue = [&]() {
    for (int c = c_begin + tid; c < c_hi; c += NTHREADS) pro_row(c, false);
    for (int m = tid; m < M_B; m += NTHREADS) epi_row(m, false);
    __syncthreads();
  };

  // ---- accumulators and per-lane voxel positions ----
  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int pos[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) pos[j] = tile_lds_pos<TAPS, TH, TW, HS, RS>((wn * NT + j) * 32 + l31);

  const float* in0n = a.in0 + (long)n * a.in0_ns + (long)a.in0_coff * V;
  const float* in1n = (PRO == PRO_GRAD) ? a.in1 + (long)n * a.in1_ns + (long)a.in1_coff * V : nullptr;
  const bool al_x = (((uintptr_t)in0n | (uintptr_t)in1n) & 15) == 0;
  const bool vecx = al_x && ((TAPS == 27) ? ((a.W & 3) == 0) : ((V & 3) == 0));
  const bool vecw = ((a.w_ld & 3) == 0) && ((a.M & 3) == 0) && (((uintptr_t)a.w & 15) == 0);

  // ---- MFMA over one staged chunk.  The operand reads of step s+1 are issued before the MFMAs of step s (two register
  // sets), so that the LDS latency hides behind the matrix pipe even with a single wave per SIMD. ----
  auto mfma_chunk = [&](int boff = 0) {
    const float* xb = Xs + boff + (2 * kg + half) * XS;
    const float* wb = Ws + boff + (2 * kg + half) * TAPS * M_B + wm * MT * 32 + l31;
    constexpr int PAIR = 2 * KS;                 // channel distance between consecutive pairs of one wave group
    constexpr int NSTEP = (KC / 2 / KS) * TAPS;
    auto rd = [&](int st, float (&av)[MT], float (&bv)[NT]) {
      const int jj = st / TAPS, tap = st % TAPS;
      const int toff = (TAPS == 27) ? (((tap / 9) * HS + (tap / 3) % 3) * RS + tap % 3) : 0;
#pragma unroll
      for (int i = 0; i < MT; ++i) av[i] = wb[(jj * PAIR * TAPS + tap) * M_B + i * 32];
#pragma unroll
      for (int j = 0; j < NT; ++j) bv[j] = xb[jj * PAIR * XS + pos[j] + toff];
    };
    auto mm = [&](const float (&av)[MT], const float (&bv)[NT]) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    };
    float a0[MT], b0[NT], a1[MT], b1[NT];
    rd(0, a0, b0);
#pragma unroll
    for (int st = 0; st < NSTEP; st += 2) {
      if (st + 1 < NSTEP) rd(st + 1, a1, b1);
      __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);   // DS reads of the next step first ...
      mm(a0, b0);
      __builtin_amdgcn_sched_group_barrier(0x008, MT * NT, 0);   // ... then this step's MFMAs
      if (st + 2 < NSTEP) rd(st + 2, a0, b0);
      __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);
      if (st + 1 < NSTEP) mm(a1, b1);
      __builtin_amdgcn_sched_group_barrier(0x008, MT * NT, 0);
    }
  };

  // ---- this sample's output tensor and the mask epilogues' operand, the pre-activation tensor `ex` ----
  float* outn = a.out + (long)n * a.out_ns + (long)a.out_coff * V;
  const float* exn = (EPI == EPI_MASK_STORE || EPI == EPI_MASK_ACCUM) ? a.ex + (long)n * a.ex_ns + (long)a.ex_coff * V : nullptr;

  if (vecx && vecw && (long)KC * V < (1l << 30)) {
    // ===== fast path: 16-byte staging through registers, software-pipelined.  The global loads of chunk k+1 are issued
    // (all at once) before the MFMA loop of chunk k and only waited for when they are written to LDS afterwards. =====
    constexpr int ROWS = (TAPS == 27) ? KC * DS * HS : KC;                   // staged rows (channel x halo row)
    constexpr int VPR = (TAPS == 27) ? TW / 4 : V_B / 4;                      // 16-byte items per row
    constexpr int XV_ITEMS = ROWS * VPR;
    constexpr int XH_ITEMS = (TAPS == 27) ? ROWS * 2 : 0;                     // halo columns: one float each
    constexpr int W_ITEMS = KC * TAPS * (M_B / 4);
    constexpr int XV_IT = (XV_ITEMS + NL - 1) / NL, XH_IT = (XH_ITEMS + NL - 1) / NL;
    constexpr int W_IT = (W_ITEMS + NL - 1) / NL;
    static_assert(XV_IT <= 32 && XH_IT <= 32 && W_IT <= 32, "validity bits of the staged items are kept in 32-bit masks");
    constexpr bool GR = (PRO == PRO_GRAD);
    // small tiles (one accumulator per wave) are latency-bound in this loop: keep TWO chunks of loads in flight
    constexpr int PF = (MT * NT == 1) ? 2 : 1;
    struct Stage {
      f32x4 xv0[XV_IT], xv1[GR ? XV_IT : 1], wr[W_IT];
      float xh0[XH_IT > 0 ? XH_IT : 1], xh1[(GR && XH_IT > 0) ? XH_IT : 1];
      unsigned okv, okh, okw;
    };
    Stage stA, stB;

    // Per-item descriptors, computed ONCE: element offset relative to the chunk's first channel (-1: never valid), LDS
    // destination and local channel.  The per-chunk staging code is then one add + one select per item -- with one wave per
    // SIMD every integer instruction spent here is a cycle the matrix pipe idles.
    int xv_off[XV_IT], xv_dst[XV_IT], xv_cl[XV_IT];
    int xh_off[XH_IT > 0 ? XH_IT : 1], xh_dst[XH_IT > 0 ? XH_IT : 1], xh_cl[XH_IT > 0 ? XH_IT : 1];
    int w_off[W_IT], w_cl[W_IT];
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
      const int it = ltid + i * NL;
      const int q = it % (M_B / 4), kr = it / (M_B / 4);
      const bool ok = (it < W_ITEMS) && (m0 + 4 * q < a.M);
      w_off[i] = ok ? kr * a.w_ld + m0 + 4 * q : -1;
      w_cl[i] = kr / TAPS;
    }
    const bool w_nomask = (a.Cin % KC == 0) && (m0 + M_B <= a.M);   // block-uniform: no padded channel or row in any weight chunk
    auto load_w = [&](int c0, Stage& st) {
      const int crem = a.Cin - c0;
      const float* bw = a.w + (long)c0 * TAPS * a.w_ld;
      unsigned okw = 0;
#pragma unroll
      for (int i = 0; i < W_IT; ++i) {
        const bool ok = w_off[i] >= 0 && w_cl[i] < crem;
        okw |= (ok ? 1u : 0u) << i;
        st.wr[i] = *reinterpret_cast<const f32x4*>(ok ? bw + w_off[i] : a.w);   // masked when written to LDS: a select on the
      }                                                                          // loaded value here would wait for the load
      st.okw = okw;
    };
    // Small tiles: the first chunk's weight loads go out NOW, before the activation descriptors are worked out -- that set-up
    // arithmetic is ~2 us of the small-extent kernels and now overlaps the (always cold) weight fetch.
    constexpr bool EARLY = (MT * NT == 1) || (TAPS == 27 && TW <= 16);
    const bool first_chunk_mine = (c_begin < c_end) && (!SPEC || loader);
    if (EARLY && first_chunk_mine) load_w(c_begin, stA);
    stamp(15);
    {
      // 32-bit offsets: this path is only taken when KC * V < 2^30 (64-bit multiplies cost four instructions each, and this
      // set-up runs before the first load of every launch: 2.5 us of the 8^3 / 4^3 kernels in the phase trace)
      auto row_info = [&](int r, int& cl, int& lrow, int& gro, bool& rowok) {
        if (TAPS == 27) {
          const int hy = r % HS, dz = (r / HS) % DS;
          cl = r / (HS * DS);
          const int d = d0 + dz - 1, h = h0 + hy - 1;
          rowok = (unsigned)d < (unsigned)a.D && (unsigned)h < (unsigned)a.H;
          gro = cl * V + (d * a.H + h) * a.W;
          lrow = cl * XS + (dz * HS + hy) * RS;
        } else {
          cl = r;
          rowok = true;
          gro = cl * V;
          lrow = cl * XS;
        }
      };
#pragma unroll
      for (int i = 0; i < XV_IT; ++i) {
        const int it = ltid + i * NL;
        int cl, lrow, gro; bool rowok;
        row_info(it / VPR, cl, lrow, gro, rowok);
        const int col = ((TAPS == 27) ? w0 : v0_) + 4 * (it % VPR);
        const bool ok = (it < XV_ITEMS) && rowok && col < ((TAPS == 27) ? a.W : V);
        xv_off[i] = ok ? gro + col : -1;
        xv_dst[i] = lrow + ((TAPS == 27) ? 4 : 0) + 4 * (it % VPR);
        xv_cl[i] = cl;
      }
#pragma unroll
      for (int i = 0; i < XH_IT; ++i) {
        const int it = ltid + i * NL;
        int cl, lrow, gro; bool rowok;
        row_info(it >> 1, cl, lrow, gro, rowok);
        const int w = (it & 1) ? w0 + TW : w0 - 1;
        const bool ok = (it < XH_ITEMS) && rowok && (unsigned)w < (unsigned)a.W;
        xh_off[i] = ok ? gro + w : -1;
        xh_dst[i] = lrow + ((it & 1) ? TW + 4 : 3);
        xh_cl[i] = cl;
      }
    }

    // NOTE: every load below is UNCONDITIONAL (out-of-range items read element 0 of their tensor and are zeroed when
    // they are written to LDS).  A load under a divergent `if` makes hipcc branch around it and wait vmcnt(0) at the join,
    // which serialises the whole batch (one memory round trip per item instead of one per chunk).
    auto load_x = [&](int c0, Stage& st) {
      unsigned okv = 0, okh = 0;
      const float* b0 = in0n + (long)c0 * V;
      const float* b1 = GR ? in1n + (long)c0 * V : nullptr;
      const int crem = a.Cin - c0;                    // channels left: items of local channel >= crem are padding
#pragma unroll
      for (int i = 0; i < XV_IT; ++i) {
        const bool ok = xv_off[i] >= 0 && xv_cl[i] < crem;
        const int off = ok ? xv_off[i] : 0;
        okv |= (ok ? 1u : 0u) << i;
        st.xv0[i] = *reinterpret_cast<const f32x4*>(ok ? b0 + off : in0n);
        if (GR) st.xv1[i] = *reinterpret_cast<const f32x4*>(ok ? b1 + off : in1n);
      }
#pragma unroll
      for (int i = 0; i < XH_IT; ++i) {
        const bool ok = xh_off[i] >= 0 && xh_cl[i] < crem;
        const int off = ok ? xh_off[i] : 0;
        okh |= (ok ? 1u : 0u) << i;
        st.xh0[i] = *(ok ? b0 + off : in0n);
        if (GR) st.xh1[i] = *(ok ? b1 + off : in1n);
      }
      st.okv = okv; st.okh = okh;
    };

    auto load_chunk = [&](int c0, Stage& st) { load_x(c0, st); load_w(c0, st); };
    auto load_first = [&](Stage& st) { if (EARLY) load_x(c_begin, st); else load_chunk(c_begin, st); };   // EARLY: weights already in flight

    auto store_chunk = [&](int c0, const Stage& st, int boff = 0) {
      const unsigned okv = st.okv, okh = st.okh;
#pragma unroll
      for (int i = 0; i < XV_IT; ++i) {
        if (ltid + i * NL < XV_ITEMS) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = pro_apply<PRO>(coef, cpad, c0 + xv_cl[i], st.xv0[i][e], GR ? st.xv1[i][e] : 0.f);
          if (!((okv >> i) & 1u)) o = f32x4{0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<f32x4*>(Xs + boff + xv_dst[i]) = o;
        }
      }
#pragma unroll
      for (int i = 0; i < XH_IT; ++i) {
        if (ltid + i * NL < XH_ITEMS) {
          const float o = pro_apply<PRO>(coef, cpad, c0 + xh_cl[i], st.xh0[i], GR ? st.xh1[i] : 0.f);
          Xs[boff + xh_dst[i]] = ((okh >> i) & 1u) ? o : 0.f;
        }
      }
      if (w_nomask) {   // uniform branch: the selects below are vector instructions, and those come out of the fp32 matrix rate
#pragma unroll
        for (int i = 0; i < W_IT; ++i) {
          const int it = ltid + i * NL;
          if (it < W_ITEMS) *reinterpret_cast<f32x4*>(Ws + boff + 4 * it) = st.wr[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < W_IT; ++i) {
          const int it = ltid + i * NL;
          if (it < W_ITEMS) *reinterpret_cast<f32x4*>(Ws + boff + 4 * it) = ((st.okw >> i) & 1u) ? st.wr[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    };

    // Small tiles (the 16^3 .. 4^3 layers) are latency chains: issue the first chunk's loads, THEN compute the coefficients.  The
    // big tiles of block 1 amortise the prologue over a long K loop and cannot afford the registers (staging registers live
    // across the fp64 coefficient math: 116 -> 188 VGPRs, one register short of losing the second wave per SIMD).
    if (!EARLY) prologue();
    // the NEXT launch's weights: after the first chunk's loads and the coefficient loads (prefetch_weight_lines)
    const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), nblocks = gridDim.x * gridDim.y * gridDim.z;
    auto prefetch_next_weights = [&]() { prefetch_weight_lines(a, lin, nblocks, NTHREADS, tid, pf_sink, pf_sink2); };
    if (SPEC) {
      // loader waves fill buffer (k+1)&1 while compute waves consume buffer k&1; one barrier per chunk
      if (loader && c_begin < c_end) load_first(stA);
      stamp(1);
      if (EARLY) { if (fastp) prologue_fast(); else prologue(); }
      prefetch_next_weights();
      stamp(2);
      if (loader && c_begin < c_end) store_chunk(c_begin, stA, 0);
      __syncthreads();
      stamp(9);
      int k = 0;
      for (int c0 = c_begin; c0 < c_end; c0 += KC, ++k) {
        if (loader) {
          if (c0 + KC < c_end) { load_chunk(c0 + KC, stA); store_chunk(c0 + KC, stA, ((k + 1) & 1) * C::STAGE); }
        } else {
          mfma_chunk((k & 1) * C::STAGE);
        }
        __syncthreads();
      }
    } else if (PF == 1) {
      if (c_begin < c_end) load_first(stA);
      stamp(1);
      if (EARLY) { if (fastp) prologue_fast(); else prologue(); }
      prefetch_next_weights();
      stamp(2);
      for (int c0 = c_begin; c0 < c_end; c0 += KC) {
        store_chunk(c0, stA);
        __syncthreads();
        if (c0 == c_begin) stamp(9);
        if (c0 + KC < c_end) load_chunk(c0 + KC, stA);
        mfma_chunk();
        __syncthreads();
      }
    } else {
      if (c_begin < c_end) load_first(stA);
      if (c_begin + KC < c_end) load_chunk(c_begin + KC, stB);
      stamp(1);
      if (EARLY) { if (fastp) prologue_fast(); else prologue(); }
      prefetch_next_weights();
      stamp(2);
      for (int c0 = c_begin; c0 < c_end; c0 += 2 * KC) {
        store_chunk(c0, stA);
        __syncthreads();
        if (c0 == c_begin) stamp(9);
        if (c0 + 2 * KC < c_end) load_chunk(c0 + 2 * KC, stA);
        mfma_chunk();
        __syncthreads();
        if (c0 + KC < c_end) {
          store_chunk(c0 + KC, stB);
          __syncthreads();
          if (c0 + 3 * KC < c_end) load_chunk(c0 + 3 * KC, stB);
          mfma_chunk();
          __syncthreads();
        }
      }
    }
  } else {
  prologue();
  for (int c0 = c_begin; c0 < c_end; c0 += KC) {
    // ================= stage activations =================
    if (TAPS == 27) {
      if (vecx) {
        constexpr int IPR = TW / 4 + 2;
        constexpr int ITEMS = KC * DS * HS * IPR;
        for (int it = tid; it < ITEMS; it += NTHREADS) {
          const int q = it % IPR;
          int row = it / IPR;
          const int hy = row % HS; row /= HS;
          const int dz = row % DS;
          const int cl = row / DS;
          const int c = c0 + cl;
          const int d = d0 + dz - 1, h = h0 + hy - 1;
          const bool rowok = (c < a.Cin) && (unsigned)d < (unsigned)a.D && (unsigned)h < (unsigned)a.H;
          float* dst = Xs + cl * XS + (dz * HS + hy) * RS;
          const long gro = (long)c * V + ((long)d * a.H + h) * a.W;
          if (q < TW / 4) {
            const int w = w0 + 4 * q;
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            if (rowok && w < a.W) {
              f32x4 x0 = *reinterpret_cast<const f32x4*>(in0n + gro + w);
              f32x4 x1 = x0;
              if (PRO == PRO_GRAD) x1 = *reinterpret_cast<const f32x4*>(in1n + gro + w);
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = pro_apply<PRO>(coef, cpad, c, x0[e], x1[e]);
            }
            *reinterpret_cast<f32x4*>(dst + 4 + 4 * q) = o;
          } else {
            const int w = (q == TW / 4) ? w0 - 1 : w0 + TW;
            float o = 0.f;
            if (rowok && (unsigned)w < (unsigned)a.W) {
              const float x0 = in0n[gro + w];
              const float x1 = (PRO == PRO_GRAD) ? in1n[gro + w] : x0;
              o = pro_apply<PRO>(coef, cpad, c, x0, x1);
            }
            dst[(q == TW / 4) ? 3 : TW + 4] = o;
          }
        }
      } else {
        constexpr int IPR = TW + 2;
        constexpr int ITEMS = KC * DS * HS * IPR;
        for (int it = tid; it < ITEMS; it += NTHREADS) {
          const int q = it % IPR;
          int row = it / IPR;
          const int hy = row % HS; row /= HS;
          const int dz = row % DS;
          const int cl = row / DS;
          const int c = c0 + cl;
          const int d = d0 + dz - 1, h = h0 + hy - 1, w = w0 + q - 1;
          float o = 0.f;
          if ((c < a.Cin) && (unsigned)d < (unsigned)a.D && (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W) {
            const long g = (long)c * V + ((long)d * a.H + h) * a.W + w;
            const float x0 = in0n[g];
            const float x1 = (PRO == PRO_GRAD) ? in1n[g] : x0;
            o = pro_apply<PRO>(coef, cpad, c, x0, x1);
          }
          Xs[cl * XS + (dz * HS + hy) * RS + 3 + q] = o;
        }
      }
    } else {
      if (vecx) {
        constexpr int ITEMS = KC * V_B / 4;
        for (int it = tid; it < ITEMS; it += NTHREADS) {
          const int q = it % (V_B / 4);
          const int cl = it / (V_B / 4);
          const int c = c0 + cl;
          const int v = v0_ + 4 * q;
          f32x4 o = {0.f, 0.f, 0.f, 0.f};
          if (c < a.Cin && v < V) {
            const long g = (long)c * V + v;
            f32x4 x0 = *reinterpret_cast<const f32x4*>(in0n + g);
            f32x4 x1 = x0;
            if (PRO == PRO_GRAD) x1 = *reinterpret_cast<const f32x4*>(in1n + g);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = pro_apply<PRO>(coef, cpad, c, x0[e], x1[e]);
          }
          *reinterpret_cast<f32x4*>(Xs + cl * XS + 4 * q) = o;
        }
      } else {
        constexpr int ITEMS = KC * V_B;
        for (int it = tid; it < ITEMS; it += NTHREADS) {
          const int q = it % V_B;
          const int cl = it / V_B;
          const int c = c0 + cl;
          const int v = v0_ + q;
          float o = 0.f;
          if (c < a.Cin && v < V) {
            const long g = (long)c * V + v;
            const float x0 = in0n[g];
            const float x1 = (PRO == PRO_GRAD) ? in1n[g] : x0;
            o = pro_apply<PRO>(coef, cpad, c, x0, x1);
          }
          Xs[cl * XS + q] = o;
        }
      }
    }
    // ================= stage weights =================
    {
      const int krows = KC * TAPS;
      const long kbase = (long)c0 * TAPS;
      const long klim = (long)a.Cin * TAPS;
      if (vecw) {
        const int items = krows * (M_B / 4);
        for (int it = tid; it < items; it += NTHREADS) {
          const int q = it % (M_B / 4);
          const int kr = it / (M_B / 4);
          const int m = m0 + 4 * q;
          f32x4 o = {0.f, 0.f, 0.f, 0.f};
          if (kbase + kr < klim && m < a.M) o = *reinterpret_cast<const f32x4*>(a.w + (kbase + kr) * a.w_ld + m);
          *reinterpret_cast<f32x4*>(Ws + kr * M_B + 4 * q) = o;
        }
      } else {
        const int items = krows * M_B;
        for (int it = tid; it < items; it += NTHREADS) {
          const int q = it % M_B;
          const int kr = it / M_B;
          float o = 0.f;
          if (kbase + kr < klim && m0 + q < a.M) o = a.w[(kbase + kr) * a.w_ld + m0 + q];
          Ws[kr * M_B + q] = o;
        }
      }
    }
    __syncthreads();
    if (!loader) mfma_chunk();
    __syncthreads();
  }
  }

  stamp(3);
  // ---- after the K loop: in-block reduction, cross-workgroup hand-off, epilogue, flush (the tails above) ----
  float* red0 = ecoef + 6 * M_B;            // [WN][M_B] partial sums, one writer per slot (no LDS atomics: reproducible)
  float* red1 = red0 + WN * M_B;
  const bool want_sums = (EPI == EPI_STORE_STATS) ? (a.st_out.sum != nullptr) : (EPI != EPI_STORE);
  using Tail = FpropTail<TAPS, PRO, EPI, WM, WN, KS, MT, NT, KC, TD, TH, TW, SPEC>;
  const Tail tail{a.D, a.H, a.W, V, a.M, TileAt{d0, h0, w0, v0_}, m0, wm, wn, kg, half, l31, lane, outn, exn, ecoef, red0, red1, Xs, want_sums};
  // cross-block K-split (kz > 1): this tile's partial accumulator tiles in a.kz_part, its arrival counter, the ticket's word of LDS
  constexpr int NSLOT = Tail::NSLOT, RP = Tail::RP;
  const int slot = tail.slot();
  const long tile_id = blockIdx.x + (long)gridDim.x * blockIdx.y;
  float* part = a.kz_part + (tile_id * kz) * NSLOT * 1024;
  auto kz_last = [&]() { return kz_arrive(a.kz_cnt + tile_id, kz, reinterpret_cast<unsigned*>(ecoef + C::ECOEF * M_B), tid, [&]() { stamp(5); }); };
  if constexpr (C::DIST) {
    float my[RP];
    tail.dist_reduce(acc[0][0], my);
    stamp(4);
    if (kz > 1) {
      // as in the general tail below, but every wave publishes and sums its own rows
      kz_publish_rows<RP>(part, NSLOT, slot, kg * RP, lane, blockIdx.z, my);
      if (!kz_last()) return;                               // not the last slice of this tile: done
      kz_sum_slices<RP>(part, NSLOT, slot, kg * RP, lane, kz, my);
    }
    stamp(6);
    tail.dist_epilogue(my);
  } else {
    if constexpr (KS > 1) tail.group_reduce(loader, acc);
    stamp(4);
    if (kz > 1) {
      // publish the partial tile; the LAST arriving slice sums all slices (in slice order: bit-reproducible) and runs the epilogue
      if (kg == 0 && !loader) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) kz_publish_rows<16>(part, NSLOT, slot + i * NT + j, 0, lane, blockIdx.z, acc[i][j]);
      }
      if (!kz_last()) return;                               // not the last slice of this tile: done
      tail.kz_collect(part, kz, loader, acc);
    }
    stamp(6);
    // the wide epilogue reuses the staging area: with an in-block K-split the group-0 waves were still reading their partners'
    // accumulators (kz == 1) or the summed slices (kz > 1) from it
    if (C::WIDE && KS > 1) __syncthreads();
    if (kg == 0 && !loader) {
      const bool wide_ok = C::WIDE && (V & 3) == 0 && ((TAPS == 27) ? ((a.W & 3) == 0) : true) && ((((uintptr_t)outn | (uintptr_t)exn) & 15) == 0);
      if (C::WIDE && wide_ok) tail.epilogue_wide(acc);
      else tail.epilogue_direct(acc);
    }
  }
  stamp(7);
  if (want_sums) {
    __syncthreads();
    for (int m = tid; m < M_B; m += NTHREADS) {
      if (m0 + m >= a.M) continue;
      flush_row_sums<EPI, WN>(a, rep, m0 + m, red0 + m, red1 + m, M_B, EpiRow<M_B>{ecoef + m}.gamma());
    }
  }
  prefetch_sink(a, pf_sink, pf_sink2);
  stamp(8);
  if (tracing) {
    a.trace[10] = ((unsigned long long)TAPS << 48) | ((unsigned long long)PRO << 40) | ((unsigned long long)EPI << 32) | ((unsigned long long)a.M << 16) | (unsigned long long)a.Cin;
    a.trace[11] = ((unsigned long long)gridDim.x << 32) | ((unsigned long long)gridDim.y << 16) | gridDim.z;
    a.trace[12] = ((unsigned long long)(WM * WN * KS) << 32) | ((unsigned long long)KC << 16) | (unsigned long long)(MT * NT);
  }
}

#endif  // __HIPCC__
}  // namespace mmnn
