// Dense-layer conv2 forward (models/densenet.py:80-85: ReLU(BN(t1)) -> 3x3x3 convolution to `growth` = 32 new channels -> channel dropout,
// + the batch statistics of the new channels for their consumers) for extents wider than 16 voxels, on the bf16 matrix pipe with fp32 accuracy:
// every fp32 operand is split into three bf16 pieces (x = hi + mid + lo, round to nearest at each step: 24 mantissa bits, bf16x3.hpp) and a
// product becomes six v_mfma_f32_32x32x16_bf16 (mid.mid, hi.lo, lo.hi, hi.mid, mid.hi, hi.hi) into one fp32 accumulator.  Measured against
// fp64 (tools/microbench/bf16x3_gemm.hip, conv3_bf16x3.hip): 4.5e-7 rms -- the fp32 matrix instruction's own error is 1.0e-6 -- at 16x the
// rate per instruction cycle; and the bf16 instruction leaves the vector ALU free beside it, which v_mfma_f32_32x32x2_f32 does not
// (profiles/r03_microbench_mfma_acc_file.txt).  Same arguments, same results to fp32 rounding and the same statistics protocol as
// fprop_kernel<27, PRO_BNRELU, EPI_STORE_STATS> (fprop.hpp), which stays the kernel for every other shape.
//   Both operands arrive pre-split.  The weights come from a panel the pack launch wrote once per parameter version (PackJob kind 5 / 6,
//   [piece][tap][k / 8][row] 16-byte entries: a lane's fragment is three 16-byte loads).  The activations come from operand planes a split
//   pass writes right before the convolution, in the same launch_*: conv3_split_bnrelu_kernel (forward, ReLU(BN(T1)) of all input channels)
//   and conv3_split_bnbwd_kernel (data gradient, the BN backward operand of the layer's 32 channels), [piece][n][c / 8][voxel] 16-byte
//   entries = one LDS operand row each.  The convolution kernels stage with 16-byte copies and do no conversion arithmetic at all; the
//   split passes use exactly the arithmetic the kernels used to apply on operand load, so the pieces -- and the results -- are the same.
//   MFMA mapping: i = output channel (32), j = voxel (32 consecutive w), k = input channel (16 per instruction); a tap is a row offset.
//   Workgroup: 4 waves, a 2 x 4 x 32 voxel tile.  In-block K-split over the taps: every wave multiplies all eight 32-voxel rows with taps
//   wv, wv + 4, ... (a weight operand serves 48 MFMAs, no two waves load the same weights); the four partial tiles are summed through LDS.
//   LDS: the halo tile of a 16-channel chunk as three bf16 planes [piece][channel half][halo voxel] of 16-byte entries, two buffers: chunk
//   ch + 1 is loaded at the head of chunk ch's tap loop and copied to the other buffer between its MFMAs; one barrier per chunk.
//   Occupancy: 154 KB of LDS per workgroup = one workgroup (one wave per SIMD) per CU; block 1 of the flagship (2 x 32^3) has exactly one
//   tile per CU, so a second resident workgroup would have nothing to run -- the latency is hidden inside the wave (one chunk ahead).
#include <stdlib.h>

#include "fprop.hpp"
#include "bf16x3.hpp"

namespace mmnn {

namespace c3b {
constexpr int KC = BF16X3_KC, NT = 7, MAXC = 256;
// The one tile of both kernels: 2 x 4 x 32 = 256 voxels, extents wider than 16 (one workgroup per CU at 2 x 32^3).
using G = HaloTile<2, 4, 32>;
constexpr size_t FWD_SMEM = G::OPER_BYTES + sizeof(float) * (2 * 4 * 32 + 32);            // + statistics scratch, dropout scales
constexpr size_t DGRAD_SMEM = G::OPER_BYTES + sizeof(float) * 512;                        // + the mask's norm2 coefficients
static_assert(G::ITEMS <= NT, "forward: one staging item per tap slot");
static_assert(FWD_SMEM <= 160 * 1024 && DGRAD_SMEM <= 160 * 1024, "LDS");
}  // namespace c3b

// ----------------------------------------------------------------------------------------------------------------
// Split passes: one thread per (voxel, group of 8 channels), one plane entry each (bf16x3.hpp).  A workgroup is 256 voxels of one channel
// group of one sample; its 8 coefficients go through LDS while its operand loads are in flight.
// ----------------------------------------------------------------------------------------------------------------
// shared end of both passes: the thread's eight values -> its plane entry of each piece
__device__ __forceinline__ void split_store(const FpropArgs& a, int n, int c8, int v, const float (&f)[8]) {
  const int C8 = a.Cin / 8, V = a.D * a.H * a.W;
  store_pieces(reinterpret_cast<uint4*>(a.x3) + plane_entry(n, c8, v, C8, V), plane_piece_stride(a.N, C8, V), f);
}

// forward operand: ReLU(BN(T1)) of all Cin channels -- exactly fmaxf(fmaf(a_c, x, b_c), 0) with bn_fwd_coef, then split3
__global__ void __launch_bounds__(256) conv3_split_bnrelu_kernel(const FpropArgs a) {
  __shared__ float cf[2][8];
  const int c8 = blockIdx.y, n = blockIdx.z, V = a.D * a.H * a.W;
  const int v = blockIdx.x * 256 + threadIdx.x;
  const float* __restrict__ x = a.in0 + (long)n * a.in0_ns + (long)(a.in0_coff + 8 * c8) * V;
  float xv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) xv[e] = v < V ? x[(long)e * V + v] : 0.f;
  if (threadIdx.x < 8) {
    float ca, cb, mu, rs;
    bn_fwd_coef(a.bn_in, 8 * c8 + threadIdx.x, ca, cb, mu, rs);
    cf[0][threadIdx.x] = ca; cf[1][threadIdx.x] = cb;
  }
  __syncthreads();
  if (v >= V) return;
#pragma unroll
  for (int e = 0; e < 8; ++e) xv[e] = fmaxf(fmaf(cf[0][e], xv[e], cf[1][e]), 0.f);
  split_store(a, n, c8, v, xv);
}

// data-gradient operand of the layer's 32 output channels: f = fmaf(p_c s, G, fmaf(q_c s, X, r_c s)), bn_bwd_coef(gr_in), s = drop_scale(drop_in)
__global__ void __launch_bounds__(256) conv3_split_bnbwd_kernel(const FpropArgs a) {
  __shared__ float cf[3][8];
  const int c8 = blockIdx.y, n = blockIdx.z, V = a.D * a.H * a.W;
  const int v = blockIdx.x * 256 + threadIdx.x;
  const float* __restrict__ gn = a.in0 + (long)n * a.in0_ns + (long)(a.in0_coff + 8 * c8) * V;
  const float* __restrict__ xn = a.in1 + (long)n * a.in1_ns + (long)(a.in1_coff + 8 * c8) * V;
  float gv[8], xv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    gv[e] = v < V ? gn[(long)e * V + v] : 0.f;
    xv[e] = v < V ? xn[(long)e * V + v] : 0.f;
  }
  if (threadIdx.x < 8) {
    const int c = 8 * c8 + threadIdx.x;
    float p_, q_, r_;
    bn_bwd_coef(a.gr_in, c, p_, q_, r_);
    const float sc = drop_scale(a.drop_in, n, c);
    cf[0][threadIdx.x] = p_ * sc; cf[1][threadIdx.x] = q_ * sc; cf[2][threadIdx.x] = r_ * sc;
  }
  __syncthreads();
  if (v >= V) return;
#pragma unroll
  for (int e = 0; e < 8; ++e) gv[e] = fmaf(cf[0][e], gv[e], fmaf(cf[1][e], xv[e], cf[2][e]));
  split_store(a, n, c8, v, gv);
}

static int launch_split(bool bwd, const FpropArgs& a, hipStream_t stream) {
  const int V = a.D * a.H * a.W;
  const dim3 grid((unsigned)cdiv(V, 256), (unsigned)(a.Cin / 8), (unsigned)a.N);
  if (bwd) MMNN_LAUNCH(conv3_split_bnbwd_kernel, grid, dim3(256), 0, stream, a);
  else MMNN_LAUNCH(conv3_split_bnrelu_kernel, grid, dim3(256), 0, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

// ----------------------------------------------------------------------------------------------------------------
// conv2 forward on the pre-split planes (a.x3) and weight panel (a.w3, pack kind 5: [piece][tap][Cin / 8][32])
// ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv3_fwd_bf16x3_kernel(const FpropArgs a) {
  using namespace c3b;
  constexpr int ROWS = G::ROWS, ITEMS = G::ITEMS;
  extern __shared__ uint4 xs128[];                          // [2][3][2][HV]
  float* const sred = reinterpret_cast<float*>(reinterpret_cast<char*>(xs128) + G::OPER_BYTES);   // [2][4][32]
  float* const dsc = sred + 2 * 4 * 32;                     // [32] dropout scale of the output channels
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int D = a.D, H = a.H, W = a.W, V = D * H * W, C8 = a.Cin / 8, nchunk = a.Cin / KC;
  const G tile(blockIdx.x, D, H, W);
  const int n = tile.n;
  const uint4* __restrict__ wp = reinterpret_cast<const uint4*>(a.w3);
  if (tid < 32) dsc[tid] = drop_scale(a.drop_out, n, tid);
  f32x16_t acc[ROWS];
#pragma unroll
  for (int t = 0; t < ROWS; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
  const HaloStage<G> stage(tile, reinterpret_cast<const uint4*>(a.x3), a.N, C8, tid, D, H, W);   // zero padding AFTER BN + ReLU
  HaloStage<G>::Regs xr;
  // weights: lane = (row m, channel half); ring slot ti holds the three pieces of tap wv + 4 ti of the chunk ahead
  bf16x8_t wr[NT][3];
  auto load_w = [&](int ti, int ch) {
    const int tap = wv + 4 * ti;
    if (tap < 27 && ch < nchunk) {
#pragma unroll
      for (int p = 0; p < 3; ++p) wr[ti][p] = as_bf16x8(wp[panel_entry(p, tap, 2 * ch + (lane >> 5), lane & 31, C8, 32)]);
    }
  };
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) load_w(ti, 0);
  stage.issue(xr, 0);
  stage.commit(xr, xs128);
  __syncthreads();
  for (int ch = 0; ch < nchunk; ++ch) {
    const int cur = ch & 1;
    const bool more = ch + 1 < nchunk;
    if (more) stage.issue(xr, ch + 1);
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int tap = wv + 4 * ti;
      if (tap < 27) {
        const int td = tap / 9, th = (tap / 3) % 3, tw = tap % 3;
        bf16x8_t aw[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) aw[p] = wr[ti][p];
        load_w(ti, ch + 1);
#pragma unroll
        for (int t = 0; t < ROWS; ++t) {
          const int hv = G::tap_hv(t, lane & 31, td, th, tw);
          bf16x8_t bb[3];
#pragma unroll
          for (int p = 0; p < 3; ++p) bb[p] = as_bf16x8(xs128[cur * G::BUF + G::lds_entry(p, lane >> 5, hv)]);
          mfma_bf16x3(acc[t], aw, bb);
        }
      }
      if (more && ti < ITEMS) stage.commit_item(xr, ti, xs128 + (cur ^ 1) * G::BUF);   // one item between the MFMAs of each tap
    }
    __syncthreads();
  }
  // sum the four waves' partial tiles (fixed order) through LDS; wave wv finishes rows wv, wv + 4, ... of the tile.
  // register q of lane l: output channel acc_row(q, l / 32), voxel column l % 32
  float* red = reinterpret_cast<float*>(xs128);            // [wave][row][q][lane]
#pragma unroll
  for (int t = 0; t < ROWS; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) red[((wv * ROWS + t) * 16 + q) * 64 + lane] = acc[t][q];
  __syncthreads();
  float* __restrict__ outn = a.out + (long)n * a.out_ns + (long)a.out_coff * V;
  const bool want_sums = a.st_out.sum != nullptr;
  float s0[16], s1[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) { s0[q] = 0.f; s1[q] = 0.f; }
#pragma unroll
  for (int tt = 0; tt < (ROWS + 3) / 4; ++tt) {
    const int t = wv + 4 * tt;
    if (t >= ROWS) break;
    int o;
    const bool ok = tile.row_pos(t, lane & 31, D, H, W, o);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float val = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) val += red[((w2 * ROWS + t) * 16 + q) * 64 + lane];
      const int m = acc_row(q, lane >> 5);
      val *= dsc[m];
      if (ok) {
        outn[(long)m * V + o] = val;
        s0[q] += val;
        s1[q] += val * val;
      }
    }
  }
  if (want_sums) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float t0 = s0[q], t1 = s1[q];
      half_sum2(t0, t1);
      if ((lane & 31) == 0) {
        const int m = acc_row(q, lane >> 5);
        sred[wv * 32 + m] = t0;
        sred[4 * 32 + wv * 32 + m] = t1;
      }
    }
    __syncthreads();
    if (tid < 32) {
      const int rep = blockIdx.x & ((a.nrep > 0 ? a.nrep : NREP) - 1);
      double v0 = 0.0, v1 = 0.0;
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) { v0 += (double)sred[w2 * 32 + tid]; v1 += (double)sred[4 * 32 + w2 * 32 + tid]; }
      atomicAdd(a.st_out.sum + (long)rep * a.st_out.stride + a.st_out.off + tid, v0);
      atomicAdd(a.st_out.sq + (long)rep * a.st_out.stride + a.st_out.off + tid, v1);
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------
// conv2 DATA GRADIENT of the wide extents (autograd adjoint of the same layer, main.py:469): 32 -> 128 channels,
//   operand f(c, v) = p_c G[c][v] + q_c X[c][v] + r_c (BN backward of the layer's output channels, dropout scale folded in, zero padding
//   after it: conv3_split_bnbwd_kernel writes it pre-split to a.x3), epilogue: ReLU mask of conv2's input (pre = a_m T1 + b_m > 0), store,
//   d beta / d gamma sums of norm2 -- the contract of fprop_kernel<27, PRO_GRAD, EPI_MASK_STORE>.  Same tile and LDS planes as the forward;
//   here the reduction is only 32 channels x 27 taps, so BOTH 16-channel chunks get an LDS buffer of their own: chunk 0 is staged up front,
//   chunk 1's copies are in flight under chunk 0's first (td, th) pair of taps and land in LDS before the second one.  Wave wv owns output
//   rows 32 wv .. 32 wv + 31 for all eight voxel rows and all taps (no cross-wave sum); its weights come through a three-tap ring of
//   pre-split fragments (pack kind 6: [piece][tap][32 / 8][128]).
// ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv3_dgrad_bf16x3_kernel(const FpropArgs a) {
  using namespace c3b;
  constexpr int ROWS = G::ROWS, PF = 3, C8 = 4;
  extern __shared__ uint4 xs128[];                          // [2 chunks][3][2][HV]
  float* const ecoef = reinterpret_cast<float*>(reinterpret_cast<char*>(xs128) + G::OPER_BYTES);   // [4][128]: a_m, b_m, mean_m, rstd_m of norm2
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int D = a.D, H = a.H, W = a.W, V = D * H * W;
  const G tile(blockIdx.x, D, H, W);
  const int n = tile.n;
  const uint4* __restrict__ wp = reinterpret_cast<const uint4*>(a.w3);
  const HaloStage<G> stage(tile, reinterpret_cast<const uint4*>(a.x3), a.N, C8, tid, D, H, W);
  HaloStage<G>::Regs xr;
  // weights: lane = (row m of this wave's tile, channel half); ring slot tap % PF
  bf16x8_t wr[PF][3];
  auto load_w = [&](int slot, int tap, int ch) {
    if (ch < 2) {
#pragma unroll
      for (int p = 0; p < 3; ++p) wr[slot][p] = as_bf16x8(wp[panel_entry(p, tap, 2 * ch + (lane >> 5), wv * 32 + (lane & 31), C8, 128)]);
    }
  };
#pragma unroll
  for (int t = 0; t < PF; ++t) load_w(t, t, 0);
  stage.issue(xr, 0);
  if (tid >= 128) {                                         // the statistics loads travel beside the operand loads
    const int m = tid - 128;
    float ea, eb, mu, rs;
    bn_fwd_coef(a.ebn, m, ea, eb, mu, rs);
    ecoef[m] = ea; ecoef[128 + m] = eb; ecoef[256 + m] = mu; ecoef[384 + m] = rs;
  }
  stage.commit(xr, xs128);
  stage.issue(xr, 1);
  __syncthreads();
  f32x16_t acc[ROWS];
#pragma unroll
  for (int t = 0; t < ROWS; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
  auto pair = [&](int ch, int tq) {                         // (td, th) pair tq of chunk ch; its three tw = the ring's three slots
    const int td = tq / 3, th = tq % 3;
#pragma unroll
    for (int tw = 0; tw < 3; ++tw) {
      const int tap = tq * 3 + tw;
      bf16x8_t aw[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) aw[p] = wr[tw][p];
      if (tq < 8) load_w(tw, tap + PF, ch); else load_w(tw, tw, ch + 1);
#pragma unroll
      for (int t = 0; t < ROWS; ++t) {
        const int hv = G::tap_hv(t, lane & 31, td, th, tw);
        bf16x8_t bb[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) bb[p] = as_bf16x8(xs128[ch * G::BUF + G::lds_entry(p, lane >> 5, hv)]);
        mfma_bf16x3(acc[t], aw, bb);
      }
    }
  };
  pair(0, 0);
  stage.commit(xr, xs128 + G::BUF);                             // chunk 1 -> its own buffer: nobody reads it before this barrier
  __syncthreads();
#pragma unroll 1
  for (int tq = 1; tq < 9; ++tq) pair(0, tq);
#pragma unroll 1
  for (int tq = 0; tq < 9; ++tq) pair(1, tq);
  // epilogue: register q of lane l = output row 32 wv + acc_row(q, l / 32), voxel column l % 32 of row t
  const float* __restrict__ exn = a.ex + (long)n * a.ex_ns + (long)a.ex_coff * V;
  float* __restrict__ outn = a.out + (long)n * a.out_ns + (long)a.out_coff * V;
  float s0[16], s1[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) { s0[q] = 0.f; s1[q] = 0.f; }
  float xn[16];
  {
    int o;
    const bool ok = tile.row_pos(0, lane & 31, D, H, W, o);
#pragma unroll
    for (int q = 0; q < 16; ++q) xn[q] = ok ? exn[(long)(wv * 32 + acc_row(q, lane >> 5)) * V + o] : 0.f;
  }
#pragma unroll
  for (int t = 0; t < ROWS; ++t) {
    int o;
    const bool ok = tile.row_pos(t, lane & 31, D, H, W, o);
    float xe[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) xe[q] = xn[q];
    if (t + 1 < ROWS) {                                     // the next row's mask operand is in flight while this row is masked and stored
      int o2;
      const bool ok2 = tile.row_pos(t + 1, lane & 31, D, H, W, o2);
#pragma unroll
      for (int q = 0; q < 16; ++q) xn[q] = ok2 ? exn[(long)(wv * 32 + acc_row(q, lane >> 5)) * V + o2] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int m = wv * 32 + acc_row(q, lane >> 5);
      if (ok) {
        const EpiRow<128> e{ecoef + m};
        float z, xh;
        mask_elem(e.a(), e.b(), e.mean(), e.rstd(), xe[q], acc[t][q], z, xh);
        outn[(long)m * V + o] = z;
        s0[q] += z;
        s1[q] += z * xh;
      }
    }
  }
  const int rep = blockIdx.x & ((a.nrep > 0 ? a.nrep : NREP) - 1);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    float t0 = s0[q], t1 = s1[q];
    half_sum2(t0, t1);
    if ((lane & 31) == 0) {
      const int m = wv * 32 + acc_row(q, lane >> 5);
      atomicAdd(a.dbeta + (long)rep * a.M + m, (double)t0);
      atomicAdd(a.dgamma + (long)rep * a.M + m, (double)t1);
    }
  }
}

// operand planes of one launch: three pieces x N x Cin / 8 x V entries of 16 bytes (the forward's Cin = 128, the data gradient's Cin = 32)
size_t conv3_bf16x3_plane_bytes(const FpropArgs& a) { return (size_t)3 * plane_piece_stride(a.N, a.Cin / 8, a.D * a.H * a.W) * 16; }

// What both launches share once their own checks have passed: the checks on the planes, the offsets and the grid (`who` names the launch in
// the messages, `chans` = channels of its widest tensor), the LDS opt-in, the split pass and the kernel, one workgroup per tile.
template <auto KERN>
static int launch_tiles(const char* who, bool bwd, int chans, size_t smem, const FpropArgs& a, hipStream_t stream) {
  MMNN_REQUIRE(a.w3 && a.x3 && a.x3_bytes >= conv3_bf16x3_plane_bytes(a), "%s: pre-split weights or plane scratch missing", who);
  MMNN_REQUIRE((long)(chans + 1) * a.D * a.H * a.W < (1l << 31), "%s: volume too large for 32-bit element offsets", who);
  const long tiles = c3b::G::count(a.N, a.D, a.H, a.W);
  MMNN_REQUIRE(tiles > 0 && tiles < (1l << 31), "%s: grid out of range", who);
  if (int rc = allow_dynamic_lds<KERN>(smem)) return rc;
  if (int rc = launch_split(bwd, a, stream)) return rc;
  MMNN_LAUNCH(KERN, dim3((unsigned)tiles), dim3(256), smem, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

bool conv3_dgrad_bf16x3_eligible(const FpropArgs& a) {
  static const int mode = [] { const char* e = getenv("MMNN_BF16X3_DGRAD"); return e ? atoi(e) : 1; }();
  static const int fmode = [] { const char* e = getenv("MMNN_BF16X3"); return e ? atoi(e) : 32; }();
  return mode != 0 && fmode != 0 && a.M == 128 && a.Cin == 32 && a.W > 16;
}

int launch_conv3_dgrad_bf16x3(const FpropArgs& a, hipStream_t stream) {
  MMNN_REQUIRE(conv3_dgrad_bf16x3_eligible(a), "conv3 dgrad bf16x3: shape not handled (M=%d, Cin=%d, W=%d)", a.M, a.Cin, a.W);
  MMNN_REQUIRE(a.in1 && a.ex && a.dgamma && a.dbeta, "conv3 dgrad bf16x3: operands missing");
  return launch_tiles<conv3_dgrad_bf16x3_kernel>("conv3 dgrad bf16x3", true, a.M, c3b::DGRAD_SMEM, a, stream);
}

// Shapes this kernel takes (everything else stays on fprop_kernel): 32 output channels, input channels in chunks of 16, rows wider than
// 16 voxels.  MMNN_BF16X3=0 switches it off (A/B runs, debugging).  (r03: a 1 x 2 x 16 tile for the 9..16-voxel extents passed parity
// but was SLOWER than fprop_kernel at 2 x 16^3 -- 40.6 vs 28.2 us per launch, profiles/r03_ab_experiments.txt: 256 workgroups of 32
// voxels each stage a 6.75x halo and read all 442 KB of weights; those layers need a cross-workgroup K-split instead.)
bool conv3_fwd_bf16x3_eligible(const FpropArgs& a) {
  static const int mode = [] { const char* e = getenv("MMNN_BF16X3"); return e ? atoi(e) : 32; }();
  return mode != 0 && a.M == 32 && a.Cin % c3b::KC == 0 && a.Cin >= c3b::KC && a.Cin <= c3b::MAXC && a.W > 16;
}

int launch_conv3_fwd_bf16x3(const FpropArgs& a, hipStream_t stream) {
  MMNN_REQUIRE(conv3_fwd_bf16x3_eligible(a), "conv3 bf16x3: shape not handled (M=%d, Cin=%d, W=%d)", a.M, a.Cin, a.W);
  MMNN_REQUIRE(a.drop_in.p <= 0.f, "conv3 bf16x3: no input dropout on this path");
  return launch_tiles<conv3_fwd_bf16x3_kernel>("conv3 bf16x3", false, a.Cin, c3b::FWD_SMEM, a, stream);
}

}  // namespace mmnn
