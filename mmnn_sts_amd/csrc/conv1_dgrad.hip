// Dense-layer conv1 data gradient with a RESIDENT operand tile (fp32 MFMA, same contract as fprop_kernel<1, PRO_GRAD, EPI_MASK_ACCUM>).
//
//     G[n][m][v] += gamma_m * relu'(a_m * X[n][m][v] + b_m) * sum_{k < 128} w[k][m] * z1[n][k][v],   z1 = BN-backward(dZ2, T1)
//
// The launch has the opposite shape to conv1 forward: K is fixed (the bottleneck width, 128) and M = cin is large.  fprop_kernel tiles
// M over blockIdx.y, so every M-tile workgroup fetches and normalises the same 2 x 128-channel voxel tile again (2-8 times at 16^3), and
// each workgroup is MFMA loop THEN epilogue, in lock-step with its neighbours.  Here one workgroup takes a 64-voxel tile, normalises the
// operand ONCE into LDS (128 x 64 floats) and walks over its rows in steps of 64:
//
//   per row step:  two K chunks of 64 channels (weights [64][64] through LDS, the next chunk's loads in flight in registers)
//                  32 MFMAs (v_mfma_f32_32x32x2_f32, k in the order of fprop_kernel's tile: KS below) per chunk and wave, waves as
//                  2 (rows) x 2 (voxels)
//                  mask / accumulate epilogue of the step in the 16-byte form of fprop_kernel (accumulator transposed through a
//                  wave-private LDS tile); the X and G loads of step t+1 are issued before the MFMAs of step t (two register
//                  sets) and stay in flight under both of its MFMA phases, the per-row coefficients of step t+1 are computed
//                  beside them.
//
// Two workgroups of four waves share a CU (71 KB of LDS each): while one is in its epilogue the other one's MFMAs keep the matrix
// pipe busy.  A workgroup owns every row of its row range for its voxels, so the read-modify-write of G needs no atomics.
// grid = (voxel tiles, row groups): the host splits the row steps over as many row groups as it takes to fill the chip once.
#include <algorithm>

#include "fprop.hpp"

namespace mmnn {

namespace {
constexpr int RK = 128;        // operand channels (the resident tile holds all of them)
constexpr int RVT = 64;        // voxels per workgroup
constexpr int RMS = 64;        // rows per step
constexpr int RKC = 64;        // channels per weight chunk
constexpr int RTHREADS = 256;
constexpr int RTS = 36;        // row stride of the transposition tile (as FpropCfg::TSTRIDE)
constexpr int R_COEF = 3 * RK, R_Z = RK * RVT, R_W = RKC * RMS, R_T = 4 * 32 * RTS, R_E = 2 * 5 * RMS, R_RED = 2 * 2 * RMS;
constexpr size_t R_SMEM = sizeof(float) * (R_COEF + R_Z + R_W + R_T + R_E + R_RED);
constexpr int R_FILL = 512;    // workgroups that fill the chip once: 256 CUs x 2
}  // namespace

#if defined(__HIPCC__)
// KS: the in-block K-split of the fprop_kernel tile that the shape would take (fprop_dispatch.hpp: 1, 2 or 8 wave groups).  The kernel
// takes its fp32 sums in THAT kernel's order, so that a plan computes the same bits whichever kernel a layer runs on (a training run of 25
// steps otherwise drifts apart by 1e-3 of the risk scores; the build has floating-point contraction off, so a sum written the same way
// is the same sum).  Over K: wave group g of fprop_kernel chains the channel pairs g, g + KS, g + 2 KS, ... through its MFMAs from zero,
// and the groups' partial tiles are added in group order.  Here one wave runs the groups one after the other: a weight chunk holds the
// rows of KS / 2 whole groups (KS = 1: the first / second 32 pairs).  Over the voxels of a row (dbeta, dgamma): see the epilogue.  Only
// the fp64 atomics see another grouping (one per 64 voxels), as they see another order from run to run.
template <int KS>
__global__ void __launch_bounds__(RTHREADS, 2) conv1_dgrad_resident_kernel(const FpropArgs a) {
  static_assert(KS == 1 || KS == 2 || KS == 8, "conv1_dgrad_resident: K-split of a fprop_kernel 1x1x1 tile");
  constexpr int GPC = KS > 1 ? KS / 2 : 1, NPG = (RKC / 2) / GPC;      // groups per weight chunk, channel pairs of a group in a chunk
  // channel pair held by local pair `lp` of weight chunk `h`
  auto pair_of = [](int h, int lp) { return KS == 1 ? h * (RKC / 2) + lp : h * GPC + lp / NPG + (lp % NPG) * KS; };
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* coef = smem;              // [3][128]  p, q, r of the BN-backward prologue
  float* Zs = coef + R_COEF;       // [128][64] the resident operand
  float* Ws = Zs + R_Z;            // [64][64]  weight chunk
  float* Tb = Ws + R_W;            // [4][32][36] transposition tiles, one per wave
  float* ecoef = Tb + R_T;         // [2][5][64] per-row a, b, mean, rstd, gamma of the current / next step
  float* red = ecoef + R_E;        // [2][2][64] per-row partial sums (sum z, sum z*xhat) of the two voxel halves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  kernarg_warm<sizeof(FpropArgs)>();
  const int V = a.D * a.H * a.W, M = a.M;
  const int nt = (V + RVT - 1) / RVT;
  const int n = (int)blockIdx.x / nt, v0 = ((int)blockIdx.x - n * nt) * RVT;
  const int nsteps = (M + RMS - 1) / RMS;
  const int t_begin = (nsteps * (int)blockIdx.y) / (int)gridDim.y, t_end = (nsteps * ((int)blockIdx.y + 1)) / (int)gridDim.y;
  const int rep = blockIdx.x & ((a.nrep > 0 ? a.nrep : NREP) - 1);
  const float* in0n = a.in0 + (long)n * a.in0_ns + (long)a.in0_coff * V;
  const float* in1n = a.in1 + (long)n * a.in1_ns + (long)a.in1_coff * V;
  const float* exn = a.ex + (long)n * a.ex_ns + (long)a.ex_coff * V;
  float* outn = a.out + (long)n * a.out_ns + (long)a.out_coff * V;
  const int q4 = 4 * (lane & 7), rl = lane >> 3;              // epilogue: this lane's voxel quad and first row within a 32 x 32 tile
  const int vq = v0 + wn * 32 + q4;

  // NOTE: every load below is unconditional with a clamped address (fprop.hpp, "every load below is UNCONDITIONAL").
  const bool fast_gr = a.gr_in.st.nrep <= 2 && a.gr_in.s.nrep <= 2;
  const bool fast_e = a.ebn.training && a.ebn.st.nrep <= 2;
  BnBwdRaw raw_gr;
  BnFwdRaw raw_e;
  if (tid < RK && fast_gr) bn_bwd_issue(a.gr_in, tid, raw_gr);

  // (Loads past the workgroup's last step are issued all the same, every lane at element 0 of the tensor: the number of loads between
  // a load and its wait is then the same on every path, and the compiler's counted waits leave the younger loads in flight.)
  f32x4 wreg[4];
  auto load_w = [&](int t, int h) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int it = tid + i * RTHREADS, q = it & 15, kr = it >> 4;
      const bool ok = t < t_end && t * RMS + 4 * q < M;
      wreg[i] = *reinterpret_cast<const f32x4*>(ok ? a.w + (long)(2 * pair_of(h, kr >> 1) + (kr & 1)) * a.w_ld + t * RMS + 4 * q : a.w);
    }
  };
  auto store_w = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int it = tid + i * RTHREADS, q = it & 15;
      const bool ok = t * RMS + 4 * q < M;
      *reinterpret_cast<f32x4*>(Ws + 4 * it) = ok ? wreg[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  f32x4 xqA[4], gqA[4], xqB[4], gqB[4];      // epilogue operands of the even / odd steps (two sets: statically indexed registers)
  auto load_xg = [&](int t, f32x4 (&xq)[4], f32x4 (&gq)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int m = t * RMS + wm * 32 + rl + 8 * k;
      const unsigned off = (t < t_end && m < M && vq < V) ? (unsigned)m * (unsigned)V + (unsigned)vq : 0u;
      xq[k] = *reinterpret_cast<const f32x4*>(exn + off);
      gq[k] = *reinterpret_cast<const f32x4*>(outn + off);
    }
  };
  auto ecoef_issue = [&](int t) {
    if (tid < RMS && fast_e) bn_fwd_issue(a.ebn, min(t * RMS + tid, M - 1), raw_e);
  };
  auto ecoef_finish = [&](int t) {
    if (tid < RMS) EpiRow<RMS>{ecoef + (t & 1) * (5 * RMS) + tid}.fill(fast_e, a.ebn, raw_e, t * RMS + tid, t * RMS + tid < M);
  };

  // ---- prologue: everything the first step needs goes out in one batch, the coefficient arithmetic runs when the statistics are back ----
  load_w(t_begin, 0);
  f32x4 z0[8], z1[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int it = tid + i * RTHREADS, q = it & 15, k = it >> 4;
    const int off = (v0 + 4 * q < V) ? k * V + v0 + 4 * q : 0;
    z0[i] = *reinterpret_cast<const f32x4*>(in0n + off);
    z1[i] = *reinterpret_cast<const f32x4*>(in1n + off);
  }
  ecoef_issue(t_begin);
  if (tid < RK) pro_coef(coef, RK, tid, true, fast_gr, a.gr_in, raw_gr, drop_scale(a.drop_in, n, tid));
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int it = tid + i * RTHREADS, q = it & 15, k = it >> 4;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pro_apply<PRO_GRAD>(coef, RK, k, z0[i][e], z1[i][e]);
    if (!(v0 + 4 * q < V)) o = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(Zs + 4 * it) = o;
  }
  ecoef_finish(t_begin);
  store_w(t_begin);
  // The epilogue operands of the first step leave AFTER the waits above (the memory counter retires in order: issued earlier they
  // would be waited for with the weights), and are in flight under the first chunk's MFMAs.
  load_xg(t_begin, xqA, gqA);
  // the NEXT launch's weights (FpropArgs::pf_ptr), consumed at the very end: nothing waits for these
  float pf_sink = 0.f, pf_sink2 = 0.f;
  prefetch_weight_lines(a, blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y, RTHREADS, tid, pf_sink, pf_sink2);

  f32x16 acc, partA, partB;
  // 32 MFMAs over weight chunk h; the operand reads of step s+1 are issued before the MFMA of step s (fprop_kernel, mfma_chunk).
  // KS > 1: a group's chain starts from zero in partA / partB (alternating, so that the sum of the finished group into `acc` does not
  // wait behind its last MFMA but runs two MFMAs into the next group); groups are added in group order.
  auto mfma_chunk = [&](int h) {
    const float* zb = Zs + half * RVT + wn * 32 + l31;
    const float* wb = Ws + half * RMS + wm * 32 + l31;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto fold = [&](int g, const f32x16& p) {
      if (h == 0 && g == 0) acc = p;
      else acc += p;
    };
    auto mm = [&](int lp, float av, float bv) {
      if constexpr (KS == 1) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
      } else {
        const int g = lp / NPG, j = lp % NPG;
        if (g & 1) partB = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, j == 0 ? zero : partB, 0, 0, 0);
        else partA = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, j == 0 ? zero : partA, 0, 0, 0);
        if (g > 0 && j == 1) fold(g - 1, (g & 1) ? partA : partB);
        if (g == GPC - 1 && j == NPG - 1) fold(g, (g & 1) ? partB : partA);
      }
    };
    float a0, b0, a1, b1;
    a0 = wb[0]; b0 = zb[pair_of(h, 0) * 2 * RVT];
#pragma unroll
    for (int s = 0; s < RKC / 2; s += 2) {
      a1 = wb[(s + 1) * 2 * RMS]; b1 = zb[pair_of(h, s + 1) * 2 * RVT];
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      mm(s, a0, b0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if (s + 2 < RKC / 2) { a0 = wb[(s + 2) * 2 * RMS]; b0 = zb[pair_of(h, s + 2) * 2 * RVT]; }
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      mm(s + 1, a1, b1);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    }
  };
  // per-row sums of step t: the two voxel halves in fp64, then the atomics (flush_row_sums with two per-wave partials)
  auto flush_sums = [&](int t) {
    const int m = t * RMS + tid;
    if (tid < RMS && m < M)
      flush_row_sums<EPI_MASK_ACCUM, 2>(a, rep, m, red + tid, red + 2 * RMS + tid, RMS, EpiRow<RMS>{ecoef + (t & 1) * (5 * RMS) + tid}.gamma());
  };

  // One row step.  `xq` / `gq`: this step's epilogue operands (complete by now), `xn` / `gn`: the set the NEXT step's are loaded into.
  // The memory counter retires in order, so the order of issue decides what a wait drains: the next step's X and G loads go out right
  // behind the second weight chunk's, whose wait (counted: 8 younger loads) leaves them in flight; they are drained by the wait for
  // the next step's first weight chunk at the end of this step's epilogue, i.e. they fly under both MFMA phases of this step.
  auto step = [&](int t, f32x4 (&xq)[4], f32x4 (&gq)[4], f32x4 (&xn)[4], f32x4 (&gn)[4]) {
    if constexpr (KS == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
    __syncthreads();                     // chunk 0 of the step (written by the prologue / the previous step's epilogue) is visible
    if (t > t_begin) flush_sums(t - 1);
    if (t + 1 < t_end) ecoef_issue(t + 1);
    load_w(t, 1);
    load_xg(t + 1, xn, gn);
    mfma_chunk(0);
    if (t + 1 < t_end) ecoef_finish(t + 1);
    __syncthreads();
    store_w(t);
    __syncthreads();
    load_w(t + 1, 0);
    mfma_chunk(1);
    __syncthreads();
    // ---- epilogue of the step: transposed through the wave's LDS tile so that a lane holds 4 consecutive voxels of 4 rows ----
    float* e = ecoef + (t & 1) * (5 * RMS);
    float* tb = Tb + wave * (32 * RTS);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) tb[acc_row(r, half) * RTS + l31] = acc[r];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f32x4 o[4];
    unsigned off[4];
    bool ok[4];
    float zs[4][4], xhs[4][4];       // z and xhat of this lane's elements, zero where out of range
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ml = wm * 32 + rl + 8 * k, m = t * RMS + ml;
      const f32x4 vt = *reinterpret_cast<const f32x4*>(tb + (rl + 8 * k) * RTS + q4);
      ok[k] = m < M && vq < V;
      off[k] = ok[k] ? (unsigned)m * (unsigned)V + (unsigned)vq : 0u;
      const EpiRow<RMS> er{e + ml};
      const float ea = er.a(), eb = er.b(), mu = er.mean(), rs = er.rstd(), gm = er.gamma();
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float z, xh;
        mask_elem(ea, eb, mu, rs, xq[k][c], vt[c], z, xh);
        z = ok[k] ? z : 0.f;
        zs[k][c] = z;
        xhs[k][c] = ok[k] ? xh : 0.f;
        o[k][c] = gq[k][c] + gm * z;
      }
      if constexpr (KS > 1) {
        // fprop_kernel's small tiles hold one voxel per lane and sum a row's 32 voxels with half_reduce_n: voxel ^ 16, ^ 8, ^ 4 (lanes
        // ^ 4, ^ 2, ^ 1 here, element by element), then voxel ^ 2 and ^ 1 (within the lane)
        float s0[4], s1[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          s0[c] = zs[k][c]; s1[c] = zs[k][c] * xhs[k][c];
          s0[c] += swz_xor<4>(s0[c]); s1[c] += swz_xor<4>(s1[c]);
          s0[c] += swz_xor<2>(s0[c]); s1[c] += swz_xor<2>(s1[c]);
          s0[c] += swz_xor<1>(s0[c]); s1[c] += swz_xor<1>(s1[c]);
        }
        const float t0 = (s0[0] + s0[2]) + (s0[1] + s0[3]), t1 = (s1[0] + s1[2]) + (s1[1] + s1[3]);
        if ((lane & 7) == 0) {
          red[wn * RMS + ml] = t0;
          red[2 * RMS + wn * RMS + ml] = t1;
        }
      }
    }
    if constexpr (KS == 1) {
      // fprop_kernel's 128-voxel tile: a lane runs through its 4 voxels of the tile's first 32-voxel column and then through the 4 of
      // the second one, which the wave beside this one holds here, and the 8 lanes of a row follow (^ 1, ^ 2, ^ 4).  The second wave's
      // values cross through the pair's transposition tiles, which both waves have read by the first barrier.
      float* xb = Tb + (wm * 2) * (32 * RTS);
      __syncthreads();
      if (wn == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int c = 0; c < 4; ++c) { xb[((k * 4 + c) * 2) * 64 + lane] = zs[k][c]; xb[((k * 4 + c) * 2 + 1) * 64 + lane] = xhs[k][c]; }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ml = wm * 32 + rl + 8 * k;
        float t0 = 0.f, t1 = 0.f;
        if (wn == 0) {
#pragma unroll
          for (int c = 0; c < 4; ++c) { t0 += zs[k][c]; t1 += zs[k][c] * xhs[k][c]; }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float z = xb[((k * 4 + c) * 2) * 64 + lane], xh = xb[((k * 4 + c) * 2 + 1) * 64 + lane];
            t0 += z; t1 += z * xh;
          }
          quad_row_sum(t0, t1);
        }
        if ((lane & 7) == 0) {
          red[wn * RMS + ml] = t0;
          red[2 * RMS + wn * RMS + ml] = t1;
        }
      }
    }
    // Every load of the step is ahead of its stores (fprop.hpp, "issued BEFORE the stores").  The next step's first weight chunk goes
    // to LDS here: every wave is past the last barrier of this step's MFMAs.
    store_w(t + 1);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ok[k]) *reinterpret_cast<f32x4*>(outn + off[k]) = o[k];
  };
  for (int t = t_begin; t < t_end; t += 2) {
    step(t, xqA, gqA, xqB, gqB);
    if (t + 1 < t_end) step(t + 1, xqB, gqB, xqA, gqA);
  }
  __syncthreads();
  flush_sums(t_end - 1);
  prefetch_sink(a, pf_sink, pf_sink2);
}
#endif  // __HIPCC__

// Shape half of the eligibility rule (no pointers: the plan's "#conv1_dgrad_resident" counter uses it as well).  `mode` is the plan
// option: 0 never, 1 where the kernel measured faster than fprop_kernel, 2 wherever the kernel can run (tests, measurements).
bool conv1_dgrad_resident_shape_ok(int mode, int N, long V, int Cin, int M, int w_ld) {
  if (mode == 0 || N <= 0 || V <= 0) return false;
  if (Cin != RK || (V & 3) != 0 || (M & 3) != 0 || (w_ld & 3) != 0 || (long)(M + RK) * V >= (1l << 31)) return false;
  if ((long)N * cdiv(V, RVT) >= (1l << 31) / RTHREADS) return false;
  // Option 1: only where the kernel measured faster than fprop_kernel (profiles/r06_conv1_dgrad_ab.txt, 2 x 128^3, per launch, rocprofv3):
  //   4^3  (2 tiles, 8-16 row groups):     6.1-8.4 -> 8.2-10.9 us on all 16 layers: 32 workgroups at the most, each a full K = 128 chain,
  //                                        against fprop_kernel's cross-workgroup K-split.  Left alone: V < 512.
  //   8^3  (16 tiles, 4-16 row groups):    10.1-16.4 -> 8.8-10.5 us on 23 of 24 layers (cin = 256: 7.6 -> 8.9), class 11.9 -> 9.3 us.
  //   16^3 (128 tiles, 2-4 row groups):    13.6-28.9 -> 12.8-24.2 us on all 12 layers, class 23.2 -> 18.6 us.
  //   32^3 (1024 tiles, two rounds):       cin 64 / 96 / 128 (ONE row tile in fprop_kernel, nothing fetched twice) 37 / 40 / 44 -> 42 / 56 / 57 us,
  //                                        cin 160 / 192 / 224: 71 / 75 / 78 -> 70 / 74 / 85 us.  Left alone: more tiles than fill the chip once.
  if (mode == 1 && (V < 512 || (long)N * cdiv(V, RVT) > R_FILL)) return false;
  return true;
}

bool conv1_dgrad_resident_eligible(const FpropArgs& a) {
  const long V = (long)a.D * a.H * a.W;
  if (!conv1_dgrad_resident_shape_ok(a.conv1_dgrad_resident, a.N, V, a.Cin, a.M, a.w_ld)) return false;
  if (!a.in0 || !a.in1 || !a.ex || !a.out || !a.w || !a.dgamma || !a.dbeta || !a.s_acc.sum || !a.s_acc.sq) return false;
  const uintptr_t ptrs = (uintptr_t)a.in0 | (uintptr_t)a.in1 | (uintptr_t)a.ex | (uintptr_t)a.out | (uintptr_t)a.w;
  const long strides = a.in0_ns | a.in1_ns | a.ex_ns | a.out_ns;      // channel offsets are multiples of V, itself a multiple of 4
  return (ptrs & 15) == 0 && (strides & 3) == 0;
}

template <int KS>
static int launch_ks(const FpropArgs& a, dim3 grid, hipStream_t stream) {
  if (int rc = allow_dynamic_lds<conv1_dgrad_resident_kernel<KS>>(R_SMEM)) return rc;
  MMNN_LAUNCH(conv1_dgrad_resident_kernel<KS>, grid, dim3(RTHREADS), R_SMEM, stream, a);
  MMNN_HIP(hipGetLastError());
  return 0;
}

int launch_conv1_dgrad_resident(const FpropArgs& a, hipStream_t stream) {
  MMNN_REQUIRE(conv1_dgrad_resident_eligible(a), "conv1_dgrad_resident: shape not eligible");
  const long V = (long)a.D * a.H * a.W;
  const long tiles = (long)a.N * cdiv(V, RVT);
  const int nsteps = cdiv(a.M, RMS);
  // row groups: as many as it takes to fill the chip once (two workgroups per CU), never more than there are row steps
  const int rg = (int)std::min<long>(nsteps, std::max<long>(1, R_FILL / tiles));
  // the order of the sums follows the tile that dispatch<1, ...> (fprop_dispatch.hpp) gives this shape, same thresholds
  const long blocks_a = (long)a.N * cdiv(V, 128) * cdiv(a.M, 128), blocks_b = (long)a.N * cdiv(V, 64) * cdiv(a.M, 64);
  const dim3 grid((unsigned)tiles, (unsigned)rg);
  if (blocks_a >= 192) return launch_ks<1>(a, grid, stream);
  if (blocks_b >= 192) return launch_ks<2>(a, grid, stream);
  return launch_ks<8>(a, grid, stream);
}

}  // namespace mmnn
