// Launch plan of the DenseNet backbone forward / backward (see densenet.hpp).
#include "densenet.hpp"

#include <string.h>

#include <algorithm>

#include "fprop.hpp"
#include "stem.hpp"
#include "wgrad.hpp"

namespace mmnn {

// cross-block K-split scratch of the plan's workspace: <= 512 blocks x (up to 4) 32x32 partial tiles, + per-tile counters
constexpr size_t KZ_PART_BYTES = (size_t)512 * 4 * 1024 * sizeof(float);
constexpr unsigned KZ_CNT_ENTRIES = 4096;

namespace {
struct Panel { const float* p; unsigned bytes; };   // a weight panel in device memory
// Everything the backward of dense layer (b, l) binds (layer_bind).  The data gradients (plan_backward_range) and the weight gradients
// (layer_wgrad_args) both take it from here: the operand of a data gradient IS the g0 / g1 / gr of the same convolution's weight gradient.
struct LayerBind {
  BnFwd bn1, bn2;          // norm1 / norm2 on batch statistics
  BnBwd gr_new, gr_t1;     // BN-backward of the layer's own concat channels (gammas folded into G) / of T1 (single consumer norm2)
  StatPtr dg1, dg2, s_x;   // dgamma/dbeta sums of norm1 / norm2; S1 / S2 of the concat buffer
  View x, g;               // concat buffer and its gradient from channel 0: what norm1 / conv1 see
  View x_new, g_new;       // the same from the layer's own channels on: what conv2 wrote
  View t1, dz2;            // conv1 output; gradient wrt the norm2 output (ReLU mask applied)
};
}  // namespace

// Floats of one weight tensor: conv1 [mid][cin], conv2 [growth][mid][27], transition conv [cout][cin].  The raw weights, their packed
// fp32 panel and one weight-gradient slab all have this size; the pre-split bf16 conv2 panel holds three 2-byte pieces of every weight.
static long conv1_elems(const Plan& p, int cin) { return (long)p.mid * cin; }
static long conv2_elems(const Plan& p) { return (long)p.cfg.growth * p.mid * 27; }
static long trans_elems(const TransOff& t) { return (long)t.cout * t.cin; }
static size_t conv2_split_bytes(const Plan& p) { return (size_t)3 * conv2_elems(p) * sizeof(uint16_t); }

int plan_build(Plan& p, const NetCfg& cfg, int N, int D, int H, int W) {
  MMNN_REQUIRE(cfg.nblocks >= 1 && cfg.nblocks <= MAX_BLOCKS, "plan: 1..%d dense blocks supported, got %d", MAX_BLOCKS, cfg.nblocks);
  MMNN_REQUIRE(cfg.in_channels >= 1 && cfg.in_channels <= 4, "plan: in_channels must be 1..4, got %d", cfg.in_channels);
  MMNN_REQUIRE(cfg.init_features >= 1 && cfg.init_features <= 64, "plan: init_features must be <= 64, got %d", cfg.init_features);
  MMNN_REQUIRE(cfg.growth >= 1 && cfg.growth <= 32, "plan: growth_rate must be <= 32, got %d", cfg.growth);
  MMNN_REQUIRE(cfg.bn_size >= 1 && cfg.dropout_p >= 0.f && cfg.dropout_p < 1.f, "plan: bad bn_size / dropout");
  MMNN_REQUIRE(N >= 1 && D >= 1 && H >= 1 && W >= 1, "plan: bad input extent");
  p.cfg = cfg; p.N = N; p.D = D; p.H = H; p.W = W;
  p.mid = cfg.bn_size * cfg.growth;
  p.D0 = (D - 1) / 2 + 1; p.H0 = (H - 1) / 2 + 1; p.W0 = (W - 1) / 2 + 1;
  int d = (p.D0 - 1) / 2 + 1, h = (p.H0 - 1) / 2 + 1, w = (p.W0 - 1) / 2 + 1;
  int c = cfg.init_features;
  for (int b = 0; b < cfg.nblocks; ++b) {
    MMNN_REQUIRE(cfg.block_layers[b] >= 1, "plan: empty dense block %d", b);
    MMNN_REQUIRE(d >= 1 && h >= 1 && w >= 1, "plan: input too small, block %d has no voxels", b + 1);
    p.Db[b] = d; p.Hb[b] = h; p.Wb[b] = w; p.Vb[b] = d * h * w;
    p.cin_b[b] = c;
    // replicas of the fp64 statistics (StatPtr::nrep): block 0 receives the stem's statistics (always NREP replicas)
    p.nrep_b[b] = (b == 0 || (long)N * d * h * w >= 32768) ? NREP : ((long)N * d * h * w >= 4096 ? 2 : 1);
    p.ctot_b[b] = c + cfg.block_layers[b] * cfg.growth;
    c = p.ctot_b[b];
    if (b != cfg.nblocks - 1) {
      MMNN_REQUIRE(c % 2 == 0, "plan: transition halves an odd channel count");
      c /= 2; d /= 2; h /= 2; w /= 2;
    }
  }
  // ---- parameter layout (PyTorch named_parameters order of `backbone`) ----
  long po = 0, ro = 0;
  int nbn = 0;
  auto bn = [&](int ch, long& w_, long& b_, long& m_, long& v_) { w_ = po; po += ch; b_ = po; po += ch; m_ = ro; ro += ch; v_ = ro; ro += ch; ++nbn; };
  p.p_conv0 = po; po += (long)cfg.init_features * cfg.in_channels * 343;
  bn(cfg.init_features, p.p_n0w, p.p_n0b, p.r_n0m, p.r_n0v);
  p.layers.assign(cfg.nblocks, {});
  p.trans.clear();
  for (int b = 0; b < cfg.nblocks; ++b) {
    int ci = p.cin_b[b];
    for (int l = 0; l < cfg.block_layers[b]; ++l) {
      LayerOff lo;
      lo.cin = ci;
      bn(ci, lo.n1w, lo.n1b, lo.r1m, lo.r1v);
      lo.c1 = po; po += conv1_elems(p, ci);
      bn(p.mid, lo.n2w, lo.n2b, lo.r2m, lo.r2v);
      lo.c2 = po; po += conv2_elems(p);
      p.layers[b].push_back(lo);
      ci += cfg.growth;
    }
    if (b != cfg.nblocks - 1) {
      TransOff t;
      t.cin = ci; t.cout = ci / 2;
      bn(ci, t.nw, t.nb, t.rm, t.rv);
      t.cw = po; po += trans_elems(t);
      p.trans.push_back(t);
    } else {
      bn(ci, p.p_n5w, p.p_n5b, p.r_n5m, p.r_n5v);
    }
  }
  p.n_params = po; p.n_runstats = ro; p.n_bn = nbn;

  // ---- workspace ----
  Carver cv;
  const int nb = cfg.nblocks;
  const size_t F = sizeof(float);
  const long V0 = (long)p.D0 * p.H0 * p.W0;
  p.o_conv0 = cv.take((size_t)N * cfg.init_features * V0 * F);
  p.o_idx = cv.take((size_t)N * cfg.init_features * p.Vb[0]);
  p.o_t1.assign(nb, {});
  size_t dap = 0;
  for (int b = 0; b < nb; ++b) {
    p.o_x[b] = cv.take((size_t)N * p.ctot_b[b] * p.Vb[b] * F);
    p.o_g[b] = cv.take((size_t)N * p.ctot_b[b] * p.Vb[b] * F);
    for (int l = 0; l < cfg.block_layers[b]; ++l) p.o_t1[b].push_back(cv.take((size_t)N * p.mid * p.Vb[b] * F));
    if (b != nb - 1) {
      p.o_ap[b] = cv.take((size_t)N * p.ctot_b[b] * p.Vb[b + 1] * F);
      dap = std::max(dap, (size_t)N * p.ctot_b[b] * p.Vb[b + 1] * F);
    } else {
      p.o_ap[b] = 0;
    }
  }
  p.o_dap = cv.take(dap ? dap : 256);
  p.o_dz0 = cv.take((size_t)N * cfg.init_features * V0 * F);
  // forward statistics (fp64, zeroed at the start of every training forward)
  const size_t PAIR = 2 * NREP * sizeof(double);
  p.o_fstat = cv.cur;
  p.o_st_conv0 = cv.take(PAIR * cfg.init_features);
  p.o_st_t1.assign(nb, {});
  for (int b = 0; b < nb; ++b) {
    p.o_st_x[b] = cv.take(PAIR * p.ctot_b[b]);
    for (int l = 0; l < cfg.block_layers[b]; ++l) p.o_st_t1[b].push_back(cv.take(PAIR * p.mid));
  }
  p.fstat_bytes = cv.cur - p.o_fstat;
  // backward statistics (fp64, zeroed at the start of every backward)
  p.o_bstat = cv.cur;
  p.o_dg_n0 = cv.take(PAIR * cfg.init_features);
  p.o_dg_n1.assign(nb, {}); p.o_dg_n2.assign(nb, {}); p.o_dg_tr.clear();
  for (int b = 0; b < nb; ++b) {
    p.o_s_x[b] = cv.take(PAIR * p.ctot_b[b]);
    for (int l = 0; l < cfg.block_layers[b]; ++l) {
      p.o_dg_n1[b].push_back(cv.take(PAIR * p.layers[b][l].cin));
      p.o_dg_n2[b].push_back(cv.take(PAIR * p.mid));
    }
    if (b != nb - 1) p.o_dg_tr.push_back(cv.take(PAIR * p.ctot_b[b]));
  }
  p.o_dg_n5 = cv.take(PAIR * p.ctot_b[nb - 1]);
  p.bstat_bytes = cv.cur - p.o_bstat;
  // packed weights
  p.o_pk_conv0 = cv.take((size_t)7 * stem_krows(cfg.in_channels) * 64 * F);
  p.o_pk_c1.assign(nb, {}); p.o_pk_c2f.assign(nb, {}); p.o_pk_c2b.assign(nb, {}); p.o_pk_tr.clear();
  p.o_pk_c2f3.assign(nb, {}); p.o_pk_c2b3.assign(nb, {});
  p.x3_bytes = 0;
  for (int b = 0; b < nb; ++b) {
    // the conv2 launches of this block that run on the three-piece bf16 kernels get their weights pre-split, and the plane scratch
    // is sized for the largest of them
    FpropArgs f, g;
    memset(&f, 0, sizeof(f));
    f.N = N; f.D = p.Db[b]; f.H = p.Hb[b]; f.W = p.Wb[b];
    g = f;
    f.Cin = p.mid; f.M = cfg.growth;
    g.Cin = cfg.growth; g.M = p.mid;
    const bool f3 = conv3_fwd_bf16x3_eligible(f), b3 = conv3_dgrad_bf16x3_eligible(g);
    if (f3) p.x3_bytes = std::max(p.x3_bytes, conv3_bf16x3_plane_bytes(f));
    if (b3) p.x3_bytes = std::max(p.x3_bytes, conv3_bf16x3_plane_bytes(g));
    for (int l = 0; l < cfg.block_layers[b]; ++l) {
      p.o_pk_c1[b].push_back(cv.take(conv1_elems(p, p.layers[b][l].cin) * F));
      p.o_pk_c2f[b].push_back(cv.take(conv2_elems(p) * F));
      p.o_pk_c2b[b].push_back(cv.take(conv2_elems(p) * F));
      p.o_pk_c2f3[b].push_back(f3 ? cv.take(conv2_split_bytes(p)) : 0);
      p.o_pk_c2b3[b].push_back(b3 ? cv.take(conv2_split_bytes(p)) : 0);
    }
    if (b != nb - 1) p.o_pk_tr.push_back(cv.take(trans_elems(p.trans[b]) * F));
  }
  p.o_x3 = p.x3_bytes ? cv.take(p.x3_bytes) : 0;
  // weight-gradient slabs
  p.ns_conv0 = stem_wgrad_pick_splits(N, p.D0, p.H0, p.W0, cfg.in_channels);
  p.o_sl_conv0 = cv.take((size_t)p.ns_conv0 * cfg.in_channels * cfg.init_features * 352 * F);
  p.o_sl_c1.assign(nb, {}); p.o_sl_c2.assign(nb, {}); p.ns_c1.assign(nb, {}); p.ns_c2.assign(nb, {});
  p.o_sl_tr.clear(); p.ns_tr.clear();
  // The weight gradients of a dense block go out together once its data-gradient chain has ended: one launch per kernel variant,
  // and the voxel splits -- hence the partial slabs `finalize` has to read back -- shrink by the number of layers that share it.
  for (int b = 0; b < nb; ++b) {
    for (int l = 0; l < cfg.block_layers[b]; ++l) {
      const int ci = p.layers[b][l].cin;
      // conv1: a launch covers the layers of the block that use the same channel-group width; `pairs` = its (layer, channel
      // group) pairs, so that every block of the launch walks the same number of voxel chunks
      int pairs = 0;
      {
        const int cw = wgrad1_channel_width(ci, p.Vb[b]);
        for (int k = 0; k < cfg.block_layers[b]; ++k)
          if (wgrad1_channel_width(p.layers[b][k].cin, p.Vb[b]) == cw) pairs += cdiv(p.layers[b][k].cin, cw);
      }
      const int s1 = wgrad_pick_splits(1, N, p.Db[b], p.Hb[b], p.Wb[b], p.mid, ci, pairs);
      const int s2 = wgrad_pick_splits(27, N, p.Db[b], p.Hb[b], p.Wb[b], cfg.growth, p.mid, cfg.block_layers[b]);
      p.ns_c1[b].push_back(s1); p.ns_c2[b].push_back(s2);
      p.o_sl_c1[b].push_back(cv.take(s1 * conv1_elems(p, ci) * F));
      p.o_sl_c2[b].push_back(cv.take(s2 * conv2_elems(p) * F));
    }
    if (b != nb - 1) {
      const int s = wgrad_pick_splits(1, N, p.Db[b + 1], p.Hb[b + 1], p.Wb[b + 1], p.trans[b].cout, p.trans[b].cin);
      p.ns_tr.push_back(s);
      p.o_sl_tr.push_back(cv.take(s * trans_elems(p.trans[b]) * F));
    }
  }
  // dZ2 (gradient wrt the norm2 output) of every layer has its own buffer: the block's batched conv1 weight gradient reads every
  // layer's dZ2 after the data-gradient chain has passed them all.
  for (int b = 0; b < nb; ++b) p.o_dz2[b] = cv.take((size_t)cfg.block_layers[b] * N * p.mid * p.Vb[b] * F);
  // cross-block K-split scratch: <= 512 blocks x (up to 4) 32x32 partial tiles, + per-tile counters
  p.o_kz_part = cv.take(KZ_PART_BYTES);
  p.o_kz_cnt = cv.take(KZ_CNT_ENTRIES * sizeof(unsigned));
  // job tables
  int nlayers = 0;
  for (int b = 0; b < nb; ++b) nlayers += cfg.block_layers[b];
  p.n_run_jobs = nbn;
  p.n_pack_jobs = 1 + 5 * nlayers + (nb - 1);             // (an upper bound: kinds 5 / 6 only for the bf16x3 layers)
  p.n_grad_jobs = 3 + 6 * nlayers + 3 * (nb - 1) + 2;
  p.o_jobs_run = cv.take(sizeof(RunStatJob) * p.n_run_jobs);
  p.o_jobs_pack = cv.take(sizeof(PackJob) * p.n_pack_jobs);
  p.o_jobs_grad = cv.take(sizeof(GradJob) * p.n_grad_jobs);
  p.n_layers = nlayers;
  p.o_wg_table = cv.take(sizeof(WgradArgs) * 2 * nlayers);     // [conv2 of every layer][conv1 of every layer], see plan_backward
  p.ws_bytes = cv.cur;
  p.host_jobs_bytes = p.o_wg_table - p.o_jobs_run;
  if (p.host_jobs) { (void)hipHostFree(p.host_jobs); p.host_jobs = nullptr; }   // (re)allocated lazily by the first forward
  p.tab_params = nullptr; p.tab_run = nullptr; p.tab_ws = nullptr;
  return 0;
}

void plan_free(Plan& p) {
  if (p.host_jobs) (void)hipHostFree(p.host_jobs);
  p.host_jobs = nullptr;
  if (p.wg_pinned) (void)hipHostFree(p.wg_pinned);
  p.wg_pinned = nullptr;
  for (hipEvent_t e : p.timer_ev) (void)hipEventDestroy(e);
  p.timer_ev.clear();
}

// ---- the batch-norm sites (densenet.hpp: NormSite) -----------------------------------------------------------------------
// a site on dense block b's concat buffer: channels [0, C) of the block's statistics row
static NormSite concat_site(const Plan& p, int b, int C, long w, long bb, long rm, long rv, size_t o_dg) {
  return {p.o_st_x[b], p.o_s_x[b], o_dg, p.ctot_b[b], 0, C, p.nrep_b[b], w, bb, rm, rv, (double)p.N * p.Vb[b]};
}
static NormSite norm0(const Plan& p) {   // on the stem convolution's output: its statistics always use NREP replicas
  const int C = p.cfg.init_features;
  return {p.o_st_conv0, p.o_dg_n0, p.o_dg_n0, C, 0, C, NREP, p.p_n0w, p.p_n0b, p.r_n0m, p.r_n0v, (double)p.N * p.D0 * p.H0 * p.W0};
}
static NormSite norm1(const Plan& p, int b, int l) {
  const LayerOff& lo = p.layers[b][l];
  return concat_site(p, b, lo.cin, lo.n1w, lo.n1b, lo.r1m, lo.r1v, p.o_dg_n1[b][l]);
}
static NormSite norm2(const Plan& p, int b, int l) {   // on T1, the layer's conv1 output
  const LayerOff& lo = p.layers[b][l];
  return {p.o_st_t1[b][l], p.o_dg_n2[b][l], p.o_dg_n2[b][l], p.mid, 0, p.mid, p.nrep_b[b], lo.n2w, lo.n2b, lo.r2m, lo.r2v, (double)p.N * p.Vb[b]};
}
static NormSite transition(const Plan& p, int b) {
  const TransOff& t = p.trans[b];
  return concat_site(p, b, t.cin, t.nw, t.nb, t.rm, t.rv, p.o_dg_tr[b]);
}
static NormSite norm5(const Plan& p) {
  const int b = p.cfg.nblocks - 1;
  return concat_site(p, b, p.ctot_b[b], p.p_n5w, p.p_n5b, p.r_n5m, p.r_n5v, p.o_dg_n5);
}

static StatPtr statptr(char* ws, size_t o, int C, int off, int nrep) {
  StatPtr s; memset(&s, 0, sizeof(s));
  s.sum = reinterpret_cast<double*>(ws + o); s.sq = s.sum + (long)NREP * C;
  s.stride = C; s.off = off; s.nrep = nrep;
  return s;
}
// What the kernels read and write at a site.  `first` moves the window along the row: the concat channels behind the ones the site sees.
// The producer of the tensor passes `training`: an eval forward accumulates no statistics (null sum).
static StatPtr stats(char* ws, const NormSite& s, int first = 0, int training = 1) {
  StatPtr st = statptr(ws, s.o_st, s.stride, s.off + first, s.nrep);
  if (!training) st.sum = nullptr;
  return st;
}
static StatPtr sums(char* ws, const NormSite& s, int first = 0) { return statptr(ws, s.o_s, s.stride, s.off + first, s.nrep); }     // S1 / S2
static StatPtr dgsums(char* ws, const NormSite& s) { return statptr(ws, s.o_dg, s.C, 0, s.nrep); }      // .sum = dbeta, .sq = dgamma
static BnFwd bnfwd(const Plan& p, char* ws, const float* params, float* run, const NormSite& s, int training) {
  BnFwd f; memset(&f, 0, sizeof(f));
  f.st = stats(ws, s);
  f.rmean = run + s.rm; f.rvar = run + s.rv; f.gamma = params + s.w; f.beta = params + s.b;
  f.inv_count = 1.0 / s.count; f.eps = p.cfg.eps; f.training = training;
  return f;
}
static BnBwd bnbwd(const Plan& p, char* ws, const float* params, const NormSite& s, int first = 0) {   // of the tensor's channels [first, ...)
  BnBwd g; memset(&g, 0, sizeof(g));
  g.st = stats(ws, s, first); g.s = sums(ws, s, first);
  g.gamma = s.o_s == s.o_dg ? params + s.w : nullptr;   // single consumer: scaled by its gamma here; concat: already folded into G
  g.inv_count = 1.0 / s.count; g.eps = p.cfg.eps;
  return g;
}

// ---- tensor views (densenet.hpp: View) and where they go in the argument structs --------------------------------------------
static float* fptr(char* ws, size_t o) { return reinterpret_cast<float*>(ws + o); }
static View concat(const Plan& p, char* ws, int b, int coff = 0) { return {fptr(ws, p.o_x[b]), (long)p.ctot_b[b] * p.Vb[b], coff}; }
static View concat_grad(const Plan& p, char* ws, int b, int coff = 0) { return {fptr(ws, p.o_g[b]), (long)p.ctot_b[b] * p.Vb[b], coff}; }
static View t1(const Plan& p, char* ws, int b, int l) { return {fptr(ws, p.o_t1[b][l]), (long)p.mid * p.Vb[b], 0}; }
static View dz2(const Plan& p, char* ws, int b, int l) { return {fptr(ws, p.o_dz2[b]) + (long)l * p.N * p.mid * p.Vb[b], (long)p.mid * p.Vb[b], 0}; }
// block b's transition input on block b + 1's grid (normalised, pooled), and the gradient wrt it (one buffer for every transition)
static View pooled(const Plan& p, char* ws, int b) { return {fptr(ws, p.o_ap[b]), (long)p.ctot_b[b] * p.Vb[b + 1], 0}; }
static View pooled_grad(const Plan& p, char* ws, int b) { return {fptr(ws, p.o_dap), (long)p.ctot_b[b] * p.Vb[b + 1], 0}; }

static void set_in0(FpropArgs& a, View v) { a.in0 = v.p; a.in0_ns = v.ns; a.in0_coff = v.coff; }
static void set_in1(FpropArgs& a, View v) { a.in1 = v.p; a.in1_ns = v.ns; a.in1_coff = v.coff; }
static void set_out(FpropArgs& a, View v) { a.out = v.p; a.out_ns = v.ns; a.out_coff = v.coff; }
static void set_ex(FpropArgs& a, View v) { a.ex = v.p; a.ex_ns = v.ns; a.ex_coff = v.coff; }
static void set_g0(WgradArgs& a, View v) { a.g0 = v.p; a.g0_ns = v.ns; a.g0_coff = v.coff; }
static void set_g1(WgradArgs& a, View v) { a.g1 = v.p; a.g1_ns = v.ns; a.g1_coff = v.coff; }
static void set_x(WgradArgs& a, View v) { a.x = v.p; a.x_ns = v.ns; a.x_coff = v.coff; }

// ---- weight panels: each is the `w` / `w3` of its own launch and the prefetch hint (FpropArgs::pf_ptr) of the launch before it -------
static Panel conv1_panel(const Plan& p, char* ws, int b, int l) { return {fptr(ws, p.o_pk_c1[b][l]), (unsigned)(sizeof(float) * conv1_elems(p, p.layers[b][l].cin))}; }
static Panel trans_panel(const Plan& p, char* ws, int b) { return {fptr(ws, p.o_pk_tr[b]), (unsigned)(sizeof(float) * trans_elems(p.trans[b]))}; }
// conv1 as the parameters hold it, [m][c]: what its data gradient reads
static Panel conv1_weights(const Plan& p, const float* params, int b, int l) { return {params + p.layers[b][l].c1, (unsigned)(sizeof(float) * conv1_elems(p, p.layers[b][l].cin))}; }
// conv2 of the forward (pack kinds 1 / 5) or of the data gradient (kinds 2 / 6).  A layer on the three-piece bf16 kernels has a pre-split
// panel beside the fp32 one, and its launch reads that one; `fp32` asks for the fp32 panel whatever the kernel.
static Panel conv2_panel(const Plan& p, char* ws, int b, int l, bool bwd, bool fp32 = false) {
  const size_t o3 = (bwd ? p.o_pk_c2b3 : p.o_pk_c2f3)[b][l];
  if (o3 && !fp32) return {fptr(ws, o3), (unsigned)conv2_split_bytes(p)};
  return {fptr(ws, (bwd ? p.o_pk_c2b : p.o_pk_c2f)[b][l]), (unsigned)(sizeof(float) * conv2_elems(p))};
}
static void set_conv2_weights(FpropArgs& a, const Plan& p, char* ws, int b, int l, bool bwd) {
  const Panel w = conv2_panel(p, ws, b, l, bwd, true), w3 = conv2_panel(p, ws, b, l, bwd);
  a.w = w.p;
  if (w3.p != w.p) { a.w3 = w3.p; a.x3 = ws + p.o_x3; a.x3_bytes = p.x3_bytes; }
}
static void prefetch(FpropArgs& a, Panel w) { a.pf_ptr = w.p; a.pf_bytes = w.bytes; }

// developer aid: every convolution launch gets its own 64 x 16 slot of the phase-trace buffer (null when tracing is off or the slots ran out)
static unsigned long long* trace_slot(const Plan& p) {
  return (p.trace_base && p.trace_seq < p.trace_slots) ? p.trace_base + (size_t)(p.trace_seq++) * 64 * 16 : nullptr;
}

// Arguments of a convolution launch over dense block b's extent: zeroed, then the extent, the block's replica count, the K-split
// scratch (capacities travel with the arguments: no process-global state) and the launch's trace slot.
static FpropArgs block_args(const Plan& p, char* ws, int b) {
  FpropArgs a; memset(&a, 0, sizeof(a));
  a.N = p.N; a.D = p.Db[b]; a.H = p.Hb[b]; a.W = p.Wb[b]; a.nrep = p.nrep_b[b];
  a.kz_part = p.no_kz ? nullptr : fptr(ws, p.o_kz_part); a.kz_cnt = reinterpret_cast<unsigned*>(ws + p.o_kz_cnt);
  a.kz_part_bytes = KZ_PART_BYTES; a.kz_cnt_entries = KZ_CNT_ENTRIES;
  a.conv1_dgrad_resident = p.conv1_dgrad_resident;
  a.trace = trace_slot(p);
  return a;
}
static void wgrad_shape(WgradArgs& w, const Plan& p, int b) {   // zeroed in place: the tables that hold them are compared bytewise
  memset(&w, 0, sizeof(w));
  w.N = p.N; w.D = p.Db[b]; w.H = p.Hb[b]; w.W = p.Wb[b];
}

// (re)build the device job tables when the buffers they point into change
// returns true when the tables were (re)built and have to be uploaded
static bool build_tables(Plan& p, const float* params, float* run, char* ws) {
  if (p.tab_params == params && p.tab_run == run && p.tab_ws == ws) return false;
  char* hj = static_cast<char*>(p.host_jobs);
  RunStatJob* rj = reinterpret_cast<RunStatJob*>(hj);
  PackJob* pj = reinterpret_cast<PackJob*>(hj + (p.o_jobs_pack - p.o_jobs_run));
  GradJob* gj = reinterpret_cast<GradJob*>(hj + (p.o_jobs_grad - p.o_jobs_run));
  const NetCfg& c = p.cfg;
  const int nb = c.nblocks;
  int ir = 0, ip = 0, ig = 0;
  p.max_pack = 0; p.max_grad = 0;
  auto pack_job = [&](long src, size_t dst, int kind, int M, int C, long count) {
    PackJob& j = pj[ip++]; memset(&j, 0, sizeof(j));
    j.src = params + src; j.dst = fptr(ws, dst); j.kind = kind; j.M = M; j.C = C; j.count = count;
    p.max_pack = std::max(p.max_pack, count);
  };
  auto grad_job = [&](int kind, const void* src, long stride, int ns, int M, int C, long dst, long count) {
    GradJob& j = gj[ig++]; memset(&j, 0, sizeof(j));
    j.kind = kind; j.src = src; j.stride = stride; j.nsplit = ns; j.M = M; j.C = C; j.dst_off = dst; j.count = count;
    p.max_grad = std::max(p.max_grad, count);
  };
  auto grad_slab = [&](int kind, size_t o, int ns, int M, int C, long dst, long count) {   // partial slabs of `count` floats each (stem: padded)
    grad_job(kind, ws + o, kind == 2 ? (long)C * M * 352 : count, ns, M, C, dst, count);
  };
  auto site_jobs = [&](const NormSite& s) {   // running statistics of a site, and its dgamma / dbeta out of the pair block
    const StatPtr st = stats(ws, s), dg = dgsums(ws, s);
    RunStatJob& j = rj[ir++]; memset(&j, 0, sizeof(j));
    j.sum = st.sum; j.sq = st.sq; j.stride = s.stride; j.off = s.off; j.C = s.C;
    j.rmean = run ? run + s.rm : nullptr; j.rvar = run ? run + s.rv : nullptr; j.count = s.count;
    grad_job(3, dg.sq, s.C, 0, 0, s.C, s.w, s.C);
    grad_job(3, dg.sum, s.C, 0, 0, s.C, s.b, s.C);
  };
  pack_job(p.p_conv0, p.o_pk_conv0, (c.in_channels % 2 == 0) ? 3 : 4, c.init_features, c.in_channels, (long)7 * stem_krows(c.in_channels) * 64);
  grad_slab(2, p.o_sl_conv0, p.ns_conv0, c.init_features, c.in_channels, p.p_conv0, (long)c.init_features * c.in_channels * 343);
  site_jobs(norm0(p));
  for (int b = 0; b < nb; ++b) {
    p.gj_begin[b] = ig;
    const long max_before = p.max_grad;
    p.max_grad = 0;
    for (int l = 0; l < c.block_layers[b]; ++l) {
      const LayerOff& lo = p.layers[b][l];
      pack_job(lo.c1, p.o_pk_c1[b][l], 0, p.mid, lo.cin, conv1_elems(p, lo.cin));
      pack_job(lo.c2, p.o_pk_c2f[b][l], 1, c.growth, p.mid, conv2_elems(p));
      pack_job(lo.c2, p.o_pk_c2b[b][l], 2, c.growth, p.mid, conv2_elems(p));
      if (p.o_pk_c2f3[b][l]) pack_job(lo.c2, p.o_pk_c2f3[b][l], 5, c.growth, p.mid, (long)27 * (p.mid / 8) * c.growth);
      if (p.o_pk_c2b3[b][l]) pack_job(lo.c2, p.o_pk_c2b3[b][l], 6, c.growth, p.mid, (long)27 * (c.growth / 8) * p.mid);
      site_jobs(norm1(p, b, l));
      grad_slab(0, p.o_sl_c1[b][l], p.ns_c1[b][l], p.mid, lo.cin, lo.c1, conv1_elems(p, lo.cin));
      site_jobs(norm2(p, b, l));
      grad_slab(1, p.o_sl_c2[b][l], p.ns_c2[b][l], c.growth, p.mid, lo.c2, conv2_elems(p));
    }
    if (b != nb - 1) {
      const TransOff& t = p.trans[b];
      pack_job(t.cw, p.o_pk_tr[b], 0, t.cout, t.cin, trans_elems(t));
      site_jobs(transition(p, b));
      grad_slab(0, p.o_sl_tr[b], p.ns_tr[b], t.cout, t.cin, t.cw, trans_elems(t));
    } else {
      site_jobs(norm5(p));
    }
    p.gj_max[b] = p.max_grad;
    p.max_grad = std::max(p.max_grad, max_before);
  }
  p.gj_begin[nb] = ig;
  p.n_run_jobs = ir; p.n_pack_jobs = ip; p.n_grad_jobs = ig;
  p.tab_params = params; p.tab_run = run; p.tab_ws = ws;
  return true;
}

// ---- live kernel timing ---------------------------------------------------------------------------------------------
namespace {
struct ScopedTimer {   // records a start/stop event pair around one launch when the plan's timer selects it
  Plan& p; hipStream_t s; bool on;
  ScopedTimer(Plan& p_, int kind, int block, hipStream_t s_) : p(p_), s(s_), on(false) {
    if (!((p.timer_mask >> kind) & 1u) || (p.timer_block >= 0 && p.timer_block != block)) return;
    if (p.timer_used + 2 > p.timer_ev.size()) {
      if (p.timer_ev.size() >= 16384) return;   // read_timer() was not called for a long time: stop recording
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      p.timer_ev.push_back(a); p.timer_ev.push_back(b);
      p.timer_tag.push_back(0);
    }
    p.timer_tag[p.timer_used / 2] = kind * MAX_BLOCKS + (block >= 0 && block < MAX_BLOCKS ? block : 0);
    on = hipEventRecord(p.timer_ev[p.timer_used], s) == hipSuccess;
  }
  ~ScopedTimer() {
    if (!on) return;
    (void)hipEventRecord(p.timer_ev[p.timer_used + 1], s);
    p.timer_used += 2;
  }
};
}  // namespace

int plan_set_timer(Plan& p, int kind, int block) {
  MMNN_REQUIRE(kind >= -1 && kind < T_COUNT, "set_timer: unknown kernel class %d", kind);
  p.timer_mask = kind < 0 ? ~1u : (kind == T_NONE ? 0u : 1u << kind);   // -1: every class
  p.timer_block = block; p.timer_used = 0;
  for (int k = 0; k < T_COUNT * MAX_BLOCKS; ++k) { p.timer_ms[k] = 0.0; p.timer_count[k] = 0; }
  return 0;
}

int plan_read_timer(Plan& p, int kind, int block, double* total_ms, long* count) {
  MMNN_REQUIRE(kind >= T_NONE && kind < T_COUNT && block < MAX_BLOCKS, "read_timer: unknown kernel class %d / block %d", kind, block);
  for (size_t i = 0; i + 1 < p.timer_used; i += 2) {
    MMNN_HIP(hipEventSynchronize(p.timer_ev[i + 1]));
    float ms = 0.f;
    MMNN_HIP(hipEventElapsedTime(&ms, p.timer_ev[i], p.timer_ev[i + 1]));
    const int k = p.timer_tag[i / 2];
    p.timer_ms[k] += ms; p.timer_count[k] += 1;
  }
  p.timer_used = 0;
  double ms = 0.0; long n = 0;
  for (int k = 1; k < T_COUNT; ++k)         // class 0: all recorded classes together; block < 0: all blocks together
    for (int b = 0; b < MAX_BLOCKS; ++b)
      if ((kind == T_NONE || kind == k) && (block < 0 || block == b)) { ms += p.timer_ms[k * MAX_BLOCKS + b]; n += p.timer_count[k * MAX_BLOCKS + b]; }
  if (total_ms) *total_ms = ms;
  if (count) *count = n;
  return 0;
}

int plan_set_option(Plan& p, const char* name, long value) {
  const std::string s(name ? name : "");
  if (s == "single_stream") return 0;   // accepted, no effect: the backward always runs on the caller's stream
  if (s == "trace_buffer") { p.trace_base = reinterpret_cast<unsigned long long*>(value); p.trace_seq = 0; return 0; }   // device pointer, 0 = off
  if (s == "trace_slots") { p.trace_slots = (int)value; return 0; }
  if (s == "params_version") { p.params_version = value; return 0; }
  if (s == "no_kz") { p.no_kz = value != 0; return 0; }
  if (s == "conv1_dgrad_resident") {
    MMNN_REQUIRE(value >= 0 && value <= 2, "set_option: conv1_dgrad_resident is 0, 1 or 2");
    p.conv1_dgrad_resident = (int)value;
    return 0;
  }
  set_error("set_option: unknown option '%s'", s.c_str());
  return 1;
}
static DropCfg dropcfg(const Plan& p, uint64_t seed, int layer, int training) {
  DropCfg d; memset(&d, 0, sizeof(d));
  d.seed = seed; d.layer = layer; d.p = training ? p.cfg.dropout_p : 0.f;
  return d;
}

int plan_forward(Plan& p, const float* params, float* run, const float* x, char* ws, float* out, int training, uint64_t seed,
                 hipStream_t stream) {
  MMNN_REQUIRE(params && run && x && ws && out, "forward: null buffer");
  MMNN_REQUIRE(((uintptr_t)ws & 255) == 0 && ((uintptr_t)params & 15) == 0 && ((uintptr_t)x & 15) == 0, "forward: buffers must be 256/16-byte aligned");
  const NetCfg& c = p.cfg;
  const int nb = c.nblocks, N = p.N;
  if (!p.host_jobs) {   // pinned staging for the job tables: the only memory the plan owns
    MMNN_HIP(hipHostMalloc(&p.host_jobs, p.host_jobs_bytes, hipHostMallocDefault));
    memset(p.host_jobs, 0, p.host_jobs_bytes);
  }
  // The job tables hold pointers and counts only: they change when a buffer moves, in practice once.  Uploading them on every
  // forward cost 0.85 ms of HOST time per step (hipMemcpyAsync from the pinned staging buffer returns only when the copy has
  // been handed to the idle stream), which kept the enqueueing thread from ever running ahead of the GPU.
  if (p.tab_params != params || p.tab_run != run || p.tab_ws != ws) {
    if (p.tab_ws != nullptr) MMNN_HIP(hipStreamSynchronize(stream));   // an earlier upload from the same staging buffer may still be in flight
    build_tables(p, params, run, ws);
    MMNN_HIP(hipMemcpyAsync(ws + p.o_jobs_run, p.host_jobs, p.host_jobs_bytes, hipMemcpyHostToDevice, stream));
  }
  p.trace_seq = 0;
  if (training) MMNN_HIP(hipMemsetAsync(ws + p.o_fstat, 0, p.fstat_bytes, stream));
  MMNN_HIP(hipMemsetAsync(ws + p.o_kz_cnt, 0, KZ_CNT_ENTRIES * sizeof(unsigned), stream));
  // The [k][m] weight panels only change when the parameters do.  A caller that can vouch for a version number (option
  // "params_version", non-zero) gets the repack skipped while it stays the same -- 31 of 32 forwards under the reference's
  // accumulate-to-64 rule (main.py:403-407).  Version 0 (the default) repacks on every forward.
  int rc = 0;
  if (p.params_version == 0 || p.params_version != p.packed_version || p.packed_params != params || p.packed_ws != ws) {
    rc = launch_pack(reinterpret_cast<const PackJob*>(ws + p.o_jobs_pack), p.n_pack_jobs, p.max_pack, stream);
    if (rc) return rc;
    p.packed_version = p.params_version; p.packed_params = params; p.packed_ws = ws;
    ++p.pack_launches;
  }

  {  // stem
    const NormSite n0 = norm0(p);
    StemConvArgs a; memset(&a, 0, sizeof(a));
    a.N = N; a.Cin = c.in_channels; a.D = p.D; a.H = p.H; a.W = p.W; a.Do = p.D0; a.Ho = p.H0; a.Wo = p.W0; a.M = c.init_features;
    a.x = x; a.wp = fptr(ws, p.o_pk_conv0); a.out = fptr(ws, p.o_conv0);
    a.st_out = stats(ws, n0, 0, training);
    { ScopedTimer t(p, T_STEM_CONV, -1, stream); rc = launch_stem_conv(a, stream); }
    if (rc) return rc;
    const View X = concat(p, ws, 0);
    StemPoolArgs q; memset(&q, 0, sizeof(q));
    q.N = N; q.C = c.init_features; q.Di = p.D0; q.Hi = p.H0; q.Wi = p.W0; q.Do = p.Db[0]; q.Ho = p.Hb[0]; q.Wo = p.Wb[0];
    q.x = fptr(ws, p.o_conv0);
    q.bn = bnfwd(p, ws, params, run, n0, training);
    q.out = X.p; q.out_ns = X.ns;
    q.idx = reinterpret_cast<unsigned char*>(ws + p.o_idx);
    q.st_out = stats(ws, norm1(p, 0, 0), 0, training);
    if ((rc = launch_stem_pool(q, stream))) return rc;
  }
  int layer_id = 0;
  for (int b = 0; b < nb; ++b) {
    const View X = concat(p, ws, b);
    for (int l = 0; l < c.block_layers[b]; ++l, ++layer_id) {
      const NormSite n1 = norm1(p, b, l), n2 = norm2(p, b, l);
      // conv1: ReLU(BN(concat)) -> T1
      FpropArgs a = block_args(p, ws, b);
      a.Cin = n1.C; a.M = p.mid;
      set_in0(a, X);
      a.bn_in = bnfwd(p, ws, params, run, n1, training);
      a.w = conv1_panel(p, ws, b, l).p; a.w_ld = p.mid;
      set_out(a, t1(p, ws, b, l));
      a.st_out = stats(ws, n2, 0, training);
      prefetch(a, conv2_panel(p, ws, b, l, false));
      { ScopedTimer t(p, T_CONV1_FWD, b, stream); rc = launch_fprop(a, 1, PRO_BNRELU, EPI_STORE_STATS, stream); }
      if (rc) return rc;
      // conv2: ReLU(BN(T1)) -> growth new channels of the concat buffer (+ channel dropout)
      FpropArgs e = block_args(p, ws, b);
      e.Cin = p.mid; e.M = c.growth;
      set_in0(e, t1(p, ws, b, l));
      e.bn_in = bnfwd(p, ws, params, run, n2, training);
      set_conv2_weights(e, p, ws, b, l, false); e.w_ld = c.growth;
      set_out(e, concat(p, ws, b, n1.C));
      e.drop_out = dropcfg(p, seed, layer_id, training);
      e.st_out = stats(ws, n1, n1.C, training);
      if (l + 1 < c.block_layers[b]) prefetch(e, conv1_panel(p, ws, b, l + 1));
      else if (b != nb - 1) prefetch(e, trans_panel(p, ws, b));
      { ScopedTimer t(p, T_CONV2_FWD, b, stream); rc = launch_fprop(e, 27, PRO_BNRELU, EPI_STORE_STATS, stream); }
      if (rc) return rc;
    }
    if (b != nb - 1) {
      const NormSite tr = transition(p, b);
      PoolFwdArgs q; memset(&q, 0, sizeof(q));
      q.N = N; q.C = tr.C; q.D = p.Db[b]; q.H = p.Hb[b]; q.W = p.Wb[b];
      q.x = X.p; q.x_ns = X.ns;
      q.bn = bnfwd(p, ws, params, run, tr, training);
      q.out = pooled(p, ws, b).p;
      if ((rc = launch_bnrelu_avgpool(q, stream))) return rc;
      FpropArgs a = block_args(p, ws, b + 1);
      a.Cin = p.trans[b].cin; a.M = p.trans[b].cout;
      set_in0(a, pooled(p, ws, b));
      a.w = trans_panel(p, ws, b).p; a.w_ld = a.M;
      set_out(a, concat(p, ws, b + 1));
      a.st_out = stats(ws, norm1(p, b + 1, 0), 0, training);
      prefetch(a, conv1_panel(p, ws, b + 1, 0));
      if ((rc = launch_fprop(a, 1, PRO_NONE, EPI_STORE_STATS, stream))) return rc;
    } else {
      const NormSite n5 = norm5(p);
      BnApplyArgs q; memset(&q, 0, sizeof(q));
      q.N = N; q.C = n5.C; q.V = p.Vb[b];
      q.x = X.p; q.x_ns = X.ns;
      q.bn = bnfwd(p, ws, params, run, n5, training);
      q.out = out;
      if ((rc = launch_bn_apply(q, stream))) return rc;
    }
  }
  if (training) {
    if ((rc = launch_running_stats(reinterpret_cast<const RunStatJob*>(ws + p.o_jobs_run), p.n_run_jobs, c.momentum,
                                   p.nbt_count == p.n_run_jobs ? p.nbt : nullptr, stream))) return rc;
  }
  return 0;
}

static LayerBind layer_bind(const Plan& p, const float* params, float* run, char* ws, int b, int l) {
  const NormSite n1 = norm1(p, b, l), n2 = norm2(p, b, l);
  LayerBind L; memset(&L, 0, sizeof(L));
  L.bn1 = bnfwd(p, ws, params, run, n1, 1); L.bn2 = bnfwd(p, ws, params, run, n2, 1);
  L.gr_new = bnbwd(p, ws, params, n1, n1.C); L.gr_t1 = bnbwd(p, ws, params, n2);
  L.dg1 = dgsums(ws, n1); L.dg2 = dgsums(ws, n2); L.s_x = sums(ws, n1);
  L.x = concat(p, ws, b); L.g = concat_grad(p, ws, b);
  L.x_new = concat(p, ws, b, n1.C); L.g_new = concat_grad(p, ws, b, n1.C);
  L.t1 = t1(p, ws, b, l); L.dz2 = dz2(p, ws, b, l);
  return L;
}

// Arguments of the two weight-gradient launches of dense layer (b, l): conv2 (3x3x3, `w2`) and conv1 (1x1x1, `w1`).  The dropout
// seed is left 0: the batched kernels take the step's as an argument.
static void layer_wgrad_args(const Plan& p, const LayerBind& L, char* ws, int b, int l, int layer_id, WgradArgs& w2, WgradArgs& w1) {
  const int cin = p.layers[b][l].cin;
  wgrad_shape(w2, p, b);
  w2.M = p.cfg.growth; w2.Cin = p.mid;
  set_g0(w2, L.g_new); set_g1(w2, L.x_new); w2.gr = L.gr_new;
  w2.drop.layer = layer_id; w2.drop.p = p.cfg.dropout_p;
  set_x(w2, L.t1); w2.bn = L.bn2;
  w2.slab = fptr(ws, p.o_sl_c2[b][l]); w2.slab_stride = conv2_elems(p); w2.nsplit = p.ns_c2[b][l];
  wgrad_shape(w1, p, b);
  w1.M = p.mid; w1.Cin = cin;
  set_g0(w1, L.dz2); set_g1(w1, L.t1); w1.gr = L.gr_t1;
  set_x(w1, L.x); w1.bn = L.bn1;
  w1.slab = fptr(ws, p.o_sl_c1[b][l]); w1.slab_stride = conv1_elems(p, cin); w1.nsplit = p.ns_c1[b][l];
}

// first contribution to block b's G from the consumer at the end of the block: norm5 (mode 0) or the transition (mode 1, un-pool + ReLU)
static ConsumerBwdArgs consumer_bwd_args(const Plan& p, const float* params, float* run, char* ws, const NormSite& s, int b, int mode, const float* dy) {
  const View X = concat(p, ws, b), G = concat_grad(p, ws, b);
  const StatPtr dg = dgsums(ws, s);
  ConsumerBwdArgs a; memset(&a, 0, sizeof(a));
  a.N = p.N; a.C = s.C; a.D = p.Db[b]; a.H = p.Hb[b]; a.W = p.Wb[b]; a.mode = mode; a.nrep = s.nrep;
  a.dy = dy; a.x = X.p; a.x_ns = X.ns;
  a.bn = bnfwd(p, ws, params, run, s, 1);
  a.g = G.p; a.g_ns = G.ns; a.dbeta = dg.sum; a.dgamma = dg.sq;
  a.s_acc = sums(ws, s);
  return a;
}

int plan_backward(Plan& p, const float* params, const float* x, char* ws, const float* grad_out, float* grad_params, int accumulate,
                  uint64_t seed, hipStream_t stream) {
  return plan_backward_range(p, params, x, ws, grad_out, grad_params, accumulate, seed, p.cfg.nblocks - 1, 0, stream);
}

int plan_block_param_range(const Plan& p, int block, long* begin, long* end) {
  const int nb = p.cfg.nblocks;
  MMNN_REQUIRE(block >= -1 && block < nb && begin && end, "block_param_range: block %d out of range [-1, %d)", block, nb);
  if (block < 0) { *begin = 0; *end = norm1(p, 0, 0).w; return 0; }             // stem: conv0, norm0
  *begin = norm1(p, block, 0).w;                                                // the block's layers, then its transition / norm5
  *end = (block + 1 < nb) ? norm1(p, block + 1, 0).w : p.n_params;
  return 0;
}

// Backward of dense blocks hi, hi-1, ..., lo (0-based; the whole backward = one call with hi = nblocks-1, lo = 0).  A caller that
// splits it must walk the blocks downwards without gaps, starting at the last block; the call for `lo == 0` also runs the stem.  When
// a call returns (in stream order) the gradients of every parameter of blocks [lo, hi] -- plus the stem's when lo == 0 -- are FINAL in
// grad_params: a data-parallel caller can start reducing that range while the next call's kernels run.
int plan_backward_range(Plan& p, const float* params, const float* x, char* ws, const float* grad_out, float* grad_params, int accumulate,
                        uint64_t seed, int hi, int lo, hipStream_t stream) {
  MMNN_REQUIRE(params && x && ws && grad_out && grad_params, "backward: null buffer");
  MMNN_REQUIRE(p.tab_ws == ws && p.tab_params == params, "backward: must follow a training forward on the same buffers");
  const NetCfg& c = p.cfg;
  const int nb = c.nblocks, N = p.N;
  MMNN_REQUIRE(hi >= lo && lo >= 0 && hi < nb, "backward: bad block range [%d, %d] of %d blocks", lo, hi, nb);
  MMNN_REQUIRE(hi == nb - 1 || p.bwd_next == hi, "backward: block range [%d, %d] out of order (expected to continue at block %d)", lo, hi, p.bwd_next);
  float* run = p.tab_run;
  int rc;
  const bool first_call = hi == nb - 1;
  if (first_call) {
    MMNN_HIP(hipMemsetAsync(ws + p.o_bstat, 0, p.bstat_bytes, stream));
    MMNN_HIP(hipMemsetAsync(ws + p.o_kz_cnt, 0, KZ_CNT_ENTRIES * sizeof(unsigned), stream));
  }
  p.bwd_next = lo - 1;
  // Device-resident argument tables of every layer's two weight-gradient launches; the pinned staging buffer is their host copy.
  // Their content does not depend on the step (the dropout seed travels as a kernel argument), so they are uploaded only when a
  // buffer moved or tracing was switched on or off -- in practice once.
  if (first_call || !p.wg_uploaded) {
    const size_t bytes = sizeof(WgradArgs) * 2 * p.n_layers;
    if (!p.wg_pinned) {
      MMNN_HIP(hipHostMalloc(&p.wg_pinned, bytes, hipHostMallocDefault));
      p.wg_shadow.assign(bytes, 0);
      p.wg_uploaded = false;
    }
    std::vector<WgradArgs> tab(2 * p.n_layers);
    int id = 0;
    for (int b = 0; b < nb; ++b)
      for (int l = 0; l < c.block_layers[b]; ++l, ++id) {
        layer_wgrad_args(p, layer_bind(p, params, run, ws, b, l), ws, b, l, id, tab[id], tab[p.n_layers + id]);
        tab[id].trace = trace_slot(p);
        tab[p.n_layers + id].trace = trace_slot(p);
      }
    if (!p.wg_uploaded || memcmp(tab.data(), p.wg_shadow.data(), bytes) != 0) {
      if (p.wg_uploaded) MMNN_HIP(hipStreamSynchronize(stream));   // an earlier upload from the pinned buffer may still be in flight
      memcpy(p.wg_pinned, tab.data(), bytes);
      memcpy(p.wg_shadow.data(), tab.data(), bytes);
      MMNN_HIP(hipMemcpyAsync(ws + p.o_wg_table, p.wg_pinned, bytes, hipMemcpyHostToDevice, stream));
      p.wg_uploaded = true;
    }
  }
  const WgradArgs* dev_w2 = reinterpret_cast<const WgradArgs*>(ws + p.o_wg_table);
  const WgradArgs* dev_w1 = dev_w2 + p.n_layers;
  const WgradArgs* host_w2 = static_cast<const WgradArgs*>(p.wg_pinned);
  const WgradArgs* host_w1 = host_w2 + p.n_layers;
  // The weight gradients of dense block b (layer ids [id0, id0 + its layer count)) go out once the data-gradient chain has passed all
  // of its layers.  The layers are independent: ONE launch per kernel variant covers them all (blockIdx.z = layer).
  auto block_wgrads = [&](int b, int id0) -> int {
    const int np = c.block_layers[b];
    int rc2;
    { ScopedTimer t(p, T_CONV2_WGRAD, b, stream); rc2 = launch_wgrad_batched(host_w2 + id0, dev_w2 + id0, np, seed, 27, PRO_BNRELU, stream); }
    if (rc2) return rc2;
    // conv1: runs [i, j) of equal channel-group width (monotonic in the layer index), last layers first; a run of one layer takes
    // the unbatched kernel
    for (int j = id0 + np; j > id0;) {
      int i = j - 1;
      while (i > id0 && wgrad1_channel_width(host_w1[i - 1].Cin, p.Vb[b]) == wgrad1_channel_width(host_w1[j - 1].Cin, p.Vb[b])) --i;
      {
        ScopedTimer t(p, T_CONV1_WGRAD, b, stream);
        rc2 = j - i > 1 ? launch_wgrad_batched(host_w1 + i, dev_w1 + i, j - i, seed, 1, PRO_BNRELU, stream)
                        : launch_wgrad1(host_w1[i], PRO_BNRELU, stream);
      }
      if (rc2) return rc2;
      j = i;
    }
    return 0;
  };
  // norm5: first contribution to the last block's G
  if (first_call && (rc = launch_consumer_bwd(consumer_bwd_args(p, params, run, ws, norm5(p), nb - 1, 0, grad_out), stream))) return rc;
  int layer_id = 0;
  for (int b = 0; b <= hi; ++b) layer_id += c.block_layers[b];
  for (int b = hi; b >= lo; --b) {
    for (int l = c.block_layers[b] - 1; l >= 0; --l) {
      --layer_id;
      const LayerBind L = layer_bind(p, params, run, ws, b, l);
      const int cin = p.layers[b][l].cin;
      // conv2 data gradient -> dZ2 (ReLU mask of norm2 applied) + dgamma2/dbeta2
      FpropArgs a = block_args(p, ws, b);
      a.Cin = c.growth; a.M = p.mid;
      set_in0(a, L.g_new); set_in1(a, L.x_new); a.gr_in = L.gr_new;
      a.drop_in = dropcfg(p, seed, layer_id, 1);
      set_conv2_weights(a, p, ws, b, l, true); a.w_ld = p.mid;
      set_out(a, L.dz2); set_ex(a, L.t1); a.ebn = L.bn2;
      a.dbeta = L.dg2.sum; a.dgamma = L.dg2.sq;
      prefetch(a, conv1_weights(p, params, b, l));
      { ScopedTimer t(p, T_CONV2_DGRAD, b, stream); rc = launch_fprop(a, 27, PRO_GRAD, EPI_MASK_STORE, stream); }
      if (rc) return rc;
      // conv1 data gradient -> G[0:cin) += gamma1 * mask * (...), dgamma1/dbeta1, S1/S2
      FpropArgs d = block_args(p, ws, b);
      d.Cin = p.mid; d.M = cin;
      set_in0(d, L.dz2); set_in1(d, L.t1); d.gr_in = L.gr_t1;
      d.w = conv1_weights(p, params, b, l).p; d.w_ld = cin;
      set_out(d, L.g); set_ex(d, L.x); d.ebn = L.bn1;
      d.dbeta = L.dg1.sum; d.dgamma = L.dg1.sq;
      d.s_acc = L.s_x;
      if (l > 0) prefetch(d, conv2_panel(p, ws, b, l - 1, true));
      { ScopedTimer t(p, T_CONV1_DGRAD, b, stream); rc = launch_fprop(d, 1, PRO_GRAD, EPI_MASK_ACCUM, stream); }
      if (rc) return rc;
    }
    if ((rc = block_wgrads(b, layer_id))) return rc;     // layer_id: the block's first layer
    const View X = concat(p, ws, b), G = concat_grad(p, ws, b);
    const BnBwd gr = bnbwd(p, ws, params, norm1(p, b, 0));   // BN-backward of the whole concat buffer (gammas folded into G)
    if (b > 0) {
      const int pb = b - 1;
      const TransOff& t = p.trans[pb];
      // transition conv weight gradient (input = pooled activations)
      WgradArgs w;
      wgrad_shape(w, p, b);
      w.M = t.cout; w.Cin = t.cin;
      set_g0(w, G); set_g1(w, X); w.gr = gr;
      set_x(w, pooled(p, ws, pb));
      w.slab = fptr(ws, p.o_sl_tr[pb]); w.slab_stride = trans_elems(t); w.nsplit = p.ns_tr[pb];
      if ((rc = launch_wgrad1(w, PRO_NONE, stream))) return rc;
      // transition conv data gradient -> gradient wrt the pooled activations
      FpropArgs d = block_args(p, ws, b);
      d.nrep = 0;   // (as it always was: the plain store epilogue accumulates no statistics)
      d.Cin = t.cout; d.M = t.cin;
      set_in0(d, G); set_in1(d, X); d.gr_in = gr;
      d.w = params + t.cw; d.w_ld = t.cin;
      set_out(d, pooled_grad(p, ws, pb));
      if ((rc = launch_fprop(d, 1, PRO_GRAD, EPI_STORE, stream))) return rc;
      // un-pool + ReLU + BN of the transition: first contribution to the previous block's G
      if ((rc = launch_consumer_bwd(consumer_bwd_args(p, params, run, ws, transition(p, pb), pb, 1, pooled_grad(p, ws, pb).p), stream))) return rc;
    } else {
      const NormSite n0 = norm0(p);
      const StatPtr dg = dgsums(ws, n0);
      StemPoolBwdArgs q; memset(&q, 0, sizeof(q));
      q.N = N; q.C = c.init_features; q.Di = p.D0; q.Hi = p.H0; q.Wi = p.W0; q.Do = p.Db[0]; q.Ho = p.Hb[0]; q.Wo = p.Wb[0];
      q.x = fptr(ws, p.o_conv0);
      q.bn = bnfwd(p, ws, params, run, n0, 1);
      q.g = G.p; q.g_ns = G.ns; q.xp = X.p; q.xp_ns = X.ns;
      q.gr = gr;
      q.idx = reinterpret_cast<const unsigned char*>(ws + p.o_idx);
      q.dz = fptr(ws, p.o_dz0);
      q.dbeta = dg.sum; q.dgamma = dg.sq;
      if ((rc = launch_stem_pool_bwd(q, stream))) return rc;
      StemWgradArgs w; memset(&w, 0, sizeof(w));
      w.N = N; w.Cin = c.in_channels; w.D = p.D; w.H = p.H; w.W = p.W; w.Do = p.D0; w.Ho = p.H0; w.Wo = p.W0; w.M = c.init_features;
      w.x = x; w.dz = fptr(ws, p.o_dz0); w.y = fptr(ws, p.o_conv0);
      w.gr = bnbwd(p, ws, params, n0);   // BN-backward of the conv output (single consumer norm0)
      w.slab = fptr(ws, p.o_sl_conv0); w.slab_stride = (long)c.in_channels * c.init_features * 352; w.nsplit = p.ns_conv0;
      { ScopedTimer t(p, T_STEM_WGRAD, -1, stream); rc = launch_stem_wgrad(w, stream); }
      if (rc) return rc;
    }
  }
  const long stem_count = (long)c.init_features * c.in_channels * 343;
  const GradJob* jobs = reinterpret_cast<const GradJob*>(ws + p.o_jobs_grad);
  // one launch for every job of this call: blocks [lo, hi] (their layers + the transition / norm5 behind them), + the stem when lo == 0
  const int j0 = lo == 0 ? 0 : p.gj_begin[lo], j1 = p.gj_begin[hi + 1];
  long jmax = lo == 0 ? stem_count : 0;
  for (int b = lo; b <= hi; ++b) jmax = std::max(jmax, p.gj_max[b]);
  return launch_finalize(jobs + j0, j1 - j0, jmax, grad_params, accumulate, stream);
}

int plan_relu_mask(Plan& p, const float* params, char* ws, int kind, int b, int l, unsigned char* out, hipStream_t stream) {
  MMNN_REQUIRE(p.tab_ws == ws && p.tab_params == params, "relu_mask: must follow a training forward on the same buffers");
  const NetCfg& c = p.cfg;
  MMNN_REQUIRE(kind == 0 || (b >= 0 && b < c.nblocks), "relu_mask: bad block %d", b);
  MMNN_REQUIRE(kind != 3 || b < c.nblocks - 1, "relu_mask: block %d has no transition", b);
  MMNN_REQUIRE(kind == 0 || kind == 3 || (l >= 0 && l < c.block_layers[b] && (kind == 1 || kind == 2)), "relu_mask: bad site (%d,%d,%d)", kind, b, l);
  const NormSite s = kind == 0 ? norm0(p) : kind == 1 ? norm1(p, b, l) : kind == 2 ? norm2(p, b, l) : transition(p, b);
  const int V = kind == 0 ? p.D0 * p.H0 * p.W0 : p.Vb[b];
  const View X = kind == 0 ? View{fptr(ws, p.o_conv0), (long)s.C * V, 0} : kind == 2 ? t1(p, ws, b, l) : concat(p, ws, b);
  MaskArgs a; memset(&a, 0, sizeof(a));
  a.out = out; a.N = p.N; a.C = s.C; a.V = V; a.x = X.p; a.x_ns = X.ns;
  a.bn = bnfwd(p, ws, params, p.tab_run, s, 1);
  return launch_relu_mask(a, stream);
}

long plan_ws_offset(const Plan& p, const char* name, int i, int j) {
  const std::string s(name);
  const int nb = p.cfg.nblocks;
  auto okb = [&](int b) { return b >= 0 && b < nb; };
  auto okl = [&](int b, int l) { return okb(b) && l >= 0 && l < p.cfg.block_layers[b]; };
  if (s == "conv0") return (long)p.o_conv0;
  if (s == "idx") return (long)p.o_idx;
  if (s == "dz0") return (long)p.o_dz0;
  if (s == "dz2" && okl(i, j)) return (long)(p.o_dz2[i] + (size_t)j * p.N * p.mid * p.Vb[i] * sizeof(float));
  if (s == "dap") return (long)p.o_dap;
  if (s == "x" && okb(i)) return (long)p.o_x[i];
  if (s == "g" && okb(i)) return (long)p.o_g[i];
  if (s == "ap" && okb(i) && i < nb - 1) return (long)p.o_ap[i];
  if (s == "t1" && okl(i, j)) return (long)p.o_t1[i][j];
  if (s == "st_conv0") return (long)p.o_st_conv0;
  if (s == "st_x" && okb(i)) return (long)p.o_st_x[i];
  if (s == "st_t1" && okl(i, j)) return (long)p.o_st_t1[i][j];
  if (s == "s_x" && okb(i)) return (long)p.o_s_x[i];
  if (s == "pk_c1" && okl(i, j)) return (long)p.o_pk_c1[i][j];
  if (s == "pk_c2f" && okl(i, j)) return (long)p.o_pk_c2f[i][j];
  if (s == "pk_c2b" && okl(i, j)) return (long)p.o_pk_c2b[i][j];
  if (s == "pk_c2f3" && okl(i, j)) return p.o_pk_c2f3[i][j] ? (long)p.o_pk_c2f3[i][j] : -1;
  if (s == "pk_c2b3" && okl(i, j)) return p.o_pk_c2b3[i][j] ? (long)p.o_pk_c2b3[i][j] : -1;
  if (s == "x3") return p.x3_bytes ? (long)p.o_x3 : -1;        // planes of the latest bf16x3 conv2 launch
  if (s == "#x3_bytes") return (long)p.x3_bytes;
  if (s == "pk_conv0") return (long)p.o_pk_conv0;
  if (s == "#pack_launches") return p.pack_launches;      // counter, not an offset (tests)
  if (s == "#ns_c2" && okl(i, j)) return p.ns_c2[i][j];   // voxel splits of the layer's weight-gradient launches (tests)
  if (s == "#ns_c1" && okl(i, j)) return p.ns_c1[i][j];
  if (s == "#conv1_dgrad_resident" && okb(i)) {   // layers of block i whose conv1 data gradient takes the resident-operand kernel (tests)
    long cnt = 0;
    for (int l = 0; l < p.cfg.block_layers[i]; ++l)
      cnt += conv1_dgrad_resident_shape_ok(p.conv1_dgrad_resident, p.N, p.Vb[i], p.mid, p.layers[i][l].cin, p.layers[i][l].cin) ? 1 : 0;
    return cnt;
  }
  return -1;
}

}  // namespace mmnn
