// pBSRNN launch plan of the native runtime (arch 0; wesep/models/bsrnn.py:300-394): band tables, ResRNN packs,
// grouped-GEMM descriptors, the separator with its speaker fusion layers, mask MLP and iSTFT.
#include "engine_internal.h"

namespace wsrt {

// ---- load-time preparation -----------------------------------------------------------------------------------
void band_table(ws_engine* e) {         // bsrnn.py:190-209
  const double nyq = e->sr / 2.0;
  auto bwid = [&](double hz) { return static_cast<int>(floor(hz / nyq * kNBin)); };
  e->bs.bw.clear();
  for (int i = 0; i < 15; ++i) e->bs.bw.push_back(bwid(100));
  for (int i = 0; i < 10; ++i) e->bs.bw.push_back(bwid(200));
  for (int i = 0; i < 5; ++i) e->bs.bw.push_back(bwid(500));
  e->bs.bw.push_back(bwid(2000));
  int sum = 0;
  for (int b : e->bs.bw) sum += b;
  e->bs.bw.push_back(kNBin - sum);
  e->bs.K = static_cast<int>(e->bs.bw.size());
  e->bs.f0.assign(e->bs.K, 0);
  for (int g = 1; g < e->bs.K; ++g) e->bs.f0[g] = e->bs.f0[g - 1] + e->bs.bw[g - 1];
}

int prep_rnn(ws_engine* e, const std::string& pre, RnnPrep* r) {
  static const char* names[] = {"rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0",
                                "rnn.weight_ih_l0_reverse", "rnn.weight_hh_l0_reverse", "rnn.bias_ih_l0_reverse",
                                "rnn.bias_hh_l0_reverse"};
  const int64_t shapes[][2] = {{kG4, kN}, {kG4, kH}, {kG4, 1}, {kG4, 1}, {kG4, kN}, {kG4, kH}, {kG4, 1}, {kG4, 1}};
  for (int i = 0; i < 8; ++i)
    if (!require(e, pre + names[i], {shapes[i][0], shapes[i][1]})) return WS_ERR_INVALID;
  if (!require(e, pre + "norm.weight", {kN}) || !require(e, pre + "norm.bias", {kN}) ||
      !require(e, pre + "proj.weight", {kN, 2 * kH}) || !require(e, pre + "proj.bias", {kN}))
    return WS_ERR_INVALID;
  const float* wih_f = e->dev(pre + names[0]);
  const float* wih_r = e->dev(pre + names[4]);
  r->whf = e->dev(pre + names[1]);
  r->whr = e->dev(pre + names[5]);
  r->norm_w = e->dev(pre + "norm.weight");
  r->norm_b = e->dev(pre + "norm.bias");
  r->proj_b = e->dev(pre + "proj.bias");
  const float* bias[4] = {e->dev(pre + names[2]), e->dev(pre + names[3]), e->dev(pre + names[6]), e->dev(pre + names[7])};
  return pack_rnn(e, kN, wih_f, wih_r, bias, e->dev(pre + "proj.weight"), r);
}

// the packs of one BLSTM + projection over C input features (r->whf / r->whr set): [W_ih_f | W_ih_r] and its biases
// (ws_lstm_cat_ih order), MFMA-fragment packs of W_ih and proj [C][2 * 256], the fused stream and both W_hh layouts
int pack_rnn(ws_engine* e, int C, const float* wih_f, const float* wih_r, const float* const bias[4], const float* proj_w,
             RnnPrep* r) {
  Arena& a = e->persist;
  float* wcat = a.alloc(size_t(2) * kG4 * C);
  r->bcat = a.alloc(2 * kG4);
  r->wih_pack = a.alloc(size_t(2) * kG4 * C);
  r->proj_pack = a.alloc(size_t(C) * 2 * kH);
  r->fpack = a.alloc(WS_LSTM_FUSED_PACK_FLOATS);
  r->pack16 = a.alloc(WS_LSTM_PACK_FLOATS);
  r->pack32 = a.alloc(WS_LSTM_PACK_FLOATS);
  float* bwd_scratch = a.alloc(WS_LSTM_PACK_FLOATS);   // the backward-pass pack is produced too; unused here
  WS_PTR(wcat && r->bcat && r->wih_pack && r->proj_pack && r->fpack && r->pack16 && r->pack32 && bwd_scratch);
  void* s = e->stream;
  WS_RUN(e, ws_lstm_cat_ih(wih_f, wih_r, bias[0], bias[1], bias[2], bias[3], C, wcat, r->bcat, s));
  WS_RUN(e, ws_pack_w(wcat, 2 * kG4, C, C, 0, 0, r->wih_pack, s));
  WS_RUN(e, ws_pack_w(proj_w, C, 2 * kH, 2 * kH, 0, 1, r->proj_pack, s));
  WS_RUN(e, ws_lstm_pack_fused(wih_f, wih_r, r->whf, r->whr, r->fpack, s));
  WS_RUN(e, ws_lstm_pack(r->whf, r->whr, r->pack16, bwd_scratch, WS_LSTM_BF16X3_BLK16, s));
  WS_RUN(e, ws_lstm_pack(r->whf, r->whr, r->pack32, bwd_scratch, WS_LSTM_BF16X3_BLK, s));
  return WS_OK;
}

// meta checks, band tables, per-band BN / mask operands, ResRNN packs, fusion layers, then the speaker stage
int prepare_bsrnn(ws_engine* e) {
  int rc = read_speaker_meta(e);
  if (rc != WS_OK) return rc;
  e->bs.num_repeat = static_cast<int>(meta_or(e, "num_repeat", 6));
  e->bs.fuse = static_cast<int>(meta_or(e, "spk_fuse_type", 2));
  e->bs.multi_fuse = static_cast<int>(meta_or(e, "multi_fuse", 0));
  if (meta_or(e, "win", 512) != 512 || meta_or(e, "stride", 128) != kHop || meta_or(e, "feature_dim", kN) != kN) {
    set_err("engine: built for win 512, stride 128, feature_dim 128");
    return WS_ERR_INVALID;
  }
  if (e->bs.fuse < 0 || e->bs.fuse > 3 || e->bs.num_repeat < 1 || e->E % 4 || e->spk.feat_dim % 8) {
    set_err("engine: unsupported configuration (fuse %d, num_repeat %d, spk_emb_dim %d, feat_dim %d)", e->bs.fuse,
            e->bs.num_repeat, e->E, e->spk.feat_dim);
    return WS_ERR_INVALID;
  }
  band_table(e);
  // weights to the device, once
  e->dw = upload(e, e->persist, e->hw.data(), e->hw.size());
  WS_PTR(e->dw);
  std::vector<int> bob, bw2, off2;
  for (int g = 0; g < e->bs.K; ++g) {
    for (int i = 0; i < e->bs.bw[g]; ++i) bob.push_back(g);
    bw2.push_back(2 * e->bs.bw[g]);
    off2.push_back(2 * e->bs.f0[g]);
  }
  e->bs.d_band_of_bin = upload_ints(e, e->persist, bob);
  e->bs.d_f0 = upload_ints(e, e->persist, e->bs.f0);
  e->bs.d_bw = upload_ints(e, e->persist, e->bs.bw);
  e->bs.d_bw2 = upload_ints(e, e->persist, bw2);
  e->bs.d_off2 = upload_ints(e, e->persist, off2);
  WS_PTR(e->bs.d_band_of_bin && e->bs.d_f0 && e->bs.d_bw && e->bs.d_bw2 && e->bs.d_off2);
  // per-band BN / mask parameters
  for (int g = 0; g < e->bs.K; ++g) {
    const std::string b = "BN." + std::to_string(g) + ".", m = "mask." + std::to_string(g) + ".";
    const int bw = e->bs.bw[g];
    if (!require(e, b + "0.weight", {2 * bw}) || !require(e, b + "0.bias", {2 * bw}) ||
        !require(e, b + "1.weight", {kN, 2 * bw}) || !require(e, b + "1.bias", {kN}) ||
        !require(e, m + "0.weight", {kN}) || !require(e, m + "0.bias", {kN}) ||
        !require(e, m + "1.weight", {4 * kN, kN}) || !require(e, m + "1.bias", {4 * kN}) ||
        !require(e, m + "3.weight", {4 * kN, 4 * kN}) || !require(e, m + "3.bias", {4 * kN}) ||
        !require(e, m + "5.weight", {4 * bw, 4 * kN}) || !require(e, m + "5.bias", {4 * bw}))
      return WS_ERR_INVALID;
  }
  // separator.separation layout (bsrnn.py:106-125)
  e->bs.sep_kind.clear();
  if (e->bs.multi_fuse) {
    for (int r = 0; r < e->bs.num_repeat; ++r) {
      e->bs.sep_kind.push_back(0);
      e->bs.sep_kind.push_back(1);
    }
  } else {
    e->bs.sep_kind.push_back(0);
    for (int r = 0; r < e->bs.num_repeat; ++r) e->bs.sep_kind.push_back(1);
  }
  for (size_t i = 0; i < e->bs.sep_kind.size(); ++i) {
    const std::string pre = "separator.separation." + std::to_string(i) + ".";
    if (e->bs.sep_kind[i] == 1) {
      RnnPrep t, b;
      if ((rc = prep_rnn(e, pre + "band_rnn.", &t)) != WS_OK) return rc;
      if ((rc = prep_rnn(e, pre + "band_comm.", &b)) != WS_OK) return rc;
      e->bs.rnn.push_back(t);
      e->bs.rnn.push_back(b);
    } else if (e->bs.fuse == 3) {
      if (!require(e, pre + "fc.gamma_fcs.0.weight", {kN, e->E}) || !require(e, pre + "fc.gamma_fcs.0.bias", {kN}) ||
          !require(e, pre + "fc.beta_fcs.0.weight", {kN, e->E}) || !require(e, pre + "fc.beta_fcs.0.bias", {kN}))
        return WS_ERR_INVALID;
    } else {
      const int in = e->bs.fuse == 0 ? kN + e->E : e->E;
      if (!require(e, pre + "fc.linear.weight", {kN, in}) || !require(e, pre + "fc.linear.bias", {kN})) return WS_ERR_INVALID;
    }
  }
  return prep_speaker(e);
}

int build_descriptors(ws_engine* e, int R, int Tf) {
  if (e->bs.desc_R == R && e->bs.desc_Tf == Tf && e->bs.d_bn) return WS_OK;
  const int K = e->bs.K, H1 = 4 * kN;
  const long long M = (long long)R * Tf;
  std::vector<ws_group_nt> bn(K), l1(K), l2(K), l3(K);
  for (int g = 0; g < K; ++g) {
    const std::string b = "BN." + std::to_string(g) + ".", m = "mask." + std::to_string(g) + ".";
    const int bw = e->bs.bw[g];
    const long long zoff = (long long)g * Tf * kN, hoff = (long long)g * M * H1;
    bn[g] = ws_group_nt{e->dev(b + "1.weight"), e->dev(b + "1.bias"), e->dev(b + "0.weight"), e->dev(b + "0.bias"),
                        2LL * e->bs.f0[g], zoff, g, 2 * bw, kN, 2 * bw, 0};
    l1[g] = ws_group_nt{e->dev(m + "1.weight"), e->dev(m + "1.bias"), e->dev(m + "0.weight"), e->dev(m + "0.bias"),
                        zoff, hoff, g, kN, H1, kN, 0};
    l2[g] = ws_group_nt{e->dev(m + "3.weight"), e->dev(m + "3.bias"), nullptr, nullptr, hoff, hoff, 0, H1, H1, H1, 0};
    l3[g] = ws_group_nt{e->dev(m + "5.weight"), e->dev(m + "5.bias"), nullptr, nullptr, hoff, 4LL * e->bs.f0[g], 0, H1,
                        4 * bw, H1, 0};
  }
  if (!e->bs.d_bn) {
    const size_t nf = (sizeof(ws_group_nt) * K + 3) / 4;
    e->bs.d_bn = reinterpret_cast<ws_group_nt*>(e->persist.alloc(nf));
    e->bs.d_l1 = reinterpret_cast<ws_group_nt*>(e->persist.alloc(nf));
    e->bs.d_l2 = reinterpret_cast<ws_group_nt*>(e->persist.alloc(nf));
    e->bs.d_l3 = reinterpret_cast<ws_group_nt*>(e->persist.alloc(nf));
    WS_PTR(e->bs.d_bn && e->bs.d_l1 && e->bs.d_l2 && e->bs.d_l3);
  }
  const size_t bytes = sizeof(ws_group_nt) * K;
  int rc;
  if ((rc = to_device(e, e->bs.d_bn, bn.data(), bytes)) != WS_OK || (rc = to_device(e, e->bs.d_l1, l1.data(), bytes)) != WS_OK ||
      (rc = to_device(e, e->bs.d_l2, l2.data(), bytes)) != WS_OK || (rc = to_device(e, e->bs.d_l3, l3.data(), bytes)) != WS_OK)
    return rc;
  e->bs.desc_R = R;
  e->bs.desc_Tf = Tf;
  return WS_OK;
}

// ResRNN (bsrnn.py:38-46) on the blocked layout; mirrors functional.ResRNNBlkFn.forward with the packs precomputed.
// d_tf (ragged batches, or nullptr): device table of the rows' valid frame counts.  Only the time view reads it: its
// GroupNorm statistics cover a row's valid frames, and the pre-activations of the frames behind them are exact zeros, so
// the reverse direction arrives at the row's last valid frame with zero state.  That needs a recurrence over precomputed
// gates: a ragged time view takes the cluster or the streaming branch, never the one that projects inside the kernel.
int resrnn(ws_engine* e, const RnnPrep& w, bool time_view, const float* z, int R, int Tf, const int* d_tf, float* out) {
  const int K = e->bs.K;
  ws_groups_geom geo = {};
  ws_seqmap sm = {};
  long long st_m1, st_m2;
  int st_div1, st_div2;
  if (time_view) {                       // band_rnn: sequences (r, k), steps over t
    geo.ngroups = R * K, geo.gdiv = 1, geo.gs1 = (long long)Tf * kN, geo.gs2 = 0, geo.rs = kN, geo.L = Tf;
    st_div1 = Tf, st_m1 = 1, st_div2 = 1, st_m2 = 0;
    sm.nseq = R * K, sm.sq_div = kBig, sm.sq_s1 = 0, sm.sq_s2 = Tf, sm.step_rows = 1, sm.L = Tf;
  } else {                               // band_comm: sequences (r, t), steps over k
    geo.ngroups = R * Tf, geo.gdiv = Tf, geo.gs1 = (long long)K * Tf * kN, geo.gs2 = kN, geo.rs = (long long)Tf * kN,
    geo.L = K;
    st_div1 = K * Tf, st_m1 = Tf, st_div2 = Tf, st_m2 = 1;
    sm.nseq = R * Tf, sm.sq_div = Tf, sm.sq_s1 = (long long)K * Tf, sm.sq_s2 = 1, sm.step_rows = Tf, sm.L = K;
  }
  geo.W = kN, geo.nbands = 1;
  const int ntile = (sm.nseq + 31) / 32;
  const size_t nb = size_t(ntile) * sm.L;
  const int lmode = 2 * ntile <= 128 ? WS_LSTM_BF16X3_BLK16 : WS_LSTM_BF16X3_BLK;
  static const bool no_cluster = getenv("WS_ENGINE_NO_CLUSTER") != nullptr;   // diagnostics: streaming kernels only
  const bool cluster = !no_cluster && sm.nseq % 64 == 0 && (sm.nseq / 32) * 8 <= e->cu_count && sm.L >= 64;
  const int* steps = time_view ? d_tf : nullptr;
  const bool fused = !cluster && lmode == WS_LSTM_BF16X3_BLK && !steps;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* stats = a.alloc(size_t(geo.ngroups) * 2);
  float* gates = a.alloc(nb * 32 * 2 * kG4);
  float* cbuf = a.alloc(nb * 32 * 2 * kH);
  float* hcat = a.alloc(nb * 32 * 2 * kH);
  float* xn = a.alloc(nb * 32 * kN);      // normalised input in BL(128): operand of the fused recurrence
  WS_PTR(stats && gates && cbuf && hcat && xn);
  if (steps)
    WS_RUN(e, ws_group_stats_len(z, &geo, steps, K, kGnEps, stats, s));
  else
    WS_RUN(e, ws_group_stats(z, &geo, kGnEps, stats, s));
  ws_gemm_p2b_args p = {};
  p.A = z;
  p.stats = stats;
  p.gamma = w.norm_w;
  p.beta = w.norm_b;
  p.sm = sm;
  p.lda = kN;
  p.st_div1 = st_div1, p.st_m1 = st_m1, p.st_div2 = st_div2, p.st_m2 = st_m2, p.st_base = 0;
  p.K = kN;
  p.A_bl = xn;
  if (fused) {          // the recurrence computes x W_ih^T itself from the normalised input in BL(128)
    p.N = 0;
    WS_RUN(e, ws_gemm_p2b(&p, s));
    ws_lstm_fused_args f = {};
    f.gates = gates, f.cbuf = cbuf, f.hcat = hcat, f.xn = xn, f.wpack = w.fpack, f.bias = w.bcat;
    f.nseq = sm.nseq, f.L = sm.L;
    WS_RUN(e, ws_lstm_fwd_fused(&f, s));
  } else {
    p.Wpack = w.wih_pack;
    p.bias = w.bcat;
    p.C = gates;
    p.N = 2 * kG4;
    if (steps)
      WS_RUN(e, ws_gemm_p2b_len(&p, steps, K, s));
    else
      WS_RUN(e, ws_gemm_p2b(&p, s));
    if (cluster) {
      const int ncl = sm.nseq / 32;
      float* xchg = a.alloc(size_t(ncl) * 2 * 8 * 8192 / 4);
      unsigned* flags = reinterpret_cast<unsigned*>(a.alloc(size_t(ncl) * 8 + 8));
      WS_PTR(xchg && flags);
      if (!e->cl_status) {
        e->cl_status = reinterpret_cast<unsigned*>(e->persist.alloc(2));
        WS_PTR(e->cl_status);
        if (zero_device(e, e->cl_status, 8) != WS_OK) return WS_ERR_LAUNCH;
      }
      ws_lstm_cluster_args c = {};
      c.gates = gates, c.cbuf = cbuf, c.hcat = hcat, c.whh_f = w.whf, c.whh_r = w.whr;
      c.xchg = xchg, c.flags = flags, c.nseq = sm.nseq, c.L = sm.L;
      c.status = e->cl_status;
      WS_RUN(e, ws_lstm_fwd_cluster(&c, s));
      // Several engines may share one GPU (separate_main --jobs): the cluster's workgroups are then not guaranteed to
      // be co-resident and a bounded wait can time out.  The streaming pair below is predicated on this launch's
      // timeout word: empty launches after a clean run, the whole layer again after a timeout -- never NaN.
      p.run_if = flags + size_t(ncl) * 8;
      if (steps)
        WS_RUN(e, ws_gemm_p2b_len(&p, steps, K, s));
      else
        WS_RUN(e, ws_gemm_p2b(&p, s));
      ws_lstm_args l = {};
      l.gates = gates, l.cbuf = cbuf, l.hcat = hcat;
      l.wpack = lmode == WS_LSTM_BF16X3_BLK16 ? w.pack16 : w.pack32;
      l.sq_s1 = sm.sq_s1, l.sq_s2 = sm.sq_s2, l.step_rows = sm.step_rows;
      l.nseq = sm.nseq, l.sq_div = sm.sq_div, l.L = sm.L, l.mode = lmode;
      l.run_if = p.run_if;
      WS_RUN(e, ws_lstm_fwd(&l, s));
    } else {
      ws_lstm_args l = {};
      l.gates = gates, l.cbuf = cbuf, l.hcat = hcat;
      l.wpack = lmode == WS_LSTM_BF16X3_BLK16 ? w.pack16 : w.pack32;
      l.sq_s1 = sm.sq_s1, l.sq_s2 = sm.sq_s2, l.step_rows = sm.step_rows;
      l.nseq = sm.nseq, l.sq_div = sm.sq_div, l.L = sm.L, l.mode = lmode;
      WS_RUN(e, ws_lstm_fwd(&l, s));
    }
  }
  ws_gemm_b2p_args b = {};
  b.A = hcat, b.Wpack = w.proj_pack, b.bias = w.proj_b, b.R = z, b.C = out, b.sm = sm, b.ldc = kN, b.N = kN, b.K = 2 * kH;
  WS_RUN(e, ws_gemm_b2p(&b, s));
  a.release(mk);
  return WS_OK;
}

// speaker fusion on Z (speaker.py:81-125, norm.py:118-139), in place
int fuse_layer(ws_engine* e, const std::string& pre, float* z, const float* emb, int R, int Tf) {
  const int K = e->bs.K, E = e->E;
  const long long P = (long long)R * K * Tf;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* v = a.alloc(size_t(R) * kN);
  float* v2 = a.alloc(size_t(R) * kN);
  WS_PTR(v && v2);
  int rc;
  if (e->bs.fuse == 3) {          // FiLM: (1 + gamma(e)) z + beta(e)
    if ((rc = linear(e, emb, R, E, e->dev(pre + "fc.gamma_fcs.0.weight"), E, kN, e->dev(pre + "fc.gamma_fcs.0.bias"), 0, v)) != WS_OK ||
        (rc = linear(e, emb, R, E, e->dev(pre + "fc.beta_fcs.0.weight"), E, kN, e->dev(pre + "fc.beta_fcs.0.bias"), 0, v2)) != WS_OK)
      return rc;
    WS_RUN(e, ws_affine_fwd(z, v, v2, 1.0f, P, K * Tf, kN, z, s));
  } else if (e->bs.fuse == 0) {   // concat: Linear(cat[z, e]) = z Wz^T + (e We^T + b)
    const float* W = e->dev(pre + "fc.linear.weight");
    if ((rc = linear(e, emb, R, E, W + kN, kN + E, kN, e->dev(pre + "fc.linear.bias"), 0, v)) != WS_OK) return rc;
    float* t = a.alloc(size_t(P) * kN);
    WS_PTR(t);
    ws_gemm_nt_args g = {};
    g.A = z, g.W = W, g.C = t;
    g.a_div = kBig, g.a_s2 = kN, g.c_div = kBig, g.c_s2 = kN, g.st_div1 = 1, g.st_div2 = 1;
    g.M = static_cast<int>(P), g.N = kN, g.K = kN, g.ldw = kN + E, g.vec = 3 | 4;
    WS_RUN(e, ws_gemm_nt(&g, s));
    WS_RUN(e, ws_affine_fwd(t, nullptr, v, 1.0f, P, K * Tf, kN, z, s));
  } else {
    if ((rc = linear(e, emb, R, E, e->dev(pre + "fc.linear.weight"), E, kN, e->dev(pre + "fc.linear.bias"), 0, v)) != WS_OK)
      return rc;
    if (e->bs.fuse == 2)
      WS_RUN(e, ws_affine_fwd(z, v, nullptr, 0.0f, P, K * Tf, kN, z, s));     // multiply
    else
      WS_RUN(e, ws_affine_fwd(z, nullptr, v, 1.0f, P, K * Tf, kN, z, s));     // additive
  }
  a.release(mk);
  return WS_OK;
}

// BSRNN.forward (bsrnn.py:300-394) with the embedding already computed: wav [R][T], emb [R][E] -> est [R][T] (device).
// d_len / d_tf (ragged batches, both or neither): device tables [R] of the rows' valid samples and frames (1 + len / 128).
// The length is known where a row's end matters -- reflect padding, the three GroupNorms over time, the start of the
// reverse time-view recurrence, the iSTFT envelope -- everything else runs over the rectangle; the frames behind a row's
// end hold finite values nothing valid reads.
int separate_device(ws_engine* e, const float* wav, int R, int T, const float* emb_in, float* est, const int* d_len,
                    const int* d_tf) {
  const int K = e->bs.K, Tf = 1 + T / kHop, H1 = 4 * kN;
  const long long M = (long long)R * Tf;
  void* s = e->stream;
  Arena& a = e->work;
  int rc = build_descriptors(e, R, Tf);
  if (rc != WS_OK) return rc;
  ws_bands bands = {e->bs.d_band_of_bin, e->bs.d_f0, e->bs.d_bw, K, kNBin};
  float* xbs = a.alloc(size_t(M) * 2 * kNBin);
  float* zA = a.alloc(size_t(R) * K * Tf * kN);
  float* zB = a.alloc(size_t(R) * K * Tf * kN);
  WS_PTR(xbs && zA && zB);
  // STFT + band split + per-band GroupNorm + Conv1d(k = 1)   (bsrnn.py:309-337)
  if (d_len)
    WS_RUN(e, ws_stft_bandsplit_len(wav, R, T, d_len, &bands, xbs, s));
  else
    WS_RUN(e, ws_stft_bandsplit(wav, R, T, &bands, xbs, s));
  {
    const Arena::Mark mk = a.mark();
    float* stats = a.alloc(size_t(R) * K * 2);
    WS_PTR(stats);
    ws_groups_geom geo = {};
    geo.band_w = e->bs.d_bw2, geo.band_off = e->bs.d_off2;
    geo.gs1 = (long long)Tf * 2 * kNBin, geo.gs2 = 0, geo.rs = 2 * kNBin;
    geo.ngroups = R * K, geo.gdiv = K, geo.L = Tf, geo.W = 128, geo.nbands = K;
    if (d_tf)
      WS_RUN(e, ws_group_stats_len(xbs, &geo, d_tf, K, kGnEps, stats, s));
    else
      WS_RUN(e, ws_group_stats(xbs, &geo, kGnEps, stats, s));
    ws_gemm_nt_args g = {};
    g.A = xbs, g.C = zA, g.stats = stats, g.groups = e->bs.d_bn;
    g.a_div = kBig, g.a_s2 = 2 * kNBin;
    g.c_div = Tf, g.c_s1 = (long long)K * Tf * kN, g.c_s2 = kN;
    g.st_div1 = Tf, g.st_m1 = K, g.st_div2 = 1, g.st_m2 = 0;
    g.M = static_cast<int>(M), g.ngroups = K, g.max_n = kN, g.vec = 0 | 4;
    WS_RUN(e, ws_gemm_nt(&g, s));
    a.release(mk);
  }
  // speaker embedding -> (optional) SpeakerTransform (speaker.py:26-49)
  const float* emb = emb_in;
  if ((rc = spk_transform(e, emb, R, &emb)) != WS_OK) return rc;
  // separator (bsrnn.py:86-148)
  float* z = zA;
  float* other = zB;
  size_t net = 0;
  for (size_t i = 0; i < e->bs.sep_kind.size(); ++i) {
    if (e->bs.sep_kind[i] == 0) {
      if ((rc = fuse_layer(e, "separator.separation." + std::to_string(i) + ".", z, emb, R, Tf)) != WS_OK) return rc;
    } else {
      if ((rc = resrnn(e, e->bs.rnn[2 * net], true, z, R, Tf, d_tf, other)) != WS_OK) return rc;
      if ((rc = resrnn(e, e->bs.rnn[2 * net + 1], false, other, R, Tf, d_tf, z)) != WS_OK) return rc;
      ++net;
    }
  }
  // mask MLP + GLU complex mask + iSTFT (bsrnn.py:366-392)
  {
    const Arena::Mark mk = a.mark();
    float* stats = a.alloc(size_t(R) * K * 2);
    float* h1 = a.alloc(size_t(K) * M * H1);
    float* h2 = a.alloc(size_t(K) * M * H1);
    float* m3 = a.alloc(size_t(M) * 4 * kNBin);
    float* frames = a.alloc(size_t(M) * 512);
    WS_PTR(stats && h1 && h2 && m3 && frames);
    ws_groups_geom geo = {};
    geo.gs1 = (long long)Tf * kN, geo.gs2 = 0, geo.rs = kN;
    geo.ngroups = R * K, geo.gdiv = 1, geo.L = Tf, geo.W = kN, geo.nbands = K;
    if (d_tf)
      WS_RUN(e, ws_group_stats_len(z, &geo, d_tf, K, kGnEps, stats, s));
    else
      WS_RUN(e, ws_group_stats(z, &geo, kGnEps, stats, s));
    int maxbw = 0;
    for (int b : e->bs.bw) maxbw = b > maxbw ? b : maxbw;
    ws_gemm_nt_args g = {};
    g.A = z, g.C = h1, g.stats = stats, g.groups = e->bs.d_l1;
    g.a_div = Tf, g.a_s1 = (long long)K * Tf * kN, g.a_s2 = kN;
    g.c_div = kBig, g.c_s2 = H1;
    g.st_div1 = Tf, g.st_m1 = K, g.st_div2 = 1, g.st_m2 = 0;
    g.M = static_cast<int>(M), g.act = 1, g.ngroups = K, g.max_n = H1, g.vec = 3 | 4;
    WS_RUN(e, ws_gemm_nt(&g, s));
    ws_gemm_nt_args g2 = {};
    g2.A = h1, g2.C = h2, g2.groups = e->bs.d_l2;
    g2.a_div = kBig, g2.a_s2 = H1, g2.c_div = kBig, g2.c_s2 = H1, g2.st_div1 = 1, g2.st_div2 = 1;
    g2.M = static_cast<int>(M), g2.act = 1, g2.ngroups = K, g2.max_n = H1, g2.vec = 3 | 4;
    WS_RUN(e, ws_gemm_nt(&g2, s));
    ws_gemm_nt_args g3 = {};
    g3.A = h2, g3.C = m3, g3.groups = e->bs.d_l3;
    g3.a_div = kBig, g3.a_s2 = H1, g3.c_div = kBig, g3.c_s2 = 4 * kNBin, g3.st_div1 = 1, g3.st_div2 = 1;
    g3.M = static_cast<int>(M), g3.ngroups = K, g3.max_n = 4 * maxbw, g3.vec = 3 | 4;
    WS_RUN(e, ws_gemm_nt(&g3, s));
    WS_RUN(e, ws_mask_istft_frames(xbs, m3, R, Tf, &bands, frames, s));
    if (d_len)
      WS_RUN(e, ws_istft_ola_len(frames, R, Tf, T, d_len, est, s));
    else
      WS_RUN(e, ws_istft_ola(frames, R, Tf, T, est, s));
    a.release(mk);
  }
  return WS_OK;
}

}  // namespace wsrt
