// =================================================================================================================
// TF-GridNet (arch 3): the launch plan of wesep_amd/models/tfgridnet.py (wesep/models/tfgridnet.py:197-302,
// wesep/modules/tfgridnet/gridnet_block.py:118-227) for the shipped recipe's geometry -- one microphone, one source,
// emb_dim 128, emb_ks = emb_hs = 1, lstm_hidden_units <= 256 (zero-padded to the 256 units the recurrence kernels are
// built for), 4 heads.  STFT / iSTFT as DFT-basis GEMMs like the DPCCN plan; Conv2d(2 -> C) + GroupNorm(1, C); per
// block: speaker fusion, the intra-frame path (row LayerNorm, BLSTM over the bins of a frame on the blocked-layout
// kernels of the pBSRNN plan, Linear + residual in the output GEMM), the inter-frame path (the same on a STRIDED
// sequence map: sequence (b, q) walks the frames -- the Python path transposes the map twice instead), attention (one
// projection GEMM for Q / K / V, ws_heads_fwd, grouped logits GEMM with the padded keys masked, row softmax, grouped
// value GEMM, head merge, projection + PReLU + LayerNorm over (bins, channels), residual); ConvTranspose2d(C -> 2).
// The mixture is scaled by its standard deviation on the host (tfgridnet.py:222-226), the estimate scaled back.
// Ragged batches: with per-row lengths the same plan runs over the rectangle; the row's frame count
// Tf_r = 1 + lengths[r] / hop goes to the reflect padding, the zero frames the two 3x3 convolutions read behind a row's
// end, the GroupNorm statistics, the inter-frame BLSTM's gates, the key mask and the overlap-add -- nowhere else.
// =================================================================================================================
#include "engine_internal.h"

namespace wsrt {

// nn.LSTM tensors of hidden size h -> the 256-unit layout (functional_tfgridnet.pad_lstm): gate-major rows g*256 + u
int grid_prep_rnn(ws_engine* e, const std::string& path, int C, int h, RnnPrep* r) {
  static const char* sfx[2] = {"", "_reverse"};
  const std::string rnn = path + "rnn.";
  float* dev_w[2][3];                    // per direction: w_ih [1024][C], w_hh [1024][256], b [1024]
  for (int d = 0; d < 2; ++d) {
    const std::string s = sfx[d];
    if (!require(e, rnn + "weight_ih_l0" + s, {4 * h, C}) || !require(e, rnn + "weight_hh_l0" + s, {4 * h, h}) ||
        !require(e, rnn + "bias_ih_l0" + s, {4 * h}) || !require(e, rnn + "bias_hh_l0" + s, {4 * h}))
      return WS_ERR_INVALID;
    const float *wi = e->host(rnn + "weight_ih_l0" + s), *wh = e->host(rnn + "weight_hh_l0" + s);
    const float *bi = e->host(rnn + "bias_ih_l0" + s), *bh = e->host(rnn + "bias_hh_l0" + s);
    std::vector<float> wip(size_t(kG4) * C, 0.f), whp(size_t(kG4) * kH, 0.f), bp(kG4, 0.f);
    for (int g = 0; g < 4; ++g)
      for (int u = 0; u < h; ++u) {
        const size_t src = size_t(g) * h + u, dst = size_t(g) * kH + u;
        memcpy(&wip[dst * C], wi + src * C, size_t(C) * 4);
        memcpy(&whp[dst * kH], wh + src * h, size_t(h) * 4);
        bp[dst] = bi[src] + bh[src];
      }
    dev_w[d][0] = upload(e, e->persist, wip.data(), wip.size());
    dev_w[d][1] = upload(e, e->persist, whp.data(), whp.size());
    dev_w[d][2] = upload(e, e->persist, bp.data(), bp.size());
    WS_PTR(dev_w[d][0] && dev_w[d][1] && dev_w[d][2]);
  }
  if (!require(e, path + "norm.weight", {C}) || !require(e, path + "norm.bias", {C}) ||
      !require(e, path + "linear.weight", {C, 2 * h}) || !require(e, path + "linear.bias", {C}))
    return WS_ERR_INVALID;
  // Linear(2h -> C): each half of the hidden columns zero-padded to 256 (pad_hidden_cols)
  std::vector<float> lin(size_t(C) * 2 * kH, 0.f), zero(kG4, 0.f);
  const float* lw = e->host(path + "linear.weight");
  for (int n = 0; n < C; ++n) {
    memcpy(&lin[size_t(n) * 2 * kH], lw + size_t(n) * 2 * h, size_t(h) * 4);
    memcpy(&lin[size_t(n) * 2 * kH + kH], lw + size_t(n) * 2 * h + h, size_t(h) * 4);
  }
  float* dlin = upload(e, e->persist, lin.data(), lin.size());
  float* dzero = upload(e, e->persist, zero.data(), zero.size());
  WS_PTR(dlin && dzero);
  r->norm_w = e->dev(path + "norm.weight"), r->norm_b = e->dev(path + "norm.bias"), r->proj_b = e->dev(path + "linear.bias");
  r->whf = dev_w[0][1], r->whr = dev_w[1][1];
  const float* bias[4] = {dev_w[0][2], dzero, dev_w[1][2], dzero};
  return pack_rnn(e, C, dev_w[0][0], dev_w[1][0], bias, dlin, r);
}

int prepare_gridnet(ws_engine* e) {
  GridNet& n = e->grid;
  int rc = read_speaker_meta(e);
  if (rc != WS_OK) return rc;
  n.n_fft = static_cast<int>(meta_or(e, "n_fft", 128)), n.hop = static_cast<int>(meta_or(e, "stride", 64));
  n.Q = n.n_fft / 2 + 1, n.C = static_cast<int>(meta_or(e, "emb_dim", 128)), n.hid = static_cast<int>(meta_or(e, "lstm_hidden_units", 192));
  n.nh = static_cast<int>(meta_or(e, "attn_n_head", 4)), n.E = static_cast<int>(meta_or(e, "attn_E", 8));
  n.layers = static_cast<int>(meta_or(e, "n_layers", 6)), n.fuse = static_cast<int>(meta_or(e, "spk_fuse_type", 2));
  const int C = n.C, Q = n.Q, nh = n.nh, E = n.E, cp = C / (nh > 0 ? nh : 1);
  if (meta_or(e, "emb_ks", 1) != 1 || meta_or(e, "emb_hs", 1) != 1 || meta_or(e, "n_srcs", 1) != 1 || meta_or(e, "n_imics", 1) != 1 ||
      C != kN || n.hid < 4 || n.hid > kH || n.hid % 4 || nh < 1 || nh > 8 || C % nh || E % 4 || cp % 4 || n.n_fft % 8 ||
      n.n_fft < 16 || n.n_fft > 1024 || n.hop * 2 != n.n_fft || (long long)Q * C > 9216 || n.fuse < 0 || n.fuse > 3 ||
      n.layers < 1 || e->E % 4 || e->spk.feat_dim % 8) {
    set_err("engine: the TF-GridNet plan is built for the recipe's geometry (emb_dim 128, emb_ks = emb_hs = 1, one microphone "
            "and source, hidden <= 256 and %% 4, heads <= 8 with widths %% 4, stride = n_fft / 2, (n_fft / 2 + 1) * 128 <= 9216, "
            "concat / multiply / additive / FiLM fusion)");
    return WS_ERR_INVALID;
  }
  e->dw = upload(e, e->persist, e->hw.data(), e->hw.size());
  WS_PTR(e->dw);
  if (!require(e, "conv.0.weight", {C, 2, 3, 3}) || !require(e, "conv.0.bias", {C}) || !require(e, "conv.1.weight", {C}) ||
      !require(e, "conv.1.bias", {C}) || !require(e, "deconv.weight", {C, 2, 3, 3}) || !require(e, "deconv.bias", {2}))
    return WS_ERR_INVALID;
  if (n.fuse == 3) {
    if (!require(e, "spk_fuse.fc.gamma_fcs.0.weight", {Q, e->E}) || !require(e, "spk_fuse.fc.gamma_fcs.0.bias", {Q}) ||
        !require(e, "spk_fuse.fc.beta_fcs.0.weight", {Q, e->E}) || !require(e, "spk_fuse.fc.beta_fcs.0.bias", {Q}))
      return WS_ERR_INVALID;
    std::vector<float> b1(e->host("spk_fuse.fc.gamma_fcs.0.bias"), e->host("spk_fuse.fc.gamma_fcs.0.bias") + Q);
    for (float& v : b1) v += 1.0f;
    n.film_bias1 = upload(e, e->persist, b1.data(), b1.size());
    WS_PTR(n.film_bias1);
  } else if (!require(e, "spk_fuse.fc.linear.weight", {Q, n.fuse == 0 ? Q + e->E : e->E}) || !require(e, "spk_fuse.fc.linear.bias", {Q})) {
    return WS_ERR_INVALID;     // (concat: Linear over the frequency axis of cat[x, e], speaker.py:95-101)
  }
  if ((rc = dp_io_convs(e, "conv.0.", C, "deconv.", C, &n.w_in, &n.w_out, &n.b_out)) != WS_OK) return rc;
  if ((rc = dft_bases(e, n.n_fft, &n.ana4, &n.syn4)) != WS_OK) return rc;
  {
    std::vector<float> ones(size_t(Q) * C, 1.f), zeros(size_t(Q) * C, 0.f), id(size_t(2) * C, 0.f);
    for (int c = 0; c < C; ++c) id[C + c] = 1.f;                        // (mean 0 | rstd 1)
    const float one = 1.f;
    n.ones_qc = upload(e, e->persist, ones.data(), ones.size());
    n.zeros_qc = upload(e, e->persist, zeros.data(), zeros.size());
    n.id_st = upload(e, e->persist, id.data(), id.size());
    n.slope1 = upload(e, e->persist, &one, 1);
    WS_PTR(n.ones_qc && n.zeros_qc && n.id_st && n.slope1);
    n.ones_c = n.ones_qc, n.zeros_c = n.zeros_qc;                       // any prefix of C elements
  }
  n.blocks.resize(n.layers);
  for (int l = 0; l < n.layers; ++l) {
    GridBlock& b = n.blocks[l];
    const std::string p = "blocks." + std::to_string(l) + ".";
    // nn.Module names: intra_norm / intra_rnn / intra_linear -> one prefix per path
    for (int path = 0; path < 2; ++path) {
      const std::string q = p + (path ? "inter_" : "intra_");
      // grid_prep_rnn reads <q>norm., <q>rnn., <q>linear.
      if ((rc = grid_prep_rnn(e, q, C, n.hid, path ? &b.inter : &b.intra)) != WS_OK) return rc;
    }
    const char* proj[3] = {"attn_conv_Q.", "attn_conv_K.", "attn_conv_V."};
    const char* norm[3] = {"attn_norm_Q.", "attn_norm_K.", "attn_norm_V."};
    const int width[3] = {nh * E, nh * E, C}, chs[3] = {E, E, cp};
    const int ld = 2 * nh * E + C;
    std::vector<float> wq(size_t(ld) * C), bq(ld);
    int row = 0;
    for (int j = 0; j < 3; ++j) {
      if (!require(e, p + proj[j] + "weight", {width[j], C, 1, 1}) || !require(e, p + proj[j] + "bias", {width[j]}) ||
          !require(e, p + norm[j] + "gamma", {1, nh, chs[j], 1, Q}) || !require(e, p + norm[j] + "beta", {1, nh, chs[j], 1, Q}) ||
          !require(e, p + norm[j] + "act.weight", {nh}))
        return WS_ERR_INVALID;
      memcpy(&wq[size_t(row) * C], e->host(p + proj[j] + "weight"), size_t(width[j]) * C * 4);
      memcpy(&bq[row], e->host(p + proj[j] + "bias"), size_t(width[j]) * 4);
      row += width[j];
      const int ch = chs[j];
      std::vector<float> g(size_t(nh) * Q * ch), bt(size_t(nh) * Q * ch);
      const float *gs = e->host(p + norm[j] + "gamma"), *bs = e->host(p + norm[j] + "beta");
      for (int h = 0; h < nh; ++h)
        for (int ee = 0; ee < ch; ++ee)
          for (int q = 0; q < Q; ++q) {
            g[(size_t(h) * Q + q) * ch + ee] = gs[(size_t(h) * ch + ee) * Q + q];
            bt[(size_t(h) * Q + q) * ch + ee] = bs[(size_t(h) * ch + ee) * Q + q];
          }
      b.gam[j] = upload(e, e->persist, g.data(), g.size());
      b.bet[j] = upload(e, e->persist, bt.data(), bt.size());
      WS_PTR(b.gam[j] && b.bet[j]);
    }
    b.wqkv = upload(e, e->persist, wq.data(), wq.size());
    b.bqkv = upload(e, e->persist, bq.data(), bq.size());
    WS_PTR(b.wqkv && b.bqkv);
    if (!require(e, p + "attn_concat_proj.0.weight", {C, C, 1, 1}) || !require(e, p + "attn_concat_proj.0.bias", {C}) ||
        !require(e, p + "attn_concat_proj.1.weight", {1}) || !require(e, p + "attn_concat_proj.2.gamma", {1, C, 1, Q}) ||
        !require(e, p + "attn_concat_proj.2.beta", {1, C, 1, Q}))
      return WS_ERR_INVALID;
    std::vector<float> pg(size_t(Q) * C), pb(size_t(Q) * C);
    const float *gs = e->host(p + "attn_concat_proj.2.gamma"), *bs = e->host(p + "attn_concat_proj.2.beta");
    for (int c = 0; c < C; ++c)
      for (int q = 0; q < Q; ++q) {
        pg[size_t(q) * C + c] = gs[size_t(c) * Q + q];
        pb[size_t(q) * C + c] = bs[size_t(c) * Q + q];
      }
    b.proj_g = upload(e, e->persist, pg.data(), pg.size());
    b.proj_b = upload(e, e->persist, pb.data(), pb.size());
    WS_PTR(b.proj_g && b.proj_b);
  }
  return prep_speaker(e);
}

// out = res + Linear(BLSTM(xn)) on the sequences of `sm` (rows of 128 features; xn = the layer-normed rows): the body of
// resrnn() without its GroupNorm (functional_tfgridnet.BlstmLinearBlkFn).  steps (device, ragged inter-frame path): sequence
// s has steps[s / steps_div] valid steps -- the gates behind them are zeros (ws_gemm_p2b_len), so the reverse direction
// reaches a row's last frame with zero state; only the branches over precomputed gates know such a table
int grid_rnn(ws_engine* e, const RnnPrep& w, const ws_seqmap& sm, const float* xn_rows, const float* res, float* out,
             const int* steps = nullptr, int steps_div = 1) {
  const int ntile = (sm.nseq + 31) / 32;
  const size_t nb = size_t(ntile) * sm.L;
  const int lmode = 2 * ntile <= 128 ? WS_LSTM_BF16X3_BLK16 : WS_LSTM_BF16X3_BLK;
  static const bool no_cluster = getenv("WS_ENGINE_NO_CLUSTER") != nullptr;
  const bool cluster = !no_cluster && sm.nseq % 64 == 0 && (sm.nseq / 32) * 8 <= e->cu_count && sm.L >= 64;
  const bool fused = !cluster && lmode == WS_LSTM_BF16X3_BLK && !steps;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* gates = a.alloc(nb * 32 * 2 * kG4);
  float* cbuf = a.alloc(nb * 32 * 2 * kH);
  float* hcat = a.alloc(nb * 32 * 2 * kH);
  float* xn = a.alloc(nb * 32 * kN);
  WS_PTR(gates && cbuf && hcat && xn);
  ws_gemm_p2b_args p = {};
  p.A = xn_rows, p.sm = sm, p.lda = kN, p.K = kN, p.A_bl = xn;
  p.st_div1 = 1, p.st_m1 = 0, p.st_div2 = 1, p.st_m2 = 0, p.st_base = 0;
  if (fused) {
    p.N = 0;
    WS_RUN(e, ws_gemm_p2b(&p, s));
    ws_lstm_fused_args f = {};
    f.gates = gates, f.cbuf = cbuf, f.hcat = hcat, f.xn = xn, f.wpack = w.fpack, f.bias = w.bcat;
    f.nseq = sm.nseq, f.L = sm.L;
    WS_RUN(e, ws_lstm_fwd_fused(&f, s));
  } else {
    p.Wpack = w.wih_pack, p.bias = w.bcat, p.C = gates, p.N = 2 * kG4;
    if (steps)
      WS_RUN(e, ws_gemm_p2b_len(&p, steps, steps_div, s));
    else
      WS_RUN(e, ws_gemm_p2b(&p, s));
    ws_lstm_args l = {};
    l.gates = gates, l.cbuf = cbuf, l.hcat = hcat;
    l.wpack = lmode == WS_LSTM_BF16X3_BLK16 ? w.pack16 : w.pack32;
    l.sq_s1 = sm.sq_s1, l.sq_s2 = sm.sq_s2, l.step_rows = sm.step_rows;
    l.nseq = sm.nseq, l.sq_div = sm.sq_div, l.L = sm.L, l.mode = lmode;
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
      c.xchg = xchg, c.flags = flags, c.nseq = sm.nseq, c.L = sm.L, c.status = e->cl_status;
      WS_RUN(e, ws_lstm_fwd_cluster(&c, s));
      p.run_if = flags + size_t(ncl) * 8;      // the streaming pair repeats the layer only after a cluster time-out
      if (steps)
        WS_RUN(e, ws_gemm_p2b_len(&p, steps, steps_div, s));
      else
        WS_RUN(e, ws_gemm_p2b(&p, s));
      l.run_if = p.run_if;
    }
    WS_RUN(e, ws_lstm_fwd(&l, s));
  }
  ws_gemm_b2p_args b = {};
  b.A = hcat, b.Wpack = w.proj_pack, b.bias = w.proj_b, b.R = res, b.C = out, b.sm = sm, b.ldc = kN, b.N = kN, b.K = 2 * kH;
  WS_RUN(e, ws_gemm_b2p(&b, s));
  a.release(mk);
  return WS_OK;
}

// the group table of grid_bmm on the device (an upload: it synchronises the stream).  bias_rows = 0: every group adds
// bias[N]; else group g adds row g % bias_rows of bias [bias_rows][N] (the ragged key mask of row r = g % R)
ws_group_nt* grid_bmm_table(ws_engine* e, const float* W, const float* bias, int bias_rows, int G, int M, int K, int N) {
  std::vector<ws_group_nt> tab(G);
  for (int g = 0; g < G; ++g) {
    ws_group_nt d = {};
    d.W = W + size_t(g) * N * K, d.a_off = (long long)g * M * K, d.c_off = (long long)g * M * N;
    d.bias = bias && bias_rows ? bias + size_t(g % bias_rows) * N : bias;
    d.K = K, d.N = N, d.ldw = K;
    tab[g] = d;
  }
  const size_t nf = (sizeof(ws_group_nt) * G + 3) / 4;
  ws_group_nt* dt = reinterpret_cast<ws_group_nt*>(e->work.alloc(nf));
  if (!dt || to_device(e, dt, tab.data(), sizeof(ws_group_nt) * G) != WS_OK) return nullptr;
  return dt;
}

// C[g][M][N] = A[g][M][K] W[g][N][K]^T (+ bias[N]) for G groups in one launch (functional_tfgridnet.BatchedMatmulNTFn);
// dt: a table built before (the ragged plan uploads both of its tables once, ahead of the first launch), or NULL
int grid_bmm(ws_engine* e, const float* A, const float* W, const float* bias, int G, int M, int K, int N, float* C,
             const ws_group_nt* dt = nullptr) {
  if (!dt) dt = grid_bmm_table(e, W, bias, 0, G, M, K, N);
  WS_PTR(dt);
  ws_gemm_nt_args g = {};
  g.A = A, g.C = C, g.groups = dt;
  g.a_div = kBig, g.a_s2 = K, g.c_div = kBig, g.c_s2 = N, g.st_div1 = 1, g.st_div2 = 1;
  g.M = M, g.ngroups = G, g.max_n = N;
  g.vec = ((K % 4 == 0 && ((long long)M * K) % 4 == 0) ? 3 : 0) | 4;
  WS_RUN(e, ws_gemm_nt(&g, e->stream));
  return WS_OK;
}

// wav [R][T] (already divided by its standard deviation), emb [R][E] -> est [R][T] (still in normalised units)
int gridnet_device(ws_engine* e, const float* wav, int R, int T, const float* emb_in, float* est, const int* h_tf,
                   const int* d_len, const int* d_tf) {
  const GridNet& n = e->grid;
  const int nf = n.n_fft, hop = n.hop, pad = nf / 2, Tf = 1 + T / hop, Q = n.Q, C = n.C, nh = n.nh, E = n.E, cp = C / nh;
  const int ld4 = 4 * Q, Tp = (Tf + 3) / 4 * 4, G = nh * R, D = Q * E, Dv = Q * cp, ldq = 2 * nh * E + C;
  const long long M = (long long)R * Tf * Q;
  void* s = e->stream;
  Arena& a = e->work;
  int rc;
  const bool ragged = h_tf != nullptr;
  if (ragged && !(d_len && d_tf)) {
    set_err("engine: the ragged TF-GridNet plan needs the host and both device length tables");
    return WS_ERR_INVALID;
  }
  // ---- STFT ----
  const int ldo = (T + 2 * pad + 3) / 4 * 4;
  float* xp = a.alloc(size_t(R) * ldo);
  float* spec4 = a.alloc(size_t(R) * Tf * ld4);
  float* hA = a.alloc(size_t(M) * C);
  float* hB = a.alloc(size_t(M) * C);
  float* hC = a.alloc(size_t(M) * C);
  WS_PTR(xp && spec4 && hA && hB && hC);
  // ---- ragged: every table of the forward goes up before the first launch (an upload synchronises the stream), so the
  //      attention's operands live outside the block loop and their two group tables are built once ----
  float *mask = nullptr, *win = nullptr, *Qa = nullptr, *Ka = nullptr, *VaT = nullptr, *logits = nullptr, *att = nullptr, *ov = nullptr;
  const ws_group_nt *tab_qk = nullptr, *tab_av = nullptr;
  if (ragged) {
    std::vector<float> mask_h(size_t(R) * Tp, 0.f), win_h(nf);
    for (int r = 0; r < R; ++r)
      for (int t = h_tf[r]; t < Tp; ++t) mask_h[size_t(r) * Tp + t] = -1e30f;       // keys behind the row's own frames
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < nf; ++k) win_h[k] = static_cast<float>(0.5 - 0.5 * cos(2.0 * pi * k / nf));   // as dft_istft's envelope
    mask = upload(e, a, mask_h.data(), mask_h.size());
    win = upload(e, a, win_h.data(), win_h.size());
    Qa = a.alloc(size_t(G) * Tf * D), Ka = a.alloc(size_t(G) * Tp * D), VaT = a.alloc(size_t(G) * Tp * Dv);
    logits = a.alloc(size_t(G) * Tf * Tp), att = a.alloc(size_t(G) * Tf * Tp), ov = a.alloc(size_t(G) * Tf * Dv);
    WS_PTR(mask && win && Qa && Ka && VaT && logits && att && ov);
    tab_qk = grid_bmm_table(e, Ka, mask, R, G, Tf, D, Tp);          // group (head, r) = head * R + r reads mask row r
    tab_av = grid_bmm_table(e, VaT, nullptr, 0, G, Tf, Tp, Dv);
    WS_PTR(tab_qk && tab_av);
  }
  if ((rc = zero_device(e, xp, size_t(R) * ldo * 4)) != WS_OK) return rc;
  if (ragged)      // the reflect padding turns at the row's own end; nothing behind lengths[r] is read
    WS_RUN(e, ws_preemph_pad_len(wav, R, T, pad, ldo, 0.0f, d_len, xp, s));
  else
    WS_RUN(e, ws_preemph_pad(wav, R, T, pad, ldo, 0.0f, xp, s));
  {
    ws_gemm_nt_args g = {};
    g.A = xp, g.W = n.ana4, g.C = spec4;
    g.a_div = Tf, g.a_s1 = ldo, g.a_s2 = hop, g.c_div = kBig, g.c_s2 = ld4, g.st_div1 = 1, g.st_div2 = 1;
    g.M = R * Tf, g.N = ld4, g.K = nf, g.ldw = nf, g.vec = 3;
    WS_RUN(e, ws_gemm_nt(&g, s));
  }
  // frame Tf_r still overlaps the reflected samples: the 3x3 convolution reads zeros there, as its padding on the row alone
  if (ragged) WS_RUN(e, ws_tail_select_len(spec4, R, Tf, ld4, d_tf, spec4, s));
  // ---- Conv2d(2 -> C) + GroupNorm(1, C) ----
  if ((rc = dp_conv_view(e, spec4, R, Tf, Q, 4, 0, Q, 1, n.w_in, C, e->dev("conv.0.bias"), hB, C)) != WS_OK) return rc;
  {
    float* st = a.alloc(size_t(R) * 2);
    WS_PTR(st);
    if (ragged) {                          // over the row's own frames; the chunk count of tas_flat_stats
      const long long npg = (long long)Tf * Q * C;
      int nchunk = static_cast<int>(npg / 16384);
      const int cap = 512 / R > 1 ? 512 / R : 1;
      if (nchunk > cap) nchunk = cap;
      if (nchunk < 1) nchunk = 1;
      float* scratch = a.alloc(size_t(R) * nchunk * 4);
      WS_PTR(scratch);
      WS_RUN(e, ws_flat_stats_len(hB, R, npg, d_tf, Q * C, kLnEps, nchunk, scratch, st, s));
    } else if ((rc = tas_flat_stats(e, hB, R, (long long)Tf * Q * C, st)) != WS_OK) {
      return rc;
    }
    WS_RUN(e, ws_dwconv_fwd(hB, st, e->dev("conv.1.weight"), e->dev("conv.1.bias"), n.ones_c, n.zeros_c, R, Tf * Q, C, 1, 1, Tf * Q,
                            hA, s));
  }
  // ---- speaker fusion operands (the same before every block) ----
  const float* emb = emb_in;
  if ((rc = spk_transform(e, emb, R, &emb)) != WS_OK) return rc;
  float* sf = a.alloc(size_t(R) * Q);
  float* bt = n.fuse == 3 ? a.alloc(size_t(R) * Q) : nullptr;
  WS_PTR(sf && (n.fuse != 3 || bt));
  if (n.fuse == 3) {
    if ((rc = linear(e, emb, R, e->E, e->dev("spk_fuse.fc.gamma_fcs.0.weight"), e->E, Q, n.film_bias1, 0, sf)) != WS_OK ||
        (rc = linear(e, emb, R, e->E, e->dev("spk_fuse.fc.beta_fcs.0.weight"), e->E, Q, e->dev("spk_fuse.fc.beta_fcs.0.bias"), 0, bt)) != WS_OK)
      return rc;
  } else if (n.fuse == 0) {      // concat: the embedding's share of the Linear, We e + bias; the x share runs per block below
    if ((rc = linear(e, emb, R, e->E, e->dev("spk_fuse.fc.linear.weight") + Q, Q + e->E, Q, e->dev("spk_fuse.fc.linear.bias"), 0, sf)) != WS_OK)
      return rc;
  } else if ((rc = linear(e, emb, R, e->E, e->dev("spk_fuse.fc.linear.weight"), e->E, Q, e->dev("spk_fuse.fc.linear.bias"), 0, sf)) != WS_OK) {
    return rc;
  }
  if (!ragged) {
    std::vector<float> mask_h(Tp, 0.f);
    for (int t = Tf; t < Tp; ++t) mask_h[t] = -1e30f;
    mask = upload(e, a, mask_h.data(), mask_h.size());
    WS_PTR(mask);
  }
  ws_seqmap intra = {}, inter = {};
  intra.nseq = R * Tf, intra.sq_div = kBig, intra.sq_s1 = 0, intra.sq_s2 = Q, intra.step_rows = 1, intra.L = Q;
  inter.nseq = R * Q, inter.sq_div = Q, inter.sq_s1 = (long long)Tf * Q, inter.sq_s2 = 1, inter.step_rows = Q, inter.L = Tf;
  float* h = hA;                          // block input / output; hB, hC rotate as scratch
  for (int l = 0; l < n.layers; ++l) {
    const GridBlock& b = n.blocks[l];
    const std::string p = "blocks." + std::to_string(l) + ".";
    const Arena::Mark mk = a.mark();
    float* x = hB;                         // fused input
    if (n.fuse == 3) {
      WS_RUN(e, ws_scale_bf_fwd(h, sf, R, Tf, Q, C, 0, hC, s));
      WS_RUN(e, ws_scale_bf_fwd(hC, bt, R, Tf, Q, C, 1, x, s));
    } else if (n.fuse == 0) {
      WS_RUN(e, ws_freq_linear_fwd(h, e->dev("spk_fuse.fc.linear.weight"), Q + e->E, sf, R, Tf, Q, C, x, s));
    } else {
      WS_RUN(e, ws_scale_bf_fwd(h, sf, R, Tf, Q, C, n.fuse == 2 ? 0 : 1, x, s));
    }
    float* y = a.alloc(size_t(M) * C);
    float* lnst = a.alloc(size_t(M) * 2);
    WS_PTR(y && lnst);
    // intra-frame path: x -> hC
    WS_RUN(e, ws_rowln_fwd(x, b.intra.norm_w, b.intra.norm_b, M, C, kLnEps, y, lnst, s));
    if ((rc = grid_rnn(e, b.intra, intra, y, x, hC)) != WS_OK) return rc;
    // inter-frame path: hC -> x  (strided sequences: no transposes)
    WS_RUN(e, ws_rowln_fwd(hC, b.inter.norm_w, b.inter.norm_b, M, C, kLnEps, y, lnst, s));
    if ((rc = grid_rnn(e, b.inter, inter, y, hC, x, d_tf, Q)) != WS_OK) return rc;       // sequence (r, q): Tf_r steps
    // attention on `x` (the block's `inter` tensor)
    float* qkv = a.alloc(size_t(M) * ldq);
    if (!ragged) Qa = a.alloc(size_t(G) * Tf * D), Ka = a.alloc(size_t(G) * Tp * D);
    float* Va = a.alloc(size_t(G) * Tp * Dv);
    if (!ragged) VaT = a.alloc(size_t(G) * Tp * Dv);
    float* hst = a.alloc(size_t(nh) * R * Tf * 2);
    if (!ragged) logits = a.alloc(size_t(G) * Tf * Tp), att = a.alloc(size_t(G) * Tf * Tp), ov = a.alloc(size_t(G) * Tf * Dv);
    WS_PTR(qkv && Qa && Ka && Va && VaT && hst && logits && att && ov);
    if ((rc = dp_gemm(e, x, M, C, b.wqkv, ldq, b.bqkv, nullptr, qkv, ldq)) != WS_OK) return rc;
    const char* norm[3] = {"attn_norm_Q.", "attn_norm_K.", "attn_norm_V."};
    float* outs[3] = {Qa, Ka, Va};
    const int chs[3] = {E, E, cp}, tps[3] = {Tf, Tp, Tp}, offs[3] = {0, nh * E, 2 * nh * E};
    for (int j = 0; j < 3; ++j) {
      ws_heads_args ha = {};
      ha.x = qkv + offs[j], ha.slope = e->dev(p + norm[j] + "act.weight"), ha.gamma = b.gam[j], ha.beta = b.bet[j];
      ha.y = outs[j], ha.stats = hst, ha.ldx = ldq, ha.B = R, ha.T = Tf, ha.Tp = tps[j], ha.Q = Q, ha.nh = nh, ha.ch = chs[j];
      ha.eps = kLnEps;
      WS_RUN(e, ws_heads_fwd(&ha, s));
    }
    // (ragged: the keys t >= Tf_r of row r carry -1e30, so their weights are exact zeros on finite values)
    if ((rc = grid_bmm(e, Qa, Ka, mask, G, Tf, D, Tp, logits, tab_qk)) != WS_OK) return rc;
    WS_RUN(e, ws_softmax_rows_fwd(logits, (long long)G * Tf, Tp, 1.0f / sqrtf(static_cast<float>(D)), att, s));
    if (ragged)
      WS_RUN(e, ws_transpose_batched(Va, G, Tp, Dv, VaT, s));
    else
      for (int g = 0; g < G; ++g)
        WS_RUN(e, ws_transpose(Va + size_t(g) * Tp * Dv, Tp, Dv, Dv, VaT + size_t(g) * Tp * Dv, s));
    if ((rc = grid_bmm(e, att, VaT, nullptr, G, Tf, Tp, Dv, ov, tab_av)) != WS_OK) return rc;
    // head merge: ov [nh][R][Tf][Q][cp] -> [R][Tf][Q][nh*cp]
    float* o = y;                          // y is free again
    if (ragged)
      WS_RUN(e, ws_heads_merge_fwd(ov, nh, R, (long long)Tf * Q, cp, o, s));
    else
      for (int hd = 0; hd < nh; ++hd)
        for (int r = 0; r < R; ++r)
          if ((rc = copy_cols(e, o + (size_t(r) * Tf * Q) * C + hd * cp, C, ov + (size_t(hd) * R + r) * Tf * Dv, cp, cp,
                              (long long)Tf * Q)) != WS_OK)
            return rc;
    // projection + PReLU + LayerNorm over (bins, channels) + residual -> the next block's input
    float* p1 = a.alloc(size_t(M) * C);
    float* p2 = a.alloc(size_t(M) * C);
    float* rst = a.alloc(size_t(R) * Tf * 2);
    float* scr = a.alloc(size_t(M) * C);
    WS_PTR(p1 && p2 && rst && scr);
    if ((rc = dp_gemm(e, o, M, C, e->dev(p + "attn_concat_proj.0.weight"), C, e->dev(p + "attn_concat_proj.0.bias"), nullptr, p1, C)) != WS_OK)
      return rc;
    WS_RUN(e, ws_prelu_fwd(p1, nullptr, e->dev(p + "attn_concat_proj.1.weight"), M * C / 4, 4, static_cast<int>(M * C / 4), p2, s));
    if ((rc = tas_row_stats(e, p2, (long long)R * Tf, Q * C, rst)) != WS_OK) return rc;
    WS_RUN(e, ws_dwconv_fwd(p2, rst, b.proj_g, b.proj_b, n.ones_qc, n.zeros_qc, R * Tf, 1, Q * C, 1, 1, 1, p1, s));
    WS_RUN(e, ws_bn_prelu_fwd(p1, n.id_st, n.ones_c, n.zeros_c, x, n.slope1, M, C, scr, h, s));    // h = LN(..) + inter
    a.release(mk);
  }
  // ---- ConvTranspose2d(C -> 2) and the inverse STFT ----
  float* est4 = a.alloc(size_t(M) * 4);
  WS_PTR(est4);
  // (ragged: the transposed 3x3 convolution at frame Tf_r - 1 reads zeros at frame Tf_r, as its padding on the row alone)
  if (ragged) WS_RUN(e, ws_tail_select_len(h, R, Tf, Q * C, d_tf, h, s));
  if ((rc = dp_conv_view(e, h, R, Tf, Q, C, 1, Q, 1, n.w_out, 4, n.b_out, est4, 4)) != WS_OK) return rc;
  if (!ragged) return dft_istft(e, est4, n.syn4, R, Tf, nf, hop, T, est);
  // dft_istft's synthesis GEMM, then one launch for overlap-add over t < Tf_r, 1 / envelope over those frames, centre trim
  // and the zeros from lengths[r] on
  float* fr = a.alloc(size_t(R) * Tf * nf);
  WS_PTR(fr);
  ws_gemm_nt_args g = {};
  g.A = est4, g.W = n.syn4, g.C = fr;
  g.a_div = kBig, g.a_s2 = ld4, g.c_div = kBig, g.c_s2 = nf, g.st_div1 = 1, g.st_div2 = 1;
  g.M = R * Tf, g.N = nf, g.K = ld4, g.ldw = ld4, g.vec = 3;
  WS_RUN(e, ws_gemm_nt(&g, s));
  WS_RUN(e, ws_ola_norm_len(fr, win, R, Tf, nf, T, d_len, est, s));
  return WS_OK;
}

}  // namespace wsrt
