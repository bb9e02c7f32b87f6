// Speaker stage of the native runtime (libwesep_engine.so): the enrollment front-ends (kaldi fbank, the in-model
// PreEmphasis + MelSpectrogram), the wespeaker encoders (ResNet / Bottleneck ResNet, ECAPA-TDNN, CAM++) in eval mode,
// their pooling layer, and SpeakerTransform.  Load: read_speaker_meta, prep_speaker; forward: speaker_embed,
// spk_transform.
#include "engine_internal.h"

namespace wsrt {

constexpr float kTstpEps = 1e-7f;
constexpr float kAstpFloor = 1e-7f;
// meta spk_pool codes (wesep_amd/bin/export_engine.py SPK_POOL)
constexpr int kPoolTSTP = 0, kPoolMHASTP = 1, kPoolMQMHASTP = 2, kPoolASTP = 3, kPoolTAP = 4, kPoolTSDP = 5;

// ---- load-time preparation -----------------------------------------------------------------------------------
int prep_conv(ws_engine* e, const std::string& conv, const std::string& bn, int cin, int cout, int k, int stride,
              bool relu, ConvPrep* c) {
  if (!require(e, conv + ".weight", {cout, cin, k, k}) || !require(e, bn + ".weight", {cout}) ||
      !require(e, bn + ".bias", {cout}) || !require(e, bn + ".running_mean", {cout}) ||
      !require(e, bn + ".running_var", {cout}))
    return WS_ERR_INVALID;
  c->cin = cin;
  c->cout = cout;
  c->k = k;
  c->stride = stride;
  c->relu = relu;
  const int kk = k * k * cin;
  c->ldp = (kk + 3) / 4 * 4;
  // [cout][cin][ky][kx] -> [cout][(ky*k + kx)*cin + c], zero-padded to ldp columns (functional_resnet.py:29-31)
  const float* w = e->host(conv + ".weight");
  std::vector<float> w2(size_t(cout) * c->ldp, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int ci = 0; ci < cin; ++ci)
      for (int t = 0; t < k * k; ++t) w2[size_t(o) * c->ldp + size_t(t) * cin + ci] = w[(size_t(o) * cin + ci) * k * k + t];
  c->w2 = upload(e, e->persist, w2.data(), w2.size());
  c->st = bn_eval_stats(e, bn, cout);
  c->gamma = e->dev(bn + ".weight");
  c->beta = e->dev(bn + ".bias");
  WS_PTR(c->w2 && c->st);
  return WS_OK;
}

// ---- speaker pooling layer (models/resnet.py run_pool), one stage for the three encoders: a channels-last
// activation [R][F'][T][C] (F' = 1: ECAPA-TDNN, CAM++) -> [R][pool_width], the layer's tensors under `prefix`.
// The ResNet plan pools with TSTP, MHASTP or MQMHASTP; ASTP / TAP / TSDP run on [R*T][C] rows (F' = 1).
int no_pool_plan(ws_engine* e) {
  set_err("engine: speaker pooling %d (%d queries, %d heads, %d layers) has no launch plan", e->spk.pool, e->spk.pool_q,
          e->spk.pool_h, e->spk.pool_layers);
  return WS_ERR_INVALID;
}

// MHASTP / MQMHASTP (models/resnet.py): the pool's tensors, packed per (query, head) as ws_mhastp_fwd reads them --
// W1 with its columns in the kernel order f*(C/H) + c, then b1, W2, b2 (csrc/mhastp.hip, ws_mhastp_pack)
int prep_mhastp(ws_engine* e, const std::string& prefix, int Fp, int C) {
  const int Q = e->spk.pool_q, H = e->spk.pool_h, L = e->spk.pool_layers;
  if (Q < 1 || (e->spk.pool == kPoolMHASTP && Q != 1) || H < 1 || C % H || (L != 1 && L != 2)) return no_pool_plan(e);
  const int Ch = C / H, dm = Ch * Fp, ds = e->spk.pool_ds, n1 = L == 2 ? 64 : ds;
  if (ds != 1 && ds != dm) {
    set_err("engine: MHASTP d_s %d (1 or d_model %d)", ds, dm);
    return WS_ERR_INVALID;
  }
  long long block_floats = 0;
  if (ws_mhastp_sizes(0, 0, 0, 0, L, ds, dm, &block_floats, nullptr) != WS_OK) return WS_ERR_INVALID;
  const size_t P1 = static_cast<size_t>(block_floats);
  std::vector<float> pack(P1 * Q * H);
  for (int q = 0; q < Q; ++q)
    for (int h = 0; h < H; ++h) {
      const std::string b = prefix + (e->spk.pool == kPoolMQMHASTP ? "n_query." + std::to_string(q) + "." : "") +
                            "heads_att_trans." + std::to_string(h) + ".att_";
      if (!require(e, b + "0.weight", {n1, dm, 1}) || !require(e, b + "0.bias", {n1})) return WS_ERR_INVALID;
      if (L == 2 && (!require(e, b + "1.weight", {ds, 64, 1}) || !require(e, b + "1.bias", {ds}))) return WS_ERR_INVALID;
      float* blk = pack.data() + P1 * (size_t(q) * H + h);
      const float* w1 = e->host(b + "0.weight");
      for (int u = 0; u < n1; ++u)
        for (int f = 0; f < Fp; ++f)
          for (int c = 0; c < Ch; ++c) blk[size_t(u) * dm + f * Ch + c] = w1[size_t(u) * dm + c * Fp + f];
      const float* b1 = e->host(b + "0.bias");
      std::copy(b1, b1 + n1, blk + size_t(n1) * dm);
      if (L == 2) {
        const float* w2 = e->host(b + "1.weight");
        const float* b2 = e->host(b + "1.bias");
        float* o2 = blk + size_t(n1) * dm + n1;
        std::copy(w2, w2 + size_t(ds) * 64, o2);
        std::copy(b2, b2 + ds, o2 + size_t(ds) * 64);
      }
    }
  e->spk.pool_pack = upload(e, e->persist, pack.data(), pack.size());
  WS_PTR(e->spk.pool_pack);
  return WS_OK;
}

// the layer's tensors checked, MHASTP's weights packed; `glob`: ASTP with global context (ECAPA_TDNN_GLOB)
int prep_pool(ws_engine* e, const std::string& prefix, int Fp, int C, int glob) {
  const int B = 128, pool = e->spk.pool;
  if (e->spk.kind == 0 && pool != kPoolTSTP && pool != kPoolMHASTP && pool != kPoolMQMHASTP) return no_pool_plan(e);
  switch (pool) {
    case kPoolTSTP:
    case kPoolTAP:
    case kPoolTSDP:
      return WS_OK;
    case kPoolASTP:
      if (!require(e, prefix + "linear1.weight", {B, glob ? 3 * C : C, 1}) || !require(e, prefix + "linear1.bias", {B}) ||
          !require(e, prefix + "linear2.weight", {C, B, 1}) || !require(e, prefix + "linear2.bias", {C}))
        return WS_ERR_INVALID;
      return WS_OK;
    case kPoolMHASTP:
    case kPoolMQMHASTP:
      return prep_mhastp(e, prefix, Fp, C);
    default:
      set_err("engine: speaker pooling %d has no launch plan (0 TSTP, 1 MHASTP, 2 MQMHASTP, 3 ASTP, 4 TAP, 5 TSDP)", pool);
      return WS_ERR_INVALID;
  }
}

// ---- ragged pass: per-row widths -------------------------------------------------------------------
// The device table of a set of per-row widths; speaker_embed uploads every set of the forward before the first launch
const int* len_tab(ws_engine* e, const std::vector<int>& w) {
  for (const auto& t : e->spk_tabs)
    if (t.first == w) return t.second;
  set_err("engine: no device table for a per-row width set of the ragged speaker pass");
  return nullptr;
}

// a row's width after a convolution along time: (W + 2p - k) / s + 1 with the layer's own k, p, s
std::vector<int> conv_widths(const std::vector<int>& w, int k, int s, int p) {
  std::vector<int> o(w.size());
  for (size_t i = 0; i < w.size(); ++i) o[i] = (w[i] + 2 * p - k) / s + 1;
  return o;
}

// which encoders run the batched ragged pass: the ResNets and ECAPA-TDNN with TSTP / TAP / TSDP / ASTP.  CAM++ and the
// attentive multi-head pools keep one enrollment at a time
bool ragged_speaker_covered(const ws_engine* e) {
  if (!e->joint || e->spk.kind > 1) return false;
  const int p = e->spk.pool;
  return p == kPoolTSTP || p == kPoolTAP || p == kPoolTSDP || (e->spk.kind == 1 && p == kPoolASTP);
}

// width of the pooled statistics of [R][F'][T][C]
int pool_width(const ws_engine* e, int Fp, int C) {
  const int P = Fp * C;
  if (e->spk.pool == kPoolTAP || e->spk.pool == kPoolTSDP) return P;
  if (e->spk.pool == kPoolMHASTP || e->spk.pool == kPoolMQMHASTP) return e->spk.pool_q * 2 * P;
  return 2 * P;
}

// the pooling layer's forward: x [R][F'][T][C] -> pooled [R][pool_width].  TSTP: ws_tstp_fwd; TAP / TSDP: one half of the
// TSTP statistics; ASTP: the attention MLP, then ws_astp_fwd; MHASTP / MQMHASTP: the ResNets' single ws_mhastp_fwd
// launch, the 1-D encoders' ws_mhastp_fwd_split (two launches, the grid split over T)
// tl: the rows' valid frames (ragged pass; TSTP / TAP / TSDP / ASTP only) or nullptr
int run_pool(ws_engine* e, const std::string& prefix, const float* x, int R, int Fp, int T, int C, int glob, float* pooled,
             const std::vector<int>* tl = nullptr) {
  const int B = 128;
  const int* tab = nullptr;
  if (tl) {
    if (e->spk.pool == kPoolMHASTP || e->spk.pool == kPoolMQMHASTP) return no_pool_plan(e);
    WS_PTR(tab = len_tab(e, *tl));
  }
  const long long M = (long long)R * T;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  int rc;
  switch (e->spk.pool) {
    case kPoolTSTP:
      if (tab)
        WS_RUN(e, ws_tstp_fwd_len(x, R, Fp, T, C, tab, kTstpEps, pooled, s));
      else
        WS_RUN(e, ws_tstp_fwd(x, R, Fp, T, C, kTstpEps, pooled, s));
      break;
    case kPoolTAP:
    case kPoolTSDP: {         // mean || std, keep one half
      const int P = Fp * C;
      float* st = a.alloc(size_t(R) * 2 * P);
      WS_PTR(st);
      if (tab)
        WS_RUN(e, ws_tstp_fwd_len(x, R, Fp, T, C, tab, kTstpEps, st, s));
      else
        WS_RUN(e, ws_tstp_fwd(x, R, Fp, T, C, kTstpEps, st, s));
      if ((rc = copy_cols(e, pooled, P, st + (e->spk.pool == kPoolTSDP ? P : 0), 2 * P, P, R)) != WS_OK) return rc;
      break;
    }
    case kPoolASTP: {
      // attentive statistics pooling (models/ecapa_tdnn.py ASTP); global context: cat(x, mean, std) W1^T =
      // x Wx^T + (mean Wm^T + std Ws^T + b1), the context a per-utterance bias of the bottleneck
      float* att = a.alloc(size_t(M) * B);
      float* logits = a.alloc(size_t(M) * C);
      float* aux = a.alloc(size_t(R) * 4 * C);
      WS_PTR(att && logits && aux);
      const float* W1 = e->dev(prefix + "linear1.weight");
      const float* rowbias = nullptr;
      if (glob) {
        float* ctx = a.alloc(size_t(R) * 2 * C);
        float* rb = a.alloc(size_t(R) * B);
        WS_PTR(ctx && rb);
        if (tab)
          WS_RUN(e, ws_tstp_fwd_len(x, R, 1, T, C, tab, kTstpEps, ctx, s));
        else
          WS_RUN(e, ws_tstp_fwd(x, R, 1, T, C, kTstpEps, ctx, s));
        if ((rc = linear(e, ctx, R, 2 * C, W1 + C, 3 * C, B, e->dev(prefix + "linear1.bias"), 0, rb)) != WS_OK) return rc;
        if ((rc = linear(e, x, static_cast<int>(M), C, W1, 3 * C, B, nullptr, 0, att)) != WS_OK) return rc;
        rowbias = rb;
      } else {
        if ((rc = linear(e, x, static_cast<int>(M), C, W1, C, B, e->dev(prefix + "linear1.bias"), 0, att)) != WS_OK) return rc;
      }
      WS_RUN(e, ws_rowbias_act_fwd(att, rowbias, M, B, T, 1, att, s));
      if ((rc = linear(e, att, static_cast<int>(M), B, e->dev(prefix + "linear2.weight"), B, C, e->dev(prefix + "linear2.bias"),
                       0, logits)) != WS_OK)
        return rc;
      if (tab)
        WS_RUN(e, ws_astp_fwd_len(x, logits, R, T, C, tab, kAstpFloor, pooled, aux, s));
      else
        WS_RUN(e, ws_astp_fwd(x, logits, R, T, C, kAstpFloor, pooled, aux, s));
      break;
    }
    default: {                // MHASTP / MQMHASTP
      const int Q = e->spk.pool_q, H = e->spk.pool_h, dm = C / H * Fp;
      float* aux = nullptr;
      if (e->spk.kind == 0) {   // one launch, straight from the [R][F'][T][C] activation
        aux = a.alloc(size_t(R) * Q * H * 4 * dm);
        WS_PTR(aux);
        WS_RUN(e, ws_mhastp_fwd(x, e->spk.pool_pack, R, Fp, T, C, Q, H, e->spk.pool_layers, e->spk.pool_ds, pooled, aux, s));
        break;
      }
      int tsplit = 1;
      long long part_floats = 0;
      if (ws_mhastp_split_sizes(R, Fp, T, C, Q, H, e->cu_count > 0 ? e->cu_count : 256, &tsplit, &part_floats) != WS_OK) {
        set_err("engine: %s", ws_last_error());        // host only: no launch
        return WS_ERR_INVALID;
      }
      float* part = a.alloc(static_cast<size_t>(part_floats));
      aux = a.alloc(size_t(R) * Q * H * 4 * dm);
      WS_PTR(part && aux);
      WS_RUN(e, ws_mhastp_fwd_split(x, e->spk.pool_pack, R, Fp, T, C, Q, H, e->spk.pool_layers, e->spk.pool_ds, tsplit, part,
                                    pooled, aux, s));
    }
  }
  a.release(mk);
  return WS_OK;
}

int prep_resnet(ws_engine* e) {
  const int m = 32, ex = e->spk.bottleneck ? 4 : 1;
  const std::string p = "spk_model.";
  int rc = prep_conv(e, p + "conv1", p + "bn1", 1, m, 3, 1, true, &e->spk.stem);
  if (rc != WS_OK) return rc;
  int inp = m;
  for (int li = 0; li < 4; ++li) {
    const int planes = m << li, first_stride = li == 0 ? 1 : 2;
    for (int bi = 0; bi < e->spk.blocks[li]; ++bi) {
      const std::string q = p + "layer" + std::to_string(li + 1) + "." + std::to_string(bi) + ".";
      const int stride = bi == 0 ? first_stride : 1;
      BlockPrep b;
      b.has_sc = stride != 1 || inp != ex * planes;
      if (e->spk.bottleneck) {
        if ((rc = prep_conv(e, q + "conv1", q + "bn1", inp, planes, 1, 1, true, &b.c1)) != WS_OK) return rc;
        if ((rc = prep_conv(e, q + "conv2", q + "bn2", planes, planes, 3, stride, true, &b.c2)) != WS_OK) return rc;
        if ((rc = prep_conv(e, q + "conv3", q + "bn3", planes, ex * planes, 1, 1, true, &b.c3)) != WS_OK) return rc;
      } else {
        if ((rc = prep_conv(e, q + "conv1", q + "bn1", inp, planes, 3, stride, true, &b.c1)) != WS_OK) return rc;
        if ((rc = prep_conv(e, q + "conv2", q + "bn2", planes, planes, 3, 1, true, &b.c2)) != WS_OK) return rc;
      }
      if (b.has_sc &&
          (rc = prep_conv(e, q + "shortcut.0", q + "shortcut.1", inp, ex * planes, 1, stride, false, &b.sc)) != WS_OK)
        return rc;
      e->spk.res_blocks.push_back(b);
      inp = ex * planes;
    }
  }
  if ((rc = prep_pool(e, p + "pool.", e->spk.feat_dim / 8, 8 * m * ex, 0)) != WS_OK) return rc;
  const int pooled = pool_width(e, e->spk.feat_dim / 8, 8 * m * ex);
  if (!require(e, p + "seg_1.weight", {e->E, pooled}) || !require(e, p + "seg_1.bias", {e->E})) return WS_ERR_INVALID;
  const float s0 = 0.f, s1 = 1.f;
  e->slope0 = upload(e, e->persist, &s0, 1);
  e->slope1 = upload(e, e->persist, &s1, 1);
  WS_PTR(e->slope0 && e->slope1);
  if (e->spk.two_emb) {        // embed_b = seg_2(BatchNorm1d(affine = False)(relu(seg_1(stats)))): the separator takes it
    if (!require(e, p + "seg_bn_1.running_mean", {e->E}) || !require(e, p + "seg_bn_1.running_var", {e->E}) ||
        !require(e, p + "seg_2.weight", {e->E, e->E}) || !require(e, p + "seg_2.bias", {e->E}))
      return WS_ERR_INVALID;
    e->spk.seg_bn_st = bn_eval_stats(e, p + "seg_bn_1", e->E);
    std::vector<float> one(e->E, 1.f), zero(e->E, 0.f);
    e->id_one = upload(e, e->persist, one.data(), one.size());
    e->id_zero = upload(e, e->persist, zero.data(), zero.size());
    WS_PTR(e->spk.seg_bn_st && e->id_one && e->id_zero);
  }
  return WS_OK;
}

// Conv1d [cout][cin][k] ('same' padding) as the k x k view of the one-row image: zero outside the middle kernel row
const float* view_weight(ws_engine* e, const std::string& conv, int cout, int cin, int k) {
  const float* w = e->host(conv + ".weight");
  std::vector<float> w2(size_t(cout) * k * k * cin, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int ci = 0; ci < cin; ++ci)
      for (int kx = 0; kx < k; ++kx) w2[(size_t(o) * k * k + size_t(k / 2) * k + kx) * cin + ci] = w[(size_t(o) * cin + ci) * k + kx];
  return upload(e, e->persist, w2.data(), w2.size());
}

// Conv1d [cout][cin][k] (dilation dil, 'same' padding) + BatchNorm1d of one Conv1dReluBn.  k > 1: the convolution runs
// as the k x k implicit-patch view of the one-row image [R][1][T][cin] (include/wesep_hip.h, ws_conv_view), whose
// weight is zero outside the middle kernel row (functional_ecapa.py:34-38).
int prep_tdnn(ws_engine* e, const std::string& conv, const std::string& bn, int cin, int cout, int k, int dil, TdnnPrep* t) {
  if (!require(e, conv + ".weight", {cout, cin, k}) || !require(e, conv + ".bias", {cout}) ||
      !require(e, bn + ".weight", {cout}) || !require(e, bn + ".bias", {cout}) ||
      !require(e, bn + ".running_mean", {cout}) || !require(e, bn + ".running_var", {cout}))
    return WS_ERR_INVALID;
  if (cin % 4 || cout % 4) {
    set_err("engine: ECAPA-TDNN channel counts must be multiples of 4 (%s: %d -> %d)", conv.c_str(), cin, cout);
    return WS_ERR_INVALID;
  }
  t->cin = cin, t->cout = cout, t->k = k, t->dil = dil;
  t->bias = e->dev(conv + ".bias");
  t->gamma = e->dev(bn + ".weight");
  t->beta = e->dev(bn + ".bias");
  t->w = k == 1 ? e->dev(conv + ".weight") : view_weight(e, conv, cout, cin, k);
  t->st = bn_eval_stats(e, bn, cout);
  WS_PTR(t->w && t->st);
  return WS_OK;
}

// wespeaker ECAPA_TDNN(_GLOB)_c512 / _c1024 (models/ecapa_tdnn.py): shapes checked against the container, conv-view
// weights and BatchNorm(eval) statistics prepared once
int prep_ecapa(ws_engine* e) {
  const std::string p = "spk_model.";
  const int C = e->spk.channels, F = e->spk.feat_dim, scale = 8, width = C / scale, P = 1536, B = 128;
  if (C % (4 * scale)) {
    set_err("engine: ECAPA-TDNN channels %d: a multiple of 32 is required", C);
    return WS_ERR_INVALID;
  }
  int rc = prep_tdnn(e, p + "layer1.conv", p + "layer1.bn", F, C, 5, 1, &e->spk.tdnn1);
  if (rc != WS_OK) return rc;
  for (int li = 0; li < 3; ++li) {
    const std::string q = p + "layer" + std::to_string(li + 2) + ".se_res2block.";
    SeRes2Prep b;
    if ((rc = prep_tdnn(e, q + "0.conv", q + "0.bn", C, C, 1, 1, &b.in)) != WS_OK) return rc;
    for (int i = 0; i < scale - 1; ++i) {
      TdnnPrep t;
      if ((rc = prep_tdnn(e, q + "1.convs." + std::to_string(i), q + "1.bns." + std::to_string(i), width, width, 3, li + 2,
                          &t)) != WS_OK)
        return rc;
      b.branch.push_back(t);
    }
    if ((rc = prep_tdnn(e, q + "2.conv", q + "2.bn", C, C, 1, 1, &b.out)) != WS_OK) return rc;
    b.se = q + "3.";
    if (!require(e, b.se + "linear1.weight", {B, C}) || !require(e, b.se + "linear1.bias", {B}) ||
        !require(e, b.se + "linear2.weight", {C, B}) || !require(e, b.se + "linear2.bias", {C}))
      return WS_ERR_INVALID;
    e->spk.se_blocks.push_back(b);
  }
  if ((rc = prep_pool(e, p + "pool.", 1, P, e->spk.glob)) != WS_OK) return rc;
  const int D = pool_width(e, 1, P);
  if (!require(e, p + "conv.weight", {P, 3 * C, 1}) || !require(e, p + "conv.bias", {P}) ||
      !require(e, p + "bn.weight", {D}) || !require(e, p + "bn.bias", {D}) ||
      !require(e, p + "bn.running_mean", {D}) || !require(e, p + "bn.running_var", {D}) ||
      !require(e, p + "linear.weight", {e->E, D}) || !require(e, p + "linear.bias", {e->E}))
    return WS_ERR_INVALID;
  e->spk.pool_bn_st = bn_eval_stats(e, p + "bn", D);
  WS_PTR(e->spk.pool_bn_st);
  if (e->spk.emb_bn) {
    if (!require(e, p + "bn2.weight", {e->E}) || !require(e, p + "bn2.bias", {e->E}) ||
        !require(e, p + "bn2.running_mean", {e->E}) || !require(e, p + "bn2.running_var", {e->E}))
      return WS_ERR_INVALID;
    e->spk.emb_bn_st = bn_eval_stats(e, p + "bn2", e->E);
    WS_PTR(e->spk.emb_bn_st);
  }
  // identity BatchNorm operands (mean 0, rstd 1, gamma 1, beta 0): ws_bn_prelu_fwd then computes y = x + res
  std::vector<float> st(2 * size_t(C), 0.f), one(C, 1.f), zero(C, 0.f);
  for (int c = 0; c < C; ++c) st[C + c] = 1.f;
  e->id_one = upload(e, e->persist, one.data(), one.size());
  e->id_zero = upload(e, e->persist, zero.data(), zero.size());
  const float s0 = 0.f, s1 = 1.f;
  e->slope0 = upload(e, e->persist, &s0, 1);
  e->slope1 = upload(e, e->persist, &s1, 1);
  WS_PTR(e->id_one && e->id_zero && e->slope0 && e->slope1);
  // (0 x C | 1 x C): the [2][c] statistics of any width c <= C start at id_st + C - c
  e->id_st = upload(e, e->persist, st.data(), st.size());
  WS_PTR(e->id_st);
  return WS_OK;
}

// wespeaker CAMPPlus (models/campplus.py, the recipe's alternative speaker encoder: bsrnn.yaml:66-74): FCM head (2-D
// convolutions that stride the mel axis only), D-TDNN backbone of three CAM-dense-TDNN blocks (12 / 24 / 16 layers, growth 32,
// bottleneck 128, kernel 3, dilations 1 / 2 / 2) with transit layers, BN-ReLU, TSTP, dense embedding layer (BatchNorm without
// affine).  Shapes checked against the container; view weights and BatchNorm(eval) statistics prepared once.
int cam_bn_prep(ws_engine* e, const std::string& bn, int c, bool affine, CamBn* b) {
  if (!require(e, bn + ".running_mean", {c}) || !require(e, bn + ".running_var", {c}) ||
      (affine && (!require(e, bn + ".weight", {c}) || !require(e, bn + ".bias", {c}))))
    return WS_ERR_INVALID;
  b->c = c;
  b->st = bn_eval_stats(e, bn, c);
  WS_PTR(b->st);
  b->gamma = affine ? e->dev(bn + ".weight") : e->spk.cam_one;
  b->beta = affine ? e->dev(bn + ".bias") : e->spk.cam_zero;
  return WS_OK;
}

int prep_campplus(ws_engine* e) {
  const std::string p = "spk_model.";
  const int F = e->spk.feat_dim, mc = 32;
  if (F % 8 || e->E % 4) {
    set_err("engine: CAM++ needs feat_dim %% 8 == 0 and an embedding size %% 4 == 0 (got %d, %d)", F, e->E);
    return WS_ERR_INVALID;
  }
  int rc;
  {   // ones / zeros / identity statistics for widths up to 1024 (affine-free BatchNorm, residual-free adds)
    const int C = 1024;
    std::vector<float> one(C, 1.f), zero(C, 0.f), st(2 * size_t(C), 0.f);
    for (int c = 0; c < C; ++c) st[C + c] = 1.f;
    e->spk.cam_one = upload(e, e->persist, one.data(), one.size());
    e->spk.cam_zero = upload(e, e->persist, zero.data(), zero.size());
    e->spk.cam_id_st = upload(e, e->persist, st.data(), st.size());
    const float s0 = 0.f, s1 = 1.f;
    e->slope0 = upload(e, e->persist, &s0, 1);
    e->slope1 = upload(e, e->persist, &s1, 1);
    WS_PTR(e->spk.cam_one && e->spk.cam_zero && e->spk.cam_id_st && e->slope0 && e->slope1);
  }
  // ---- FCM head ----
  auto add = [&](const std::string& conv, const std::string& bn, int cin, int k, int sh, bool relu, int kind) -> int {
    ConvPrep c;
    const int r = prep_conv(e, p + conv, p + bn, cin, mc, k, sh, relu, &c);
    if (r != WS_OK) return r;
    c.sw = 1;
    e->spk.cam_fcm.push_back(c);
    e->spk.cam_fcm_kind.push_back(kind);
    return WS_OK;
  };
  if ((rc = add("head.conv1", "head.bn1", 1, 3, 1, true, 0)) != WS_OK) return rc;
  for (int L = 1; L <= 2; ++L)
    for (int b = 0; b < 2; ++b) {
      const std::string q = "head.layer" + std::to_string(L) + "." + std::to_string(b) + ".";
      const int sh = b == 0 ? 2 : 1;
      if ((rc = add(q + "conv1", q + "bn1", mc, 3, sh, true, 1)) != WS_OK) return rc;
      if (b == 0 && (rc = add(q + "shortcut.0", q + "shortcut.1", mc, 1, sh, false, 2)) != WS_OK) return rc;
      if ((rc = add(q + "conv2", q + "bn2", mc, 3, 1, true, 3)) != WS_OK) return rc;
    }
  if ((rc = add("head.conv2", "head.bn2", mc, 3, 2, true, 0)) != WS_OK) return rc;
  // ---- D-TDNN backbone ----
  const int cin0 = mc * (F / 8), init = e->spk.cam_init, growth = e->spk.cam_growth, bnc = e->spk.cam_bn;
  const std::string x = p + "xvector.";
  if (!require(e, x + "tdnn.linear.weight", {init, cin0, 5})) return WS_ERR_INVALID;
  e->spk.cam_tdnn_w = view_weight(e, x + "tdnn.linear", init, cin0, 5);
  WS_PTR(e->spk.cam_tdnn_w);
  if ((rc = cam_bn_prep(e, x + "tdnn.nonlinear.batchnorm", init, true, &e->spk.cam_tdnn_bn)) != WS_OK) return rc;
  const int nlayers[3] = {12, 24, 16}, dils[3] = {1, 2, 2};
  int ch = init;
  for (int bi = 0; bi < 3; ++bi) {
    std::vector<CamLayer> layers;
    for (int i = 0; i < nlayers[bi]; ++i) {
      const std::string q = x + "block" + std::to_string(bi + 1) + ".tdnnd" + std::to_string(i + 1) + ".";
      CamLayer l;
      l.cin = ch + i * growth, l.dil = dils[bi];
      if ((rc = cam_bn_prep(e, q + "nonlinear1.batchnorm", l.cin, true, &l.bn1)) != WS_OK) return rc;
      if (!require(e, q + "linear1.weight", {bnc, l.cin, 1})) return WS_ERR_INVALID;
      l.w1 = e->dev(q + "linear1.weight");
      if ((rc = cam_bn_prep(e, q + "nonlinear2.batchnorm", bnc, true, &l.bn2)) != WS_OK) return rc;
      if (!require(e, q + "cam_layer.linear_local.weight", {growth, bnc, 3}) ||
          !require(e, q + "cam_layer.linear1.weight", {bnc / 2, bnc, 1}) || !require(e, q + "cam_layer.linear1.bias", {bnc / 2}) ||
          !require(e, q + "cam_layer.linear2.weight", {growth, bnc / 2, 1}) || !require(e, q + "cam_layer.linear2.bias", {growth}))
        return WS_ERR_INVALID;
      l.wloc = view_weight(e, q + "cam_layer.linear_local", growth, bnc, 3);
      WS_PTR(l.wloc);
      l.l1w = e->dev(q + "cam_layer.linear1.weight"), l.l1b = e->dev(q + "cam_layer.linear1.bias");
      l.l2w = e->dev(q + "cam_layer.linear2.weight"), l.l2b = e->dev(q + "cam_layer.linear2.bias");
      layers.push_back(l);
    }
    e->spk.cam_blocks.push_back(layers);
    ch += nlayers[bi] * growth;
    CamTransit t;
    t.cin = ch, t.cout = ch / 2;
    const std::string q = x + "transit" + std::to_string(bi + 1) + ".";
    if ((rc = cam_bn_prep(e, q + "nonlinear.batchnorm", ch, true, &t.bn)) != WS_OK) return rc;
    if (!require(e, q + "linear.weight", {t.cout, ch, 1})) return WS_ERR_INVALID;
    t.w = e->dev(q + "linear.weight");
    e->spk.cam_transit.push_back(t);
    ch /= 2;
  }
  if (ch > 512) {
    set_err("engine: CAM++ backbone width %d exceeds the plan's buffers", ch);
    return WS_ERR_INVALID;
  }
  if ((rc = cam_bn_prep(e, x + "out_nonlinear.batchnorm", ch, true, &e->spk.cam_out_bn)) != WS_OK) return rc;
  if ((rc = prep_pool(e, p + "pool.", 1, ch, 0)) != WS_OK) return rc;
  if (!require(e, x + "dense.linear.weight", {e->E, pool_width(e, 1, ch), 1})) return WS_ERR_INVALID;
  if ((rc = cam_bn_prep(e, x + "dense.nonlinear.batchnorm", e->E, false, &e->spk.cam_dense_bn)) != WS_OK) return rc;
  return WS_OK;
}

// kaldi fbank as two GEMMs: every per-frame step before the power spectrum (2^15 scaling, DC removal, 0.97
// pre-emphasis with the first sample replicated, symmetric Hamming window, zero padding, real DFT) folded into one
// [2 * padded/2][win] basis; triangular mel bank [feat_dim][padded/2]   (wesep_amd/utils/funcs.py, DESIGN 11a;
// reference: runtime/frontend/fbank.h:31-222, wesep/utils/funcs.py:91-116)
int prep_fbank(ws_engine* e) {
  const int win = e->sr / 40, shift = e->sr / 100;
  int padded = 1;
  while (padded < win) padded <<= 1;
  const int nf = padded / 2, nb = e->spk.feat_dim;
  e->spk.fb_win = win;
  e->spk.fb_shift = shift;
  e->spk.fb_padded = padded;
  // B = (DFT * window) P D  with P = pre-emphasis, D = I - 11^T/win, applied column by column in double
  std::vector<double> bw_(size_t(2) * nf * win);
  for (int k = 0; k < nf; ++k)
    for (int n = 0; n < win; ++n) {
      const double w = 0.54 - 0.46 * cos(2.0 * M_PI * n / (win - 1));
      const double ang = 2.0 * M_PI * double(k) * n / padded;
      bw_[(size_t(2) * k) * win + n] = cos(ang) * w;
      bw_[(size_t(2) * k + 1) * win + n] = -sin(ang) * w;
    }
  std::vector<float> basis(size_t(2) * nf * win);
  std::vector<double> row(win);
  for (int r = 0; r < 2 * nf; ++r) {
    const double* b = &bw_[size_t(r) * win];
    // (b P)[j] = b[j] - 0.97 b[j+1]  (+ for j = 0: - 0.97 b[0], the replicated first sample)
    for (int j = 0; j < win; ++j) row[j] = b[j] - (j + 1 < win ? 0.97 * b[j + 1] : 0.0);
    row[0] -= 0.97 * b[0];
    double mean = 0.0;
    for (int j = 0; j < win; ++j) mean += row[j];
    mean /= win;
    for (int j = 0; j < win; ++j) basis[size_t(r) * win + j] = static_cast<float>((row[j] - mean) * 32768.0);
  }
  auto mel = [](double f) { return 1127.0 * log(1.0 + f / 700.0); };
  const double lo = mel(20.0), hi = mel(0.5 * e->sr), delta = (hi - lo) / (nb + 1);
  std::vector<float> bank(size_t(nb) * nf, 0.f);
  for (int b = 0; b < nb; ++b) {
    const double left = lo + b * delta, center = left + delta, right = center + delta;
    for (int i = 0; i < nf; ++i) {
      const double m = mel(double(e->sr) / padded * i);
      const double up = (m - left) / (center - left), down = (right - m) / (right - center);
      const double v = up < down ? up : down;
      bank[size_t(b) * nf + i] = v > 0.0 ? static_cast<float>(v) : 0.f;
    }
  }
  std::vector<float> floor_row(nb, -kGnEps);
  e->spk.fb_basis = upload(e, e->persist, basis.data(), basis.size());
  e->spk.fb_bank = upload(e, e->persist, bank.data(), bank.size());
  e->spk.fb_floor = upload(e, e->persist, floor_row.data(), floor_row.size());
  WS_PTR(e->spk.fb_basis && e->spk.fb_bank && e->spk.fb_floor);
  return WS_OK;
}

// PreEmphasis (speaker.py:10-23) + torchaudio MelSpectrogram(n_fft = win_length = 512, hop 128, hamming window buffer,
// HTK filterbank buffer) of spk_feat = False models, as in modules/common/frontend.py: windowed DFT basis
// [2 * 257 (padded to 516)][512] and fb^T [n_mels][257 (padded to 260)] built from the model's own buffers
int prep_mel_frontend(ws_engine* e) {
  const int n = 512, nf = n / 2 + 1, nm = e->spk.feat_dim;
  if (!require(e, "spk_encoder.spectrogram.window", {n}) || !require(e, "spk_encoder.mel_scale.fb", {nf, nm}) ||
      !require(e, "preEmphasis.flipped_filter", {2}))
    return WS_ERR_INVALID;
  const float* win = e->host("spk_encoder.spectrogram.window");
  const float* fb = e->host("spk_encoder.mel_scale.fb");
  e->spk.mel_coef = -e->host("preEmphasis.flipped_filter")[0];
  e->spk.mel_lds = (2 * nf + 3) / 4 * 4;
  e->spk.mel_ldp = (nf + 3) / 4 * 4;
  std::vector<float> basis(size_t(e->spk.mel_lds) * n, 0.f), fbt(size_t(nm) * e->spk.mel_ldp, 0.f);
  for (int k = 0; k < nf; ++k)
    for (int j = 0; j < n; ++j) {
      const double ang = 2.0 * M_PI * double(k) * j / n;
      basis[(size_t(2) * k) * n + j] = static_cast<float>(cos(ang) * win[j]);
      basis[(size_t(2) * k + 1) * n + j] = static_cast<float>(-sin(ang) * win[j]);
    }
  for (int m = 0; m < nm; ++m)
    for (int k = 0; k < nf; ++k) fbt[size_t(m) * e->spk.mel_ldp + k] = fb[size_t(k) * nm + m];
  e->spk.mel_basis = upload(e, e->persist, basis.data(), basis.size());
  e->spk.mel_fbt = upload(e, e->persist, fbt.data(), fbt.size());
  WS_PTR(e->spk.mel_basis && e->spk.mel_fbt);
  return WS_OK;
}

// the speaker-stage part of the container's meta block (pBSRNN, DPCCN and TF-GridNet plans)
int read_speaker_meta(ws_engine* e) {
  e->spk.feat = static_cast<int>(meta_or(e, "spk_feat", 1));
  e->E = static_cast<int>(meta_or(e, "spk_emb_dim", 256));
  e->use_xform = static_cast<int>(meta_or(e, "use_spk_transform", 0));
  e->joint = static_cast<int>(meta_or(e, "joint_training", 0));
  e->spk.feat_dim = static_cast<int>(meta_or(e, "feat_dim", 80));
  for (int i = 0; i < 4; ++i) e->spk.blocks[i] = static_cast<int>(meta_or(e, ("spk_blocks" + std::to_string(i)).c_str(), 0));
  e->spk.kind = static_cast<int>(meta_or(e, "spk_kind", 0));          // 0 wespeaker ResNet, 1 ECAPA-TDNN, 2 CAM++
  e->spk.channels = static_cast<int>(meta_or(e, "spk_channels", 512));
  e->spk.glob = static_cast<int>(meta_or(e, "spk_glob", 0));
  e->spk.emb_bn = static_cast<int>(meta_or(e, "spk_emb_bn", 0));
  e->spk.bottleneck = static_cast<int>(meta_or(e, "spk_bottleneck", 0));
  e->spk.two_emb = static_cast<int>(meta_or(e, "spk_two_emb", 0));
  e->spk.pool = static_cast<int>(meta_or(e, "spk_pool", e->spk.kind == 1 ? kPoolASTP : kPoolTSTP));
  e->spk.pool_q = static_cast<int>(meta_or(e, "spk_pool_queries", 1));
  e->spk.pool_h = static_cast<int>(meta_or(e, "spk_pool_heads", 1));
  e->spk.pool_layers = static_cast<int>(meta_or(e, "spk_pool_layers", 2));
  e->spk.pool_ds = static_cast<int>(meta_or(e, "spk_pool_ds", 1));
  if (e->spk.kind < 0 || e->spk.kind > 2) {
    set_err("engine: speaker encoder kind %d is not built (0 ResNet, 1 ECAPA-TDNN, 2 CAM++)", e->spk.kind);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

// conv + BatchNorm(eval) + ReLU/identity (+ residual), channels-last (functional_resnet.py:15-46).  The convolution is
// one GEMM on the implicit patch matrix of x (ws_conv_view, nothing materialised); the 1-channel stem, whose patch
// rows are not float4-addressable, writes its 9-column patch matrix with ws_im2col first.
// win / wout (ragged pass): the rows' valid widths of x, which is zero behind them, and of y, whose tail the masked
// epilogue selects to zero again.
int conv_bn_act(ws_engine* e, const ConvPrep& c, const float* x, const float* res, int R, int H, int W, float* y,
                int* Ho_out, int* Wo_out, const std::vector<int>* win = nullptr, std::vector<int>* wout = nullptr) {
  const int pad = c.k / 2, sw = c.sw ? c.sw : c.stride;
  const int Ho = (H + 2 * pad - c.k) / c.stride + 1, Wo = (W + 2 * pad - c.k) / sw + 1;
  const long long M = (long long)R * Ho * Wo;
  const bool implicit = c.cin % 4 == 0 && (long long)H * W * c.cin < 0x7fffffffLL;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* conv = a.alloc(size_t(M) * c.cout);
  float* u = a.alloc(size_t(M) * c.cout);
  WS_PTR(conv && u);
  ws_gemm_nt_args g = {};
  g.W = c.w2, g.C = conv;
  g.a_div = kBig, g.a_s2 = c.ldp, g.c_div = kBig, g.c_s2 = c.cout, g.st_div1 = 1, g.st_div2 = 1;
  g.M = static_cast<int>(M), g.N = c.cout, g.K = c.ldp, g.ldw = c.ldp, g.vec = 3 | 4;
  if (implicit) {
    g.A = x;
    g.conv.on = 1, g.conv.mode = 0, g.conv.H = H, g.conv.W = W, g.conv.C = c.cin, g.conv.Ho = Ho, g.conv.Wo = Wo;
    g.conv.k = c.k, g.conv.sh = c.stride, g.conv.sw = sw, g.conv.p = pad, g.conv.dil = 1;
  } else {
    if (sw != c.stride) {
      set_err("engine: a convolution with different strides along H and W needs cin %% 4 == 0 (the implicit-patch view)");
      return WS_ERR_INVALID;
    }
    float* patches = a.alloc(size_t(M) * c.ldp);
    WS_PTR(patches);
    if (c.ldp != c.k * c.k * c.cin) {
      const int rc = zero_device(e, patches, size_t(M) * c.ldp * 4);
      if (rc != WS_OK) return rc;
    }
    WS_RUN(e, ws_im2col(x, R, H, W, c.cin, c.k, c.stride, pad, c.ldp, patches, s));
    g.A = patches;
  }
  WS_RUN(e, ws_gemm_nt(&g, s));
  if (win) {
    *wout = conv_widths(*win, c.k, sw, pad);
    const int* tab = len_tab(e, *wout);
    WS_PTR(tab);
    WS_RUN(e, ws_bn_prelu_fwd_len(conv, c.st, c.gamma, c.beta, res, c.relu ? e->slope0 : e->slope1, M, c.cout, Ho * Wo, Wo,
                                  tab, u, y, s));
  } else {
    WS_RUN(e, ws_bn_prelu_fwd(conv, c.st, c.gamma, c.beta, res, c.relu ? e->slope0 : e->slope1, M, c.cout, u, y, s));
  }
  a.release(mk);
  *Ho_out = Ho;
  *Wo_out = Wo;
  return WS_OK;
}

// fbank [R][Te][F] (device) -> embedding [R][E]   (wespeaker ResNet, eval mode; models/resnet.py: BasicBlock and
// Bottleneck stacks, TSTP, one or two embedding layers)
// tl (ragged pass): the rows' valid frames; fbank is zero behind them
int resnet_embed(ws_engine* e, const float* fbank, int R, int Te, float* emb, const std::vector<int>* tl) {
  const int F = e->spk.feat_dim, ex = e->spk.bottleneck ? 4 : 1;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  // [R][Te][F] -> [R][F][Te][1]
  float* x = a.alloc(size_t(R) * F * Te);
  WS_PTR(x);
  for (int r = 0; r < R; ++r)
    WS_RUN(e, ws_transpose(fbank + size_t(r) * Te * F, Te, F, F, x + size_t(r) * F * Te, s));
  int H = F, W = Te, Ho, Wo, rc;
  // rotating activation buffers sized for the largest activation (the first stage's output: 32 * ex channels)
  const size_t act = size_t(R) * H * W * 32 * ex;
  float* bufs[4] = {a.alloc(act), a.alloc(act), a.alloc(act), nullptr};
  bufs[3] = e->spk.bottleneck ? a.alloc(act) : bufs[0];        // BasicBlock stacks rotate through three
  WS_PTR(bufs[0] && bufs[1] && bufs[2] && bufs[3]);
  // per-row widths of the block input (w), of the block's intermediate tensors and of its shortcut
  std::vector<int> w, w1, w2, ws;
  const std::vector<int>* in = tl;
  auto out = [&](std::vector<int>* v) { return tl ? v : nullptr; };
  if ((rc = conv_bn_act(e, e->spk.stem, x, nullptr, R, H, W, bufs[0], &Ho, &Wo, in, out(&w))) != WS_OK) return rc;
  in = out(&w);
  int cur = 0, C = 32;
  for (const BlockPrep& b : e->spk.res_blocks) {
    float* y = bufs[cur];
    float* t1 = bufs[(cur + 1) % 4];
    float* t2 = bufs[(cur + 2) % 4];
    float* t3 = bufs[(cur + 3) % 4];
    int H1, W1, H2, W2, Hs, Ws;
    const float* shortcut = y;
    if (e->spk.bottleneck) {
      if ((rc = conv_bn_act(e, b.c1, y, nullptr, R, H, W, t1, &H1, &W1, in, out(&w1))) != WS_OK) return rc;
      if ((rc = conv_bn_act(e, b.c2, t1, nullptr, R, H1, W1, t2, &H2, &W2, out(&w1), out(&w2))) != WS_OK) return rc;
      if (b.has_sc) {
        if ((rc = conv_bn_act(e, b.sc, y, nullptr, R, H, W, t1, &Hs, &Ws, in, out(&ws))) != WS_OK) return rc;
        shortcut = t1;
      }
      if ((rc = conv_bn_act(e, b.c3, t2, shortcut, R, H2, W2, t3, &H2, &W2, out(&w2), out(&w))) != WS_OK) return rc;
      cur = (cur + 3) % 4;
      C = b.c3.cout;
    } else {                     // three of the buffers: conv2 writes over the block input unless that is the shortcut
      float* o = bufs[(cur + 1) % 3];
      float* sc = bufs[(cur + 2) % 3];
      if ((rc = conv_bn_act(e, b.c1, y, nullptr, R, H, W, o, &H1, &W1, in, out(&w1))) != WS_OK) return rc;
      if (b.has_sc) {
        if ((rc = conv_bn_act(e, b.sc, y, nullptr, R, H, W, sc, &Hs, &Ws, in, out(&ws))) != WS_OK) return rc;
        shortcut = sc;
      }
      float* dst = b.has_sc ? y : sc;
      if ((rc = conv_bn_act(e, b.c2, o, shortcut, R, H1, W1, dst, &H2, &W2, out(&w1), out(&w))) != WS_OK) return rc;
      cur = b.has_sc ? cur : (cur + 2) % 3;
      C = b.c2.cout;
    }
    H = H2, W = W2;
  }
  const std::string p = "spk_model.";
  const int pooled = pool_width(e, H, C);
  float* stats = a.alloc(size_t(R) * pooled);
  WS_PTR(stats);
  if ((rc = run_pool(e, p + "pool.", bufs[cur], R, H, W, C, 0, stats, in)) != WS_OK) return rc;
  if (!e->spk.two_emb) {
    rc = linear(e, stats, R, pooled, e->dev(p + "seg_1.weight"), pooled, e->E, e->dev(p + "seg_1.bias"), 0, emb);
  } else {
    float* t = a.alloc(size_t(R) * e->E);
    float* u = a.alloc(size_t(R) * e->E);
    float* v = a.alloc(size_t(R) * e->E);
    WS_PTR(t && u && v);
    if ((rc = linear(e, stats, R, pooled, e->dev(p + "seg_1.weight"), pooled, e->E, e->dev(p + "seg_1.bias"), 2, t)) != WS_OK)
      return rc;
    WS_RUN(e, ws_bn_prelu_fwd(t, e->spk.seg_bn_st, e->id_one, e->id_zero, nullptr, e->slope1, R, e->E, u, v, s));
    rc = linear(e, v, R, e->E, e->dev(p + "seg_2.weight"), e->E, e->E, e->dev(p + "seg_2.bias"), 0, emb);
  }
  a.release(mk);
  return rc;
}

// y = x + res on [M][c] (c <= spk_channels): the BatchNorm kernel with identity operands
// (T, tab: the ragged pass -- rows of T frames, zeros selected behind tab[r])
int add_rows(ws_engine* e, const float* x, const float* res, long long M, int c, float* scratch, float* y, int T = 0,
             const int* tab = nullptr) {
  if (tab)
    WS_RUN(e, ws_bn_prelu_fwd_len(x, e->id_st + (e->spk.channels - c), e->id_one, e->id_zero, res, e->slope1, M, c, T, T, tab,
                                  scratch, y, e->stream));
  else
    WS_RUN(e, ws_bn_prelu_fwd(x, e->id_st + (e->spk.channels - c), e->id_one, e->id_zero, res, e->slope1, M, c, scratch, y,
                              e->stream));
  return WS_OK;
}

// y [M][cout] = BN(ReLU(conv1d(x [R][T][cin]))), x rows lda apart (k == 1) or dense (k > 1)   (functional_ecapa.py:23-51)
// tab (ragged pass): x is zero behind tab[r] frames of row r, and so is y ('same' padding: the widths never change)
int tdnn(ws_engine* e, const TdnnPrep& t, const float* x, long long lda, int R, int T, float* y, const int* tab = nullptr) {
  const long long M = (long long)R * T;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* c = a.alloc(size_t(M) * t.cout);
  float* u = a.alloc(size_t(M) * t.cout);
  WS_PTR(c && u);
  ws_gemm_nt_args g = {};
  g.A = x, g.W = t.w, g.bias = t.bias, g.C = c;
  g.a_div = kBig, g.a_s2 = lda, g.c_div = kBig, g.c_s2 = t.cout, g.st_div1 = 1, g.st_div2 = 1;
  g.M = static_cast<int>(M), g.N = t.cout, g.act = 2, g.vec = 3 | 4;
  if (t.k == 1) {
    g.K = t.cin, g.ldw = t.cin;
  } else {
    g.K = t.k * t.k * t.cin, g.ldw = g.K;
    g.conv.on = 1, g.conv.mode = 0, g.conv.H = 1, g.conv.W = T, g.conv.C = t.cin, g.conv.Ho = 1, g.conv.Wo = T;
    g.conv.k = t.k, g.conv.sh = 1, g.conv.sw = 1, g.conv.p = t.dil * (t.k / 2), g.conv.dil = t.dil;
  }
  WS_RUN(e, ws_gemm_nt(&g, s));
  if (tab)
    WS_RUN(e, ws_bn_prelu_fwd_len(c, t.st, t.gamma, t.beta, nullptr, e->slope1, M, t.cout, T, T, tab, u, y, s));
  else
    WS_RUN(e, ws_bn_prelu_fwd(c, t.st, t.gamma, t.beta, nullptr, e->slope1, M, t.cout, u, y, s));
  a.release(mk);
  return WS_OK;
}

// SE_Res2Block (models/ecapa_tdnn.py:78-92): x [M][C] dense -> out [M][C] dense
int se_res2_block(ws_engine* e, const SeRes2Prep& b, const float* x, int R, int T, float* out, const int* tab = nullptr) {
  const int C = e->spk.channels, scale = 8, w = C / scale, B = 128;
  const long long M = (long long)R * T;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* h = a.alloc(size_t(M) * C);          // first 1x1 TDNN
  float* r2 = a.alloc(size_t(M) * C);         // the branches' outputs, concatenated
  float* slice = a.alloc(size_t(M) * w);
  float* in = a.alloc(size_t(M) * w);
  float* y = a.alloc(size_t(M) * w);
  float* scratch = a.alloc(size_t(M) * C);
  WS_PTR(h && r2 && slice && in && y && scratch);
  int rc;
  if ((rc = tdnn(e, b.in, x, C, R, T, h, tab)) != WS_OK) return rc;
  for (int i = 0; i < scale - 1; ++i) {       // group i >= 1 adds the previous group's output before its own TDNN
    const float* src = slice;
    if ((rc = copy_cols(e, slice, w, h + size_t(i) * w, C, w, M)) != WS_OK) return rc;
    if (i > 0) {
      if ((rc = add_rows(e, y, slice, M, w, scratch, in, T, tab)) != WS_OK) return rc;
      src = in;
    }
    if ((rc = tdnn(e, b.branch[i], src, w, R, T, y, tab)) != WS_OK) return rc;
    if ((rc = copy_cols(e, r2 + size_t(i) * w, C, y, w, w, M)) != WS_OK) return rc;
  }
  if ((rc = copy_cols(e, r2 + size_t(scale - 1) * w, C, h + size_t(scale - 1) * w, C, w, M)) != WS_OK) return rc;
  if ((rc = tdnn(e, b.out, r2, C, R, T, h, tab)) != WS_OK) return rc;
  // squeeze-excitation: gate [R][C] = sigmoid(W2 relu(W1 mean_t + b1) + b2), broadcast over the frames
  float* mean2 = a.alloc(size_t(R) * 2 * C);
  float* z = a.alloc(size_t(R) * B);
  float* gate = a.alloc(size_t(R) * C);
  WS_PTR(mean2 && z && gate);
  if (tab)                                     // the mean over the row's own frames, dense [R][C]
    WS_RUN(e, ws_time_mean_len(h, R, T, C, tab, mean2, s));
  else if ((rc = time_mean(e, h, R, T, C, mean2)) != WS_OK)
    return rc;
  {
    ws_gemm_nt_args g = {};
    g.A = mean2, g.W = e->dev(b.se + "linear1.weight"), g.bias = e->dev(b.se + "linear1.bias"), g.C = z;
    g.a_div = kBig, g.a_s2 = tab ? C : 2 * C, g.c_div = kBig, g.c_s2 = B, g.st_div1 = 1, g.st_div2 = 1;
    g.M = R, g.N = B, g.K = C, g.ldw = C, g.act = 2, g.vec = 3 | 4;
    WS_RUN(e, ws_gemm_nt(&g, s));
  }
  if ((rc = linear(e, z, R, B, e->dev(b.se + "linear2.weight"), B, C, e->dev(b.se + "linear2.bias"), 0, gate)) != WS_OK)
    return rc;
  WS_RUN(e, ws_rowbias_act_fwd(gate, nullptr, R, C, 1, 3, gate, s));
  WS_RUN(e, ws_bcast_rows(gate, 1.0f, T, M, C, r2, s));
  WS_RUN(e, ws_maskmul_fwd(h, C, r2, M, C, scratch, s));
  float* u = r2;                               // free again: pre-activation scratch of the residual add
  if ((rc = add_rows(e, scratch, x, M, C, u, out, T, tab)) != WS_OK) return rc;   // the gated sum's tail selected to zero
  a.release(mk);
  return WS_OK;
}

// fbank [R][Te][F] (device) -> embedding [R][E]   (wespeaker ECAPA-TDNN, eval mode; models/ecapa_tdnn.py:135-160)
// tl (ragged pass): the rows' valid frames; fbank is zero behind them
int ecapa_embed(ws_engine* e, const float* fbank, int R, int Te, float* emb, const std::vector<int>* tl) {
  const int C = e->spk.channels, P = 1536, T = Te;
  const long long M = (long long)R * T;
  const std::string p = "spk_model.";
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* cur = a.alloc(size_t(M) * C);
  float* nxt = a.alloc(size_t(M) * C);
  float* cat = a.alloc(size_t(M) * 3 * C);
  WS_PTR(cur && nxt && cat);
  int rc;
  const int* tab = nullptr;
  if (tl) WS_PTR(tab = len_tab(e, *tl));
  if ((rc = tdnn(e, e->spk.tdnn1, fbank, e->spk.feat_dim, R, T, cur, tab)) != WS_OK) return rc;
  for (int li = 0; li < 3; ++li) {
    if ((rc = se_res2_block(e, e->spk.se_blocks[li], cur, R, T, nxt, tab)) != WS_OK) return rc;
    if ((rc = copy_cols(e, cat + size_t(li) * C, 3 * C, nxt, C, C, M)) != WS_OK) return rc;
    std::swap(cur, nxt);
  }
  const int D = pool_width(e, 1, P);
  float* h = a.alloc(size_t(M) * P);           // relu(conv1x1(cat)): the pooled sequence
  float* pooled = a.alloc(size_t(R) * D);
  float* normed = a.alloc(size_t(R) * D);
  float* u = a.alloc(size_t(R) * D);
  WS_PTR(h && pooled && normed && u);
  if ((rc = linear(e, cat, static_cast<int>(M), 3 * C, e->dev(p + "conv.weight"), 3 * C, P, e->dev(p + "conv.bias"), 2, h)) != WS_OK)
    return rc;
  if ((rc = run_pool(e, p + "pool.", h, R, 1, T, P, e->spk.glob, pooled, tl)) != WS_OK) return rc;
  WS_RUN(e, ws_bn_prelu_fwd(pooled, e->spk.pool_bn_st, e->dev(p + "bn.weight"), e->dev(p + "bn.bias"), nullptr, e->slope1, R,
                            D, u, normed, s));
  if (e->spk.emb_bn) {
    float* raw = a.alloc(size_t(R) * e->E);
    float* u2 = a.alloc(size_t(R) * e->E);
    WS_PTR(raw && u2);
    if ((rc = linear(e, normed, R, D, e->dev(p + "linear.weight"), D, e->E, e->dev(p + "linear.bias"), 0, raw)) != WS_OK)
      return rc;
    WS_RUN(e, ws_bn_prelu_fwd(raw, e->spk.emb_bn_st, e->dev(p + "bn2.weight"), e->dev(p + "bn2.bias"), nullptr, e->slope1, R, e->E,
                              u2, emb, s));
  } else if ((rc = linear(e, normed, R, D, e->dev(p + "linear.weight"), D, e->E, e->dev(p + "linear.bias"), 0, emb)) !=
             WS_OK) {
    return rc;
  }
  a.release(mk);
  return WS_OK;
}

// ---- CAM++ forward (models/campplus.py, eval mode) ---------------------------------------------------------------------
// y = act(BatchNorm(x)) on dense rows [M][c]
int cam_bn_act(ws_engine* e, const CamBn& b, const float* x, long long M, bool relu, float* scratch, float* y) {
  WS_RUN(e, ws_bn_prelu_fwd(x, b.st, b.gamma, b.beta, nullptr, relu ? e->slope0 : e->slope1, M, b.c, scratch, y, e->stream));
  return WS_OK;
}

// y [M][nout] = x [M][k] (rows lda apart) W^T + bias
int cam_lin(ws_engine* e, const float* x, long long lda, long long M, int k, const float* W, int nout, const float* bias, float* y) {
  ws_gemm_nt_args a = {};
  a.A = x, a.W = W, a.bias = bias, a.C = y;
  a.a_div = kBig, a.a_s2 = lda, a.c_div = kBig, a.c_s2 = nout, a.st_div1 = 1, a.st_div2 = 1;
  a.M = static_cast<int>(M), a.N = nout, a.K = k, a.ldw = k;
  a.vec = vec_bits({(long long)k, lda});
  WS_RUN(e, ws_gemm_nt(&a, e->stream));
  return WS_OK;
}

// y [R*To][cout] = conv1d(x [R][T][cin], k taps, dilation dil, stride sw, 'same' padding), bias-free: the k x k view of the
// one-row image (functional_campplus.Conv1dFn)
int cam_conv(ws_engine* e, const float* x, int R, int T, int cin, const float* Wv, int cout, int k, int dil, int sw, float* y,
             int* To_out) {
  const int p = dil * (k / 2), To = (T + 2 * p - dil * (k - 1) - 1) / sw + 1;
  ws_gemm_nt_args g = {};
  g.A = x, g.W = Wv, g.C = y;
  g.a_div = kBig, g.a_s2 = cin, g.c_div = kBig, g.c_s2 = cout, g.st_div1 = 1, g.st_div2 = 1;
  g.M = R * To, g.N = cout, g.K = k * k * cin, g.ldw = g.K, g.vec = 3 | 4;
  g.conv.on = 1, g.conv.mode = 0, g.conv.H = 1, g.conv.W = T, g.conv.C = cin, g.conv.Ho = 1, g.conv.Wo = To;
  g.conv.k = k, g.conv.sh = 1, g.conv.sw = sw, g.conv.p = p, g.conv.dil = dil;
  WS_RUN(e, ws_gemm_nt(&g, e->stream));
  *To_out = To;
  return WS_OK;
}

// CAMDenseTDNNLayer (campplus.py:120-170): x = the first l.cin columns of `cat` (rows ld apart) -> 32 new channels written
// behind them.  Context-aware mask: m = sigmoid(W2 relu(W1 (segment mean + utterance mean) + b1) + b2) per 100-frame segment
int cam_layer(ws_engine* e, const CamLayer& l, float* cat, long long ld, int R, int T) {
  const int bnc = e->spk.cam_bn, growth = e->spk.cam_growth, hid = bnc / 2, seg = 100, nseg = (T + seg - 1) / seg;
  const long long M = (long long)R * T, Ms = (long long)R * nseg;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* xin = a.alloc(size_t(M) * l.cin);
  float* u = a.alloc(size_t(M) * (l.cin > bnc ? l.cin : bnc));
  float* x1 = a.alloc(size_t(M) * l.cin);
  float* h = a.alloc(size_t(M) * bnc);
  float* x2 = a.alloc(size_t(M) * bnc);
  float* yl = a.alloc(size_t(M) * growth);
  float* sums = a.alloc(size_t(Ms) * bnc);
  float* mseg = a.alloc(size_t(Ms) * bnc);
  float* mean2 = a.alloc(size_t(R) * 2 * bnc);
  float* rb = a.alloc(size_t(R) * hid);
  float* rbf = a.alloc(size_t(Ms) * hid);
  float* g1 = a.alloc(size_t(Ms) * hid);
  float* g1u = a.alloc(size_t(Ms) * hid);
  float* hh = a.alloc(size_t(Ms) * hid);
  float* m = a.alloc(size_t(Ms) * growth);
  WS_PTR(xin && u && x1 && h && x2 && yl && sums && mseg && mean2 && rb && rbf && g1 && g1u && hh && m);
  int rc, To;
  if ((rc = copy_cols(e, xin, l.cin, cat, ld, l.cin, M)) != WS_OK) return rc;
  if ((rc = cam_bn_act(e, l.bn1, xin, M, true, u, x1)) != WS_OK) return rc;
  if ((rc = cam_lin(e, x1, l.cin, M, l.cin, l.w1, bnc, nullptr, h)) != WS_OK) return rc;
  if ((rc = cam_bn_act(e, l.bn2, h, M, true, u, x2)) != WS_OK) return rc;
  if ((rc = cam_conv(e, x2, R, T, bnc, l.wloc, growth, 3, l.dil, 1, yl, &To)) != WS_OK) return rc;
  // context: mean over each segment (the last one may be shorter) + mean over the utterance
  WS_RUN(e, ws_seg_sums(x2, nullptr, R, T, bnc, seg, sums, s));
  WS_RUN(e, ws_bcast_rows(sums, 1.0f / seg, 1, Ms, bnc, mseg, s));
  const int last = T - (nseg - 1) * seg;
  if (last != seg)
    for (int r = 0; r < R; ++r) {
      const size_t o = (size_t(r) * nseg + nseg - 1) * bnc;
      WS_RUN(e, ws_bcast_rows(sums + o, 1.0f / last, 1, 1, bnc, mseg + o, s));
    }
  if ((rc = time_mean(e, x2, R, T, bnc, mean2)) != WS_OK) return rc;
  // W1 (mean_seg + mean_all) + b1 = W1 mean_seg + (W1 mean_all + b1): the utterance part is a per-row bias
  if ((rc = cam_lin(e, mean2, 2 * bnc, R, bnc, l.l1w, hid, l.l1b, rb)) != WS_OK) return rc;
  if ((rc = cam_lin(e, mseg, bnc, Ms, bnc, l.l1w, hid, nullptr, g1)) != WS_OK) return rc;
  WS_RUN(e, ws_bcast_rows(rb, 1.0f, nseg, Ms, hid, rbf, s));
  WS_RUN(e, ws_bn_prelu_fwd(g1, e->spk.cam_id_st + (1024 - hid), e->spk.cam_one, e->spk.cam_zero, rbf, e->slope0, Ms, hid, g1u, hh, s));
  if ((rc = cam_lin(e, hh, hid, Ms, hid, l.l2w, growth, l.l2b, m)) != WS_OK) return rc;
  WS_RUN(e, ws_rowbias_act_fwd(m, nullptr, Ms, growth, 1, 3, m, s));
  WS_RUN(e, ws_seg_scale(yl, m, R, T, growth, seg, yl, s));
  if ((rc = copy_cols(e, cat + l.cin, ld, yl, growth, growth, M)) != WS_OK) return rc;
  a.release(mk);
  return WS_OK;
}

// fbank [R][Te][F] (device) -> embedding [R][E]   (wespeaker CAMPPlus, eval mode; models/campplus.py:225-262)
int campplus_embed(ws_engine* e, const float* fbank, int R, int Te, float* emb, const std::vector<int>* tl) {
  if (tl) {
    set_err("engine: CAM++ has no ragged pass (one enrollment at a time)");
    return WS_ERR_INVALID;
  }
  const int F = e->spk.feat_dim, mc = 32;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  int rc;
  // ---- FCM head on [R][F][Te][1]; the mel axis is strided three times, the frame axis never ----
  float* x = a.alloc(size_t(R) * F * Te);
  WS_PTR(x);
  for (int r = 0; r < R; ++r) WS_RUN(e, ws_transpose(fbank + size_t(r) * Te * F, Te, F, F, x + size_t(r) * F * Te, s));
  const size_t act = size_t(R) * F * Te * mc;
  float* bufs[3] = {a.alloc(act), a.alloc(act), a.alloc(act)};
  WS_PTR(bufs[0] && bufs[1] && bufs[2]);
  int H = F, W = Te, Ho, Wo;
  const float* cur = x;
  int ci = 0;                 // buffer that holds `cur` (-1: x)
  auto other = [&](int a0, int a1) { for (int i = 0; i < 3; ++i) if (i != a0 && i != a1) return i; return 0; };
  size_t k = 0;
  {
    if ((rc = conv_bn_act(e, e->spk.cam_fcm[k++], cur, nullptr, R, H, W, bufs[0], &Ho, &Wo)) != WS_OK) return rc;
    cur = bufs[0], ci = 0;
  }
  while (k < e->spk.cam_fcm.size()) {
    const int kind = e->spk.cam_fcm_kind[k];
    if (kind == 0) {          // the final strided convolution
      const int o = other(ci, ci);
      if ((rc = conv_bn_act(e, e->spk.cam_fcm[k++], cur, nullptr, R, H, W, bufs[o], &Ho, &Wo)) != WS_OK) return rc;
      cur = bufs[o], ci = o, H = Ho, W = Wo;
      continue;
    }
    // BasicResBlock: conv1 [, shortcut], conv2 + residual
    const int o1 = other(ci, ci);
    int H1, W1;
    if ((rc = conv_bn_act(e, e->spk.cam_fcm[k++], cur, nullptr, R, H, W, bufs[o1], &H1, &W1)) != WS_OK) return rc;
    const float* sc = cur;
    int o2 = other(ci, o1);
    if (e->spk.cam_fcm_kind[k] == 2) {
      int Hs, Ws;
      if ((rc = conv_bn_act(e, e->spk.cam_fcm[k++], cur, nullptr, R, H, W, bufs[o2], &Hs, &Ws)) != WS_OK) return rc;
      sc = bufs[o2];
      // conv2 may now overwrite the block input
      if ((rc = conv_bn_act(e, e->spk.cam_fcm[k++], bufs[o1], sc, R, H1, W1, bufs[ci], &Ho, &Wo)) != WS_OK) return rc;
      cur = bufs[ci];
    } else {
      if ((rc = conv_bn_act(e, e->spk.cam_fcm[k++], bufs[o1], sc, R, H1, W1, bufs[o2], &Ho, &Wo)) != WS_OK) return rc;
      cur = bufs[o2], ci = o2;
    }
    H = Ho, W = Wo;
  }
  // [R][H'][T][32] -> [R*T][32 * H'] with channel index c * H' + h (the reference's reshape of [B, C, H', T])
  const int Hp = H, T0 = W, c0 = mc * Hp;
  float* feat = a.alloc(size_t(R) * T0 * c0);
  WS_PTR(feat);
  for (int r = 0; r < R; ++r)
    WS_RUN(e, ws_transpose(cur + size_t(r) * Hp * T0 * mc, Hp, T0 * mc, T0 * mc, feat + size_t(r) * T0 * c0, s));
  // ---- D-TDNN backbone ----
  int T;
  const int init = e->spk.cam_init, growth = e->spk.cam_growth;
  const int Tmax = (T0 - 1) / 2 + 1;
  float* t0 = a.alloc(size_t(R) * Tmax * init);
  float* scratch = a.alloc(size_t(R) * Tmax * 1024);
  WS_PTR(t0 && scratch);
  if ((rc = cam_conv(e, feat, R, T0, c0, e->spk.cam_tdnn_w, init, 5, 1, 2, t0, &T)) != WS_OK) return rc;
  const long long M = (long long)R * T;
  int ch = init;
  float* y = a.alloc(size_t(M) * init);
  WS_PTR(y);
  if ((rc = cam_bn_act(e, e->spk.cam_tdnn_bn, t0, M, true, scratch, y)) != WS_OK) return rc;
  for (size_t bi = 0; bi < e->spk.cam_blocks.size(); ++bi) {
    const std::vector<CamLayer>& layers = e->spk.cam_blocks[bi];
    const long long ld = ch + (long long)layers.size() * growth;
    float* cat = a.alloc(size_t(M) * ld);
    float* tin = a.alloc(size_t(M) * ld);
    float* tout = a.alloc(size_t(M) * (ld / 2));
    WS_PTR(cat && tin && tout);
    if ((rc = copy_cols(e, cat, ld, y, ch, ch, M)) != WS_OK) return rc;
    for (const CamLayer& l : layers)
      if ((rc = cam_layer(e, l, cat, ld, R, T)) != WS_OK) return rc;
    const CamTransit& t = e->spk.cam_transit[bi];
    if ((rc = cam_bn_act(e, t.bn, cat, M, true, scratch, tin)) != WS_OK) return rc;
    if ((rc = cam_lin(e, tin, ld, M, static_cast<int>(ld), t.w, t.cout, nullptr, tout)) != WS_OK) return rc;
    y = tout, ch = t.cout;
  }
  const int D = pool_width(e, 1, ch);
  float* yo = a.alloc(size_t(M) * ch);
  float* stats = a.alloc(size_t(R) * D);
  float* raw = a.alloc(size_t(R) * e->E);
  float* u2 = a.alloc(size_t(R) * e->E);
  WS_PTR(yo && stats && raw && u2);
  if ((rc = cam_bn_act(e, e->spk.cam_out_bn, y, M, true, scratch, yo)) != WS_OK) return rc;
  if ((rc = run_pool(e, "spk_model.pool.", yo, R, 1, T, ch, 0, stats)) != WS_OK) return rc;
  if ((rc = cam_lin(e, stats, D, R, D, e->dev("spk_model.xvector.dense.linear.weight"), e->E, nullptr, raw)) != WS_OK)
    return rc;
  if ((rc = cam_bn_act(e, e->spk.cam_dense_bn, raw, R, false, u2, emb)) != WS_OK) return rc;
  a.release(mk);
  return WS_OK;
}

// per-row CMN over the frames: feats [R][Te][nb] -= mean_t          (shared by both front-ends)
int subtract_time_mean(ws_engine* e, float* feats, int R, int Te, int nb) {
  const long long M = (long long)R * Te;
  void* s = e->stream;
  Arena& a = e->work;
  int nsplit = Te / 32;
  const int cap = 1024 / R > 1 ? 1024 / R : 1;
  if (nsplit > cap) nsplit = cap;
  if (nsplit < 1) nsplit = 1;
  float* slab = a.alloc(size_t(nsplit) * R * 2 * nb);
  float* sums = a.alloc(size_t(R) * 2 * nb);
  float* neg_mean = a.alloc(size_t(R) * nb);
  WS_PTR(slab && sums && neg_mean);
  WS_RUN(e, ws_chan_sums(feats, nullptr, nullptr, 1, Te, R, nsplit, nb, slab, s));
  WS_RUN(e, ws_reduce_slabs(slab, nsplit, (long long)R * 2 * nb, (long long)R * 2 * nb, sums, 0, 0, s));
  // rows of `sums` are [2][nb] per utterance: scale the first half of each by -1/Te into a dense [R][nb]
  for (int r = 0; r < R; ++r)
    WS_RUN(e, ws_affine_fwd(sums + size_t(r) * 2 * nb, nullptr, nullptr, -1.0f / Te, 1, 1, nb, neg_mean + size_t(r) * nb, s));
  WS_RUN(e, ws_affine_fwd(feats, nullptr, neg_mean, 1.0f, M, Te, nb, feats, s));
  return WS_OK;
}

// waveform [R][Tw] in [-1, 1] (device) -> mean-normalised kaldi fbank [R][Te][F]  (utils/funcs.py compute_fbank +
// apply_cmvn with dither 0; reference: SeparateEngine::ExtractFeature, separate_engine.cc:53-74)
// te_tab (ragged pass, device int[R]): the rows' own frame counts.  With snip-edges framing frame f < te_tab[r] reads only
// samples below the row's length, so the GEMMs run over the rectangle; CMN over the row's frames, the tail zeroed
int kaldi_fbank(ws_engine* e, const float* wav, int R, int Tw, float* feats, int Te, const int* te_tab = nullptr) {
  const int win = e->spk.fb_win, shift = e->spk.fb_shift, nf = e->spk.fb_padded / 2, nb = e->spk.feat_dim;
  const long long M = (long long)R * Te;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* spec = a.alloc(size_t(M) * 2 * nf);
  float* power = a.alloc(size_t(M) * nf);
  float* mel = a.alloc(size_t(M) * nb);
  WS_PTR(spec && power && mel);
  ws_gemm_nt_args g = {};
  g.A = wav, g.W = e->spk.fb_basis, g.C = spec;
  g.a_div = Te, g.a_s1 = Tw, g.a_s2 = shift;            // frame f of row r starts at r*Tw + f*shift: overlapping view
  g.c_div = kBig, g.c_s2 = 2 * nf, g.st_div1 = 1, g.st_div2 = 1;
  g.M = static_cast<int>(M), g.N = 2 * nf, g.K = win, g.ldw = win;
  g.vec = (Tw % 4 == 0 && shift % 4 == 0 && win % 4 == 0) ? 3 : (win % 4 == 0 ? 2 : 0);     // exact-fp32 products
  WS_RUN(e, ws_gemm_nt(&g, s));
  WS_RUN(e, ws_power_spec(spec, M, nf, 2 * nf, nf, power, s));
  ws_gemm_nt_args h = {};
  h.A = power, h.W = e->spk.fb_bank, h.C = mel;
  h.a_div = kBig, h.a_s2 = nf, h.c_div = kBig, h.c_s2 = nb, h.st_div1 = 1, h.st_div2 = 1;
  h.M = static_cast<int>(M), h.N = nb, h.K = nf, h.ldw = nf, h.vec = 3;
  WS_RUN(e, ws_gemm_nt(&h, s));
  // log(max(x, eps)) = log(relu(x - eps) + eps)
  WS_RUN(e, ws_prelu_fwd(mel, e->spk.fb_floor, e->slope0, M, nb, static_cast<int>(M), feats, s));
  WS_RUN(e, ws_log_eps(feats, M * nb, kGnEps, s));
  if (te_tab) {
    WS_RUN(e, ws_cmn_len(feats, R, Te, nb, te_tab, feats, s));
  } else {
    const int rc = subtract_time_mean(e, feats, R, Te, nb);
    if (rc != WS_OK) return rc;
  }
  a.release(mk);
  return WS_OK;
}

// waveform [R][Tw] (device) -> log-mel features [R][Te][F], mean-normalised over time: the in-model front-end of
// spk_feat = False models (bsrnn.py:343-350; modules/common/frontend.py fbank_frontend); Te = 1 + Tw / 128
// len_tab_ / te_tab (ragged pass, device int[R]): the rows' samples and frames 1 + n / 128 -- the reflect padding turns at
// the row's own end, CMN runs over the row's frames, the tail is zeroed
int mel_frontend(ws_engine* e, const float* wav, int R, int Tw, float* feats, int Te, const int* len_tab_ = nullptr,
                 const int* te_tab = nullptr) {
  const int n = 512, hop = kHop, pad = n / 2, nf = n / 2 + 1, nm = e->spk.feat_dim;
  const int ldo = (Tw + 2 * pad + 3) / 4 * 4;
  const long long M = (long long)R * Te;
  void* s = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* xp = a.alloc(size_t(R) * ldo);
  float* spec = a.alloc(size_t(M) * e->spk.mel_lds);
  float* power = a.alloc(size_t(M) * e->spk.mel_ldp);
  WS_PTR(xp && spec && power);
  int rc = zero_device(e, xp, size_t(R) * ldo * 4);
  if (rc != WS_OK) return rc;
  if (len_tab_)
    WS_RUN(e, ws_preemph_pad_len(wav, R, Tw, pad, ldo, e->spk.mel_coef, len_tab_, xp, s));
  else
    WS_RUN(e, ws_preemph_pad(wav, R, Tw, pad, ldo, e->spk.mel_coef, xp, s));
  ws_gemm_nt_args g = {};
  g.A = xp, g.W = e->spk.mel_basis, g.C = spec;
  g.a_div = Te, g.a_s1 = ldo, g.a_s2 = hop;             // centred frames as an overlapping row view
  g.c_div = kBig, g.c_s2 = e->spk.mel_lds, g.st_div1 = 1, g.st_div2 = 1;
  g.M = static_cast<int>(M), g.N = e->spk.mel_lds, g.K = n, g.ldw = n, g.vec = 3;       // exact-fp32 products
  WS_RUN(e, ws_gemm_nt(&g, s));
  WS_RUN(e, ws_power_spec(spec, M, nf, e->spk.mel_lds, e->spk.mel_ldp, power, s));
  ws_gemm_nt_args h = {};
  h.A = power, h.W = e->spk.mel_fbt, h.C = feats;
  h.a_div = kBig, h.a_s2 = e->spk.mel_ldp, h.c_div = kBig, h.c_s2 = nm, h.st_div1 = 1, h.st_div2 = 1;
  h.M = static_cast<int>(M), h.N = nm, h.K = e->spk.mel_ldp, h.ldw = e->spk.mel_ldp, h.vec = 3;
  WS_RUN(e, ws_gemm_nt(&h, s));
  WS_RUN(e, ws_log_eps(feats, M * nm, 1e-8f, s));
  if (te_tab)
    WS_RUN(e, ws_cmn_len(feats, R, Te, nm, te_tab, feats, s));
  else if ((rc = subtract_time_mean(e, feats, R, Te, nm)) != WS_OK)
    return rc;
  a.release(mk);
  return WS_OK;
}

int spk_transform(ws_engine* e, const float* emb, int R, const float** out) {
  *out = emb;
  if (!e->use_xform) return WS_OK;
  Arena& a = e->work;
  const Tensor* t0 = e->find("spk_transform.transforms.0.weight");
  const int hid = static_cast<int>(t0->dims[0]);
  float* h0 = a.alloc(size_t(R) * hid);
  float* h1 = a.alloc(size_t(R) * hid);
  float* eo = a.alloc(size_t(R) * e->E);
  WS_PTR(h0 && h1 && eo);
  int rc;
  if ((rc = linear(e, emb, R, e->E, e->dev("spk_transform.transforms.0.weight"), e->E, hid,
                   e->dev("spk_transform.transforms.0.bias"), 0, h0)) != WS_OK ||
      (rc = linear(e, h0, R, hid, e->dev("spk_transform.transforms.1.weight"), hid, hid,
                   e->dev("spk_transform.transforms.1.bias"), 1, h1)) != WS_OK ||
      (rc = linear(e, h1, R, hid, e->dev("spk_transform.transforms.3.weight"), hid, e->E,
                   e->dev("spk_transform.transforms.3.bias"), 0, eo)) != WS_OK)
    return rc;
  *out = eo;
  return WS_OK;
}

// ---- the speaker stage as the separator plans see it -------------------------------------------------------------
struct EncoderPlan {        // per meta spk_kind
  int (*prep)(ws_engine* e);
  int (*embed)(ws_engine* e, const float* fbank, int R, int Te, float* emb, const std::vector<int>* tl);
};
const EncoderPlan kEncoders[3] = {{prep_resnet, resnet_embed}, {prep_ecapa, ecapa_embed}, {prep_campplus, campplus_embed}};

int prep_spk_transform(ws_engine* e) {
  if (!e->use_xform) return WS_OK;
  const Tensor* t0 = e->find("spk_transform.transforms.0.weight");
  if (!t0 || t0->dims.size() < 2 || t0->dims[1] != e->E || !e->find("spk_transform.transforms.1.weight") ||
      !e->find("spk_transform.transforms.3.weight")) {
    set_err("engine: spk_transform tensors missing or mis-shaped");
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

// load: the SpeakerTransform check, then for joint models the encoder (meta spk_kind) and its front-end (meta spk_feat)
int prep_speaker(ws_engine* e) {
  int rc = prep_spk_transform(e);
  if (rc != WS_OK || !e->joint) return rc;
  if ((rc = kEncoders[e->spk.kind].prep(e)) != WS_OK) return rc;
  return e->spk.feat ? prep_fbank(e) : prep_mel_frontend(e);
}

// enrollment -> embedding emb [R][E] (device): enroll is the host fbank [R][Te][F] (WS_ENROLL_FBANK) or waveform
// [R][enroll_len] (WS_ENROLL_WAVE, through the model's front-end to Te frames).  enroll_lengths / te_row: the ragged pass --
// every row's own length and frame count; the rectangle's tail may hold anything (it is selected away, never multiplied)
int speaker_embed(ws_engine* e, const void* enroll, int enroll_kind, int R, int enroll_len, int Te, float* emb,
                  const int* enroll_lengths, const int* te_row) {
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  int rc;
  const bool ragged = enroll_lengths && te_row;
  std::vector<int> tl;
  const int *d_len = nullptr, *d_te = nullptr;
  e->spk_tabs.clear();
  if (ragged) {
    if (!ragged_speaker_covered(e)) {
      set_err("engine: this speaker encoder has no ragged pass");
      return WS_ERR_INVALID;
    }
    // every width set of the forward in one upload, before the first launch: the rows' samples (WAVE), their frames, and
    // for the ResNets the frames after each of the three stride-2 stages (3x3, padding 1; the 1x1 stride-2 shortcut agrees)
    tl.assign(te_row, te_row + R);
    std::vector<std::vector<int>> sets;
    sets.push_back(std::vector<int>(enroll_lengths, enroll_lengths + R));
    sets.push_back(tl);
    if (e->spk.kind == 0)
      for (int i = 0; i < 3; ++i) sets.push_back(conv_widths(sets.back(), 3, 2, 1));
    std::vector<int> all;
    for (const auto& v : sets) all.insert(all.end(), v.begin(), v.end());
    const int* d = upload_ints(e, a, all);
    WS_PTR(d);
    d_len = d;
    d_te = d + R;
    for (size_t i = 1; i < sets.size(); ++i) e->spk_tabs.emplace_back(sets[i], d + i * R);
  }
  float* fb = a.alloc(size_t(R) * Te * e->spk.feat_dim);
  WS_PTR(fb);
  if (enroll_kind == WS_ENROLL_FBANK) {
    if ((rc = to_device(e, fb, enroll, size_t(R) * Te * e->spk.feat_dim * 4)) != WS_OK) return rc;
    // the caller's rectangle: whatever lies behind a row's frames is selected to zero
    if (ragged) WS_RUN(e, ws_tail_select_len(fb, R, Te, e->spk.feat_dim, d_te, fb, e->stream));
  } else {
    float* d_wave = a.alloc(size_t(R) * enroll_len);
    WS_PTR(d_wave);
    if ((rc = to_device(e, d_wave, enroll, size_t(R) * enroll_len * 4)) != WS_OK) return rc;
    if ((rc = e->spk.feat ? kaldi_fbank(e, d_wave, R, enroll_len, fb, Te, d_te)
                          : mel_frontend(e, d_wave, R, enroll_len, fb, Te, d_len, d_te)) != WS_OK)
      return rc;
  }
  rc = kEncoders[e->spk.kind].embed(e, fb, R, Te, emb, ragged ? &tl : nullptr);
  e->spk_tabs.clear();
  if (rc != WS_OK) return rc;
  a.release(mk);
  return WS_OK;
}

}  // namespace wsrt
