// =================================================================================================================
// The streaming runtime of a causal cLN Conv-TasNet / SpEx+ container (tasnet_plan.cc).  Only two kernels of a causal model
// look across time; their chunked forms (wesep_hip.h: ws_tcn_mid_stream_fwd, ws_ola_stream_fwd and the _rows forms of a pool)
// carry a ring of normalised past frames per block and the not-yet-final samples of the overlap-add.
// What the four front ends share lives here, once:
//   stream_chain      the launch chain of a group of frames over a rectangle: 3 framing GEMMs, row statistics, projection; per
//                     block GEMM, the fused middle, GEMM -- or ONE call, the block kernel (WS_STREAM_BLOCK_KERNEL); mask GEMM,
//                     mask product, synthesis GEMM, overlap-add.  The solo and the rows form differ in how the time-crossing
//                     kernels address their rows (ChainRows), in nothing else
//   stream_core_*     the state block (StreamCore): ONE device allocation made at open and owned by the stream or pool (the
//                     engine's arenas may be reset or rebuilt by other calls between two pushes) -- rings, the owner's parts,
//                     row biases, an optional extra part; every weight pointer is resolved once, at open
//   stream_enroll     the speaker stage of some rows of a stream
// Transient activations come from the engine's work arena under an ArenaScope.
// ws_engine_stream_*: the native form of wesep_amd/streaming.py's ConvTasNetStreamer, with its emission rule.  Per group of at
// most max_chunk_frames frames: the chain and the copy that moves the unconsumed pending samples to the other buffer -- 3 R X +
// 10 entry-point calls (WS_STREAM_GROUP_LAUNCHES), R X + 10 with the block kernel (WS_STREAM_BLOCK_GROUP_LAUNCHES).
// =================================================================================================================
#include <optional>

#include "engine_internal.h"

using namespace wsrt;

namespace {

void resolve_stream_weights(const ws_engine* e, StreamWeights* w) {   // blocks: weights, ldw and dil; cap, ring, rb: stream_core_open
  const TasNet& t = e->tas;
  const char* enc[3] = {"encoder.encoder_1d_short.", "encoder.encoder_1d_middle.", "encoder.encoder_1d_long."};
  for (int i = 0; i < 3; ++i) w->enc_w[i] = e->dev(std::string(enc[i]) + "weight"), w->enc_b[i] = e->dev(std::string(enc[i]) + "bias");
  w->ln_g = e->dev("encoder.ln.weight"), w->ln_b = e->dev("encoder.ln.bias");
  w->proj_w = e->dev("encoder.proj.weight"), w->proj_b = e->dev("encoder.proj.bias");
  w->mask_w = e->dev("decoder.mask1.weight"), w->mask_b = e->dev("decoder.mask1.bias"), w->dec_b = e->dev("decoder.decoder_1d_1.bias");
  w->blocks.clear();
  for (int r = 0; r < t.R; ++r)
    for (int k = 0; k < t.X; ++k) {
      const bool fuse = k == 0;
      const std::string pre = fuse ? "separation.separation." + std::to_string(2 * r) + "."
                                   : "separation.separation." + std::to_string(2 * r + 1) + ".separation." + std::to_string(k - 1) + ".";
      const std::string n1 = pre + (fuse ? "lnorm1." : "norm_1."), n2 = pre + (fuse ? "lnorm2." : "norm_2.");
      const std::string dw = pre + (fuse ? "dconv." : "dwconv."), outc = pre + (fuse ? "sconv." : "Output.");
      StreamBlock b;
      b.w1 = e->dev(pre + "conv1x1.weight"), b.b1 = e->dev(pre + "conv1x1.bias"), b.ldw = fuse ? t.B + e->E : t.B;
      b.a1 = e->dev(pre + (fuse ? "prelu1.weight" : "PReLU_1.weight")), b.a2 = e->dev(pre + (fuse ? "prelu2.weight" : "PReLU_2.weight"));
      b.g1 = e->dev(n1 + "weight"), b.be1 = e->dev(n1 + "bias"), b.g2 = e->dev(n2 + "weight"), b.be2 = e->dev(n2 + "bias");
      b.wd = e->dev(dw + "weight"), b.bd = e->dev(dw + "bias"), b.w3 = e->dev(outc + "weight"), b.b3 = e->dev(outc + "bias");
      b.dil = 1 << k, b.cap = 0, b.ring = nullptr, b.rb = nullptr;
      w->blocks.push_back(b);
    }
}

}  // namespace

namespace wsrt {

int refuse_not_streamable(const ws_engine* e, const char* who) {
  if (e->arch != 1)
    set_err("%s: this container holds arch %d; streaming is built for causal cLN Conv-TasNet / SpEx+ (arch 1)", who, e->arch);
  else
    set_err("%s: this Conv-TasNet container is %s with %s; streaming needs causal blocks with cLN (gLN takes "
            "its statistics over the whole utterance, non-causal blocks look ahead)", who, e->tas.causal ? "causal" : "non-causal",
            e->tas.norm == 1 ? "cLN" : "gLN");
  return WS_ERR_INVALID;
}

int stream_chain(ws_engine* e, const StreamWeights& w, bool block_kernel, const float* x0, long long pitch, const ChainRows& r,
                 float* carry, float** est_out) {
  const TasNet& t = e->tas;
  const int N = t.N, L = t.L, B = t.B, H = t.H, P = t.P, s = L / 2, R = r.rows, Tc = r.Tc;
  const long long M = (long long)R * Tc;
  void* q = e->stream;
  Arena& a = e->work;
  float* cat = a.alloc(size_t(M) * 3 * N);
  float* st0 = a.alloc(size_t(M) * 2);
  float* xa = a.alloc(size_t(M) * B);
  float* xb = a.alloc(size_t(M) * B);
  float* c = a.alloc(size_t(M) * H);      // (c, y2 and st2 stay unused with the block kernel)
  float* y2 = a.alloc(size_t(M) * H);
  float* st2 = a.alloc(size_t(M) * 2);
  float* m = a.alloc(size_t(M) * N);
  float* sm = a.alloc(size_t(M) * N);
  float* fr = a.alloc(size_t(M) * L);
  float* est = a.alloc(size_t(R) * Tc * s);
  WS_PTR(cat && st0 && xa && xb && c && y2 && st2 && m && sm && fr && est);
  int rc;
  const int Ls[3] = {L, 80, kEncLmax};
  for (int i = 0; i < 3; ++i) {
    TasGemm g;
    g.A = x0, g.a_div = Tc, g.a_s1 = pitch, g.lda = s, g.M = M, g.K = Ls[i], g.W = w.enc_w[i], g.ldw = Ls[i], g.N = N;
    g.bias = w.enc_b[i], g.act = 2, g.C = cat + (long long)i * N, g.ldc = 3 * N;
    if ((rc = tas_gemm(e, g)) != WS_OK) return rc;
  }
  if ((rc = tas_row_stats(e, cat, M, 3 * N, st0)) != WS_OK) return rc;
  {
    TasGemm g;
    g.A = cat, g.lda = 3 * N, g.M = M, g.K = 3 * N, g.W = w.proj_w, g.ldw = 3 * N, g.N = B, g.bias = w.proj_b, g.C = xa, g.ldc = B;
    g.stats = st0, g.gamma = w.ln_g, g.beta = w.ln_b, g.st_div1 = 1;
    if ((rc = tas_gemm(e, g)) != WS_OK) return rc;
  }
  float *x = xa, *other = xb;
  for (const StreamBlock& b : w.blocks) {
    if (block_kernel) {
      if (r.d_slot)
        WS_RUN(e, ws_tcn_block_stream_rows_fwd(x, b.rb, b.w1, b.ldw, b.rb ? nullptr : b.b1, b.a1, b.g1, b.be1, b.wd, b.bd, b.a2, b.g2,
                                               b.be2, b.w3, b.b3, R, Tc, B, H, P, b.dil, kLnEps, r.nslots, r.d_slot, r.d_t0, r.d_tc,
                                               b.cap, b.ring, other, q));
      else
        WS_RUN(e, ws_tcn_block_stream_fwd(x, b.rb, b.w1, b.ldw, b.rb ? nullptr : b.b1, b.a1, b.g1, b.be1, b.wd, b.bd, b.a2, b.g2, b.be2,
                                          b.w3, b.b3, R, Tc, B, H, P, b.dil, kLnEps, r.t0, b.cap, b.ring, other, q));
      std::swap(x, other);
      continue;
    }
    TasGemm g;
    g.A = x, g.lda = B, g.M = M, g.K = B, g.W = b.w1, g.ldw = b.ldw, g.N = H, g.bias = b.rb ? nullptr : b.b1, g.C = c, g.ldc = H;
    if ((rc = tas_gemm(e, g)) != WS_OK) return rc;
    if (r.d_slot)
      WS_RUN(e, ws_tcn_mid_stream_rows_fwd(c, b.rb, b.a1, b.g1, b.be1, b.wd, b.bd, b.a2, R, Tc, H, P, b.dil, kLnEps, r.nslots, r.d_slot,
                                           r.d_t0, r.d_tc, b.cap, b.ring, y2, st2, q));
    else
      WS_RUN(e, ws_tcn_mid_stream_fwd(c, b.rb, b.a1, b.g1, b.be1, b.wd, b.bd, b.a2, R, Tc, H, P, b.dil, kLnEps, r.t0, b.cap, b.ring, y2,
                                      st2, q));
    TasGemm o;
    o.A = y2, o.lda = H, o.M = M, o.K = H, o.W = b.w3, o.ldw = H, o.N = B, o.bias = b.b3, o.C = other, o.ldc = B, o.R = x;
    o.stats = st2, o.gamma = b.g2, o.beta = b.be2, o.st_div1 = 1;
    if ((rc = tas_gemm(e, o)) != WS_OK) return rc;
    std::swap(x, other);
  }
  TasGemm g;
  g.A = x, g.lda = B, g.M = M, g.K = B, g.W = w.mask_w, g.ldw = B, g.N = N, g.bias = w.mask_b, g.act = 2, g.C = m, g.ldc = N;
  if ((rc = tas_gemm(e, g)) != WS_OK) return rc;
  WS_RUN(e, ws_maskmul_fwd(cat, 3 * N, m, M, N, sm, q));
  TasGemm d;
  d.A = sm, d.lda = N, d.M = M, d.K = N, d.W = t.dec_wt, d.ldw = N, d.N = L, d.C = fr, d.ldc = L;
  if ((rc = tas_gemm(e, d)) != WS_OK) return rc;
  if (r.d_slot)
    WS_RUN(e, ws_ola_stream_rows_fwd(fr, w.dec_b, R, Tc, L, s, r.nslots, r.d_slot, r.d_t0, r.d_tc, carry, est, q));
  else
    WS_RUN(e, ws_ola_stream_fwd(fr, w.dec_b, R, Tc, L, s, carry, est, q));
  *est_out = est;
  return WS_OK;
}

int stream_core_check(const ws_engine* e, const char* who, const char* noun, int rows, int G) {
  const TasNet& t = e->tas;
  if ((long long)rows * G * 3 * t.N > 0x7fffffffLL || (long long)rows * ((long long)(t.P - 1) * (1 << (t.X - 1)) + G) * t.H > 0x7fffffffLL) {
    set_err("%s: %s=%d with max_chunk_frames=%d reaches 2^31 elements in one buffer", who, noun, rows, G);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

int stream_core_open(StreamCore* c, const char* who, ws_engine* e, int rows, int G, unsigned flags, const std::vector<size_t>& parts,
                     size_t extra_floats, std::vector<float*>* at) {
  const TasNet& t = e->tas;
  c->e = e, c->rows = rows, c->G = G, c->block_kernel = (flags & WS_STREAM_BLOCK_KERNEL) != 0;
  std::vector<size_t> off;
  size_t total = 0;
  auto part = [&](size_t nfloats) {
    off.push_back(total);
    total += Arena::round_up(nfloats * 4);
  };
  for (int r = 0; r < t.R; ++r)
    for (int k = 0; k < t.X; ++k) part(size_t(rows) * ((size_t)(t.P - 1) * (1 << k) + G) * t.H);
  for (size_t n : parts) part(n);
  for (int r = 0; r < t.R; ++r) part(size_t(rows) * t.H);
  if (extra_floats) part(extra_floats);
  c->state_bytes = total;
  if (e->dry) {
    c->state = static_cast<char*>(malloc(total));
  } else if (hipMalloc(reinterpret_cast<void**>(&c->state), total) != hipSuccess) {
    c->state = nullptr;
  }
  if (!c->state) {
    set_err("%s: device allocation of %zu bytes failed", who, total);
    return WS_ERR_LAUNCH;
  }
  if (e->work.poison && !e->dry) {      // WS_ENGINE_POISON (tests): state no launch has written reads as NaN
    (void)hipDeviceSynchronize();
    (void)hipMemset(c->state, 0xFF, total);
    (void)hipDeviceSynchronize();
  }
  size_t si = 0;
  auto next = [&] { return reinterpret_cast<float*>(c->state + off[si++]); };
  resolve_stream_weights(e, c);
  for (StreamBlock& b : c->blocks) b.cap = (t.P - 1) * b.dil + G, b.ring = next();
  for (size_t i = 0; i < parts.size(); ++i) at->push_back(next());
  for (int r = 0; r < t.R; ++r) c->rb.push_back(next()), c->blocks[size_t(r) * t.X].rb = c->rb[r];
  if (extra_floats) at->push_back(next());
  return WS_OK;
}

void stream_core_free(StreamCore* c) {
  if (!c->state) return;
  if (c->e->dry)
    free(c->state);
  else
    (void)hipFree(c->state);
  c->state = nullptr;
}

int stream_enroll(StreamCore* c, const char* who, const void* enroll, int enroll_kind, int enroll_len, int row0, int n) {
  ws_engine* e = c->e;
  const TasNet& t = e->tas;
  ArenaScope scope(e->work);
  float* d_emb = e->work.alloc(size_t(n) * e->E);
  WS_PTR(d_emb);
  const float* embp = nullptr;
  float* emb = c->emb + size_t(row0) * e->E;
  int rc;
  if ((rc = speaker_stage(e, enroll, enroll_kind, n, enroll_len, enroll_len, nullptr, nullptr, d_emb)) != WS_OK) return rc;
  if ((rc = spk_transform(e, d_emb, n, &embp)) != WS_OK) return rc;
  if ((rc = copy_async(e, who, "device copy", emb, embp, size_t(n) * e->E * 4, hipMemcpyDeviceToDevice)) != WS_OK) return rc;
  for (int r = 0; r < t.R; ++r) {
    const StreamBlock& b = c->blocks[size_t(r) * t.X];
    if ((rc = linear(e, emb, n, e->E, b.w1 + t.B, t.B + e->E, t.H, b.b1, 0, c->rb[r] + size_t(row0) * t.H)) != WS_OK) return rc;
  }
  return WS_OK;
}

}  // namespace wsrt

struct ws_stream : wsrt::StreamCore {   // carry0 is [rows][L - s]
  int pcap = 0;                         // floats per row of a pending buffer: G s + kEncLmax rounded up to 4
  float* pend[2] = {nullptr, nullptr};
  int cur = 0, npend = 0;
  long long n = 0, k = 0;               // samples pushed, frames run
  bool done = false, failed = false;
  bool dev_io = false;                  // the inner stream of a rate stream (rate.cc): chunks and estimates are DEVICE buffers
};

namespace {

constexpr const char* kWho = "ws_engine_stream";

int zero_cols(ws_engine* e, float* p, int pitch, int from, int to, int rows) {
  if (to <= from) return WS_OK;
  if (e->dry) {
    for (int r = 0; r < rows; ++r) memset(p + size_t(r) * pitch + from, 0, size_t(to - from) * 4);
    return WS_OK;
  }
  if (hipMemset2DAsync(p + from, size_t(pitch) * 4, 0, size_t(to - from) * 4, rows, e->stream) != hipSuccess) {
    set_err("ws_engine_stream: memset failed");
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

// frames [k, k + Tc) from the first (Tc - 1) s + kEncLmax pending samples; est [rows][Tc s] goes to host columns [col, col + Tc s)
// (a rate stream's inner stream: est is a device buffer, the copy is device to device)
int run_group(ws_stream* st, int Tc, float* host_est, long long host_pitch, int col) {
  ws_engine* e = st->e;
  const int s = e->tas.L / 2, R = st->rows;
  ArenaScope scope(e->work);
  ChainRows rows;
  rows.rows = R, rows.Tc = Tc, rows.t0 = st->k;
  float* est = nullptr;
  int rc;
  if ((rc = stream_chain(e, *st, st->block_kernel, st->pend[st->cur], st->pcap, rows, st->carry, &est)) != WS_OK) return rc;
  if ((rc = copy_async(e, kWho, "device-to-host copy", host_est + col, size_t(host_pitch) * 4, est, size_t(Tc) * s * 4, size_t(Tc) * s * 4,
                       R, st->dev_io ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost)) != WS_OK)
    return rc;
  // the unconsumed pending samples move to the OTHER buffer (no overlapping copy in place)
  const int keep = st->npend - Tc * s;
  ++e->n_launches;
  if ((rc = copy_async(e, kWho, "pending-sample copy", st->pend[1 - st->cur], size_t(st->pcap) * 4, st->pend[st->cur] + Tc * s,
                       size_t(st->pcap) * 4, size_t(keep) * 4, R, hipMemcpyDeviceToDevice)) != WS_OK)
    return rc;
  st->cur ^= 1;
  st->npend = keep;
  st->k += Tc;
  return WS_OK;
}

int check_stream(const ws_stream* s, const char* who) {
  if (!s || !s->e) {
    set_err("%s: null stream", who);
    return WS_ERR_INVALID;
  }
  if (s->failed) {
    set_err("%s: an earlier call on this stream failed half way; call ws_engine_stream_reset", who);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

int reset_state(ws_stream* s) {
  ws_engine* e = s->e;
  s->n = s->k = 0, s->npend = 0, s->cur = 0, s->done = s->failed = false;
  return copy_async(e, "ws_engine_stream_reset", "device copy", s->carry, s->carry0, size_t(s->rows) * (e->tas.L - e->tas.L / 2) * 4,
                    hipMemcpyDeviceToDevice);
}

void free_stream(ws_stream* s) {
  stream_core_free(s);
  delete s;
}

}  // namespace

WS_ENGINE_API int ws_engine_stream_open(ws_engine* e, int rows, const void* enroll, int enroll_kind, int enroll_len,
                                        int max_chunk_frames, ws_stream** out) {
  return ws_engine_stream_open_ex(e, rows, enroll, enroll_kind, enroll_len, max_chunk_frames, 0, out);
}

WS_ENGINE_API int ws_engine_stream_open_ex(ws_engine* e, int rows, const void* enroll, int enroll_kind, int enroll_len,
                                           int max_chunk_frames, unsigned flags, ws_stream** out) {
  return wsrt::stream_open_impl(e, rows, enroll, enroll_kind, enroll_len, max_chunk_frames, flags, 0, out, nullptr);
}

// extra_floats > 0: the state allocation gets one more part of that many floats, returned in *extra, and the stream takes
// and returns DEVICE buffers (stream_push_impl / stream_flush_impl): the inner stream of a rate stream (rate.cc)
int wsrt::stream_open_impl(ws_engine* e, int rows, const void* enroll, int enroll_kind, int enroll_len, int max_chunk_frames,
                           unsigned flags, size_t extra_floats, ws_stream** out, float** extra) {
  const char* who = "ws_engine_stream_open";
  int rc = check_engine(e, who);
  if (rc != WS_OK) return rc;
  if (out) *out = nullptr;
  if (!tas_streamable(e)) return refuse_not_streamable(e, who);
  if (flags & ~unsigned(WS_STREAM_BLOCK_KERNEL)) {
    set_err("ws_engine_stream_open_ex: unknown flag bits 0x%x (known: WS_STREAM_BLOCK_KERNEL = 1)", flags & ~unsigned(WS_STREAM_BLOCK_KERNEL));
    return WS_ERR_INVALID;
  }
  if (!enroll || !out || rows < 1 || max_chunk_frames < 1 || max_chunk_frames > 65536) {
    set_err("ws_engine_stream_open: bad arguments (rows=%d, max_chunk_frames=%d in [1, 65536], enroll %s, out %s)", rows,
            max_chunk_frames, enroll ? "given" : "NULL", out ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  if ((rc = tasnet_check_enroll(e, enroll_kind, enroll_len)) != WS_OK) return rc;
  const int L = e->tas.L, s = L / 2, G = max_chunk_frames;
  if ((rc = stream_core_check(e, who, "rows", rows, G)) != WS_OK) return rc;
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  ws_stream* st = new ws_stream();
  st->pcap = (G * s + kEncLmax + 3) / 4 * 4;
  st->dev_io = extra_floats != 0;
  // the stream's parts of the state block: carry, its reset image, two pending buffers, embedding
  const size_t nc = size_t(rows) * (L - s), np = size_t(rows) * st->pcap;
  std::vector<float*> at;
  if ((rc = stream_core_open(st, who, e, rows, G, flags, {nc, nc, np, np, size_t(rows) * e->E}, extra_floats, &at)) == WS_OK) {
    st->carry = at[0], st->carry0 = at[1], st->pend[0] = at[2], st->pend[1] = at[3], st->emb = at[4];
    if (extra_floats) *extra = at[5];
    rc = stream_enroll(st, who, enroll, enroll_kind, enroll_len, 0, rows);     // the speaker stage, once
  }
  if (rc == WS_OK) {                    // the reset image of the carry: the decoder bias
    const std::vector<float> c0(nc, e->host("decoder.decoder_1d_1.bias")[0]);
    rc = to_device(e, st->carry0, c0.data(), c0.size() * 4);
  }
  if (rc == WS_OK) rc = reset_state(st);
  if (rc == WS_OK) rc = sync_stream(e, kWho);
  if (rc != WS_OK) {
    free_stream(st);
    return rc;
  }
  e->stream_state_bytes = static_cast<long long>(st->state_bytes);
  *out = st;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_stream_push(ws_stream* st, const float* chunk, int n, float* est, int est_cap, int* n_out) {
  if (st && st->dev_io) {
    set_err("ws_engine_stream_push: this stream belongs to a rate stream; use ws_engine_rate_stream_push");
    return WS_ERR_INVALID;
  }
  return wsrt::stream_push_impl(st, chunk, n, n, est, -1, est_cap, n_out);
}

// The plain stream (host chunk and est, est's row pitch is the emitted count: est_pitch < 0), or the inner stream of a rate
// stream (dev_io: device chunk and est of the given pitches; the caller holds the turn, counts the launches over its whole
// call and synchronises once, after its own last copy).
int wsrt::stream_push_impl(ws_stream* st, const float* chunk, long long chunk_pitch, int n, float* est, long long est_pitch,
                           int est_cap, int* n_out) {
  int rc = check_stream(st, "ws_engine_stream_push");
  if (rc != WS_OK) return rc;
  ws_engine* e = st->e;
  const int L = e->tas.L, s = L / 2, R = st->rows;
  if (st->done) {
    set_err("ws_engine_stream_push: the stream was flushed (call ws_engine_stream_reset to start another)");
    return WS_ERR_INVALID;
  }
  if (!chunk || !n_out || n < 1) {
    set_err("ws_engine_stream_push: bad arguments (n=%d >= 1, chunk %s, n_out %s)", n, chunk ? "given" : "NULL", n_out ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  const long long emit = (plain_frames(st->n + n, L) - st->k) * s;
  if (emit > est_cap || (emit > 0 && !est)) {
    set_err("ws_engine_stream_push: this push emits %lld samples a row, est_cap is %d (WS_STREAM_PUSH_CAP(n, L) = %d always suffices)",
            emit, est_cap, WS_STREAM_PUSH_CAP(n, L));
    return WS_ERR_INVALID;
  }
  const bool dev = st->dev_io;
  std::optional<ForwardTurn> turn;      // (the caller of a device-buffer stream holds the turn)
  if (!dev) turn.emplace(e);
  if (turn && turn->rc != WS_OK) return turn->rc;
  e->long_windows = e->long_forwards = 0;
  if (!dev) e->n_launches = 0;
  if (est_pitch < 0) est_pitch = emit;
  st->failed = true;                    // until the push is complete
  int off = 0, col = 0;
  while (off < n) {
    // at most G s + kEncLmax - 1 pending samples: a piece completes at most G frames, one group (and fewer than kEncLmax stay pending)
    const int take = std::min(n - off, st->G * s + kEncLmax - 1 - st->npend);
    if ((rc = copy_async(e, kWho, "host-to-device copy", st->pend[st->cur] + st->npend, size_t(st->pcap) * 4, chunk + off,
                         size_t(chunk_pitch) * 4, size_t(take) * 4, R, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)) != WS_OK)
      return rc;
    st->npend += take, off += take, st->n += take;
    while (st->npend >= kEncLmax) {
      const int Tc = std::min((st->npend - kEncLmax) / s + 1, st->G);
      if ((rc = run_group(st, Tc, est, est_pitch, col)) != WS_OK) return rc;
      col += Tc * s;
    }
  }
  if (!dev && (rc = sync_stream(e, kWho)) != WS_OK) return rc;     // the one host synchronisation of a push
  st->failed = false;
  *n_out = static_cast<int>(emit);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_stream_flush(ws_stream* st, float* est, int est_cap, int* n_out) {
  if (st && st->dev_io) {
    set_err("ws_engine_stream_flush: this stream belongs to a rate stream; use ws_engine_rate_stream_flush");
    return WS_ERR_INVALID;
  }
  return wsrt::stream_flush_impl(st, est, -1, est_cap, n_out);
}

int wsrt::stream_flush_impl(ws_stream* st, float* est, long long est_pitch, int est_cap, int* n_out) {
  int rc = check_stream(st, "ws_engine_stream_flush");
  if (rc != WS_OK) return rc;
  ws_engine* e = st->e;
  const int L = e->tas.L, s = L / 2, R = st->rows;
  if (st->done) {
    set_err("ws_engine_stream_flush: the stream was flushed already (call ws_engine_stream_reset)");
    return WS_ERR_INVALID;
  }
  if (st->n < L) {
    set_err("ws_engine_stream_flush: %lld samples were pushed, fewer than the encoder window L = %d", st->n, L);
    return WS_ERR_INVALID;
  }
  const long long target = plain_frames(st->n, L, true);
  const long long emit = (target - st->k) * s + (L - s);
  if (!est || !n_out || emit > est_cap) {
    set_err("ws_engine_stream_flush: the flush emits %lld samples a row, est_cap is %d%s (WS_STREAM_FLUSH_CAP = %d always suffices)",
            emit, est_cap, est && n_out ? "" : ", est or n_out is NULL", WS_STREAM_FLUSH_CAP);
    return WS_ERR_INVALID;
  }
  const bool dev = st->dev_io;
  std::optional<ForwardTurn> turn;      // (the caller of a device-buffer stream holds the turn)
  if (!dev) turn.emplace(e);
  if (turn && turn->rc != WS_OK) return turn->rc;
  e->long_windows = e->long_forwards = 0;
  if (!dev) e->n_launches = 0;
  if (est_pitch < 0) est_pitch = emit;
  st->failed = true;
  int col = 0;
  while (st->k < target) {
    // zero-extend, as the whole-utterance encoder does at its end: the buffer counts as full of (zero) samples
    if ((rc = zero_cols(e, st->pend[st->cur], st->pcap, st->npend, st->pcap, R)) != WS_OK) return rc;
    st->npend = st->pcap;
    const int Tc = static_cast<int>(std::min<long long>(target - st->k, st->G));
    if ((rc = run_group(st, Tc, est, est_pitch, col)) != WS_OK) return rc;
    col += Tc * s;
  }
  if ((rc = copy_async(e, kWho, "device-to-host copy", est + col, size_t(est_pitch) * 4, st->carry, size_t(L - s) * 4, size_t(L - s) * 4, R,
                       dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost)) != WS_OK)
    return rc;
  if (!dev && (rc = sync_stream(e, kWho)) != WS_OK) return rc;
  st->failed = false;
  st->done = true;
  *n_out = static_cast<int>(emit);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_stream_reset(ws_stream* st) {
  if (!st || !st->e) {
    set_err("ws_engine_stream_reset: null stream");
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(st->e);
  if (turn.rc != WS_OK) return turn.rc;
  int rc = reset_state(st);
  if (rc != WS_OK) return rc;
  return sync_stream(st->e, kWho);
}

WS_ENGINE_API void ws_engine_stream_close(ws_stream* st) {
  if (!st) return;
  if (st->e && !st->e->dry) {
    (void)hipSetDevice(st->e->device);
    (void)hipStreamSynchronize(st->e->stream);
  }
  free_stream(st);
}
