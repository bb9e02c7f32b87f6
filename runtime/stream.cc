// =================================================================================================================
// ws_engine_stream_*: a causal cLN Conv-TasNet / SpEx+ container (tasnet_plan.cc) fed audio as it arrives -- the native
// form of wesep_amd/streaming.py's ConvTasNetStreamer, with its emission rule.  Only two kernels of a causal model look
// across time; their chunked forms (wesep_hip.h: ws_tcn_mid_stream_fwd, ws_ola_stream_fwd) carry a ring of normalised past
// frames per block and the not-yet-final samples of the overlap-add.  All carried state is ONE device allocation owned by
// the stream (the engine's arenas may be reset or rebuilt by other calls between two pushes); transient activations come
// from the engine's work arena under mark / release.  Every weight pointer is resolved once, at open.
// Per group of at most max_chunk_frames frames: 3 framing GEMMs, row statistics, projection; per block GEMM, the fused
// middle, GEMM; mask GEMM, mask product, synthesis GEMM, overlap-add; the copy that moves the unconsumed pending samples
// to the other buffer -- 3 R X + 10 entry-point calls (WS_STREAM_GROUP_LAUNCHES).  A stream opened with
// WS_STREAM_BLOCK_KERNEL runs every block as ONE call, ws_tcn_block_stream_fwd: R X + 10 (WS_STREAM_BLOCK_GROUP_LAUNCHES).
// =================================================================================================================
#include <optional>

#include "engine_internal.h"

using namespace wsrt;

namespace {

constexpr int kLmax = 160;     // the longest window of the MultiEncoder (encoder.py:66-114)

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

void resolve_stream_weights(const ws_engine* e, StreamWeights* w) {
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

}  // namespace wsrt

struct ws_stream : wsrt::StreamWeights {
  ws_engine* e = nullptr;
  int rows = 0, G = 0, pcap = 0;        // pcap: floats per row of a pending buffer, G * s + 160 rounded up to 4
  char* state = nullptr;                // the one allocation
  size_t state_bytes = 0;
  std::vector<float*> rb;               // per stack [rows][H]
  float *carry = nullptr, *carry0 = nullptr, *emb = nullptr, *pend[2] = {nullptr, nullptr};
  int cur = 0, npend = 0;
  long long n = 0, k = 0;               // samples pushed, frames run
  bool done = false, failed = false;
  bool block_kernel = false;            // WS_STREAM_BLOCK_KERNEL: one call per block
  bool dev_io = false;                  // the inner stream of a rate stream (rate.cc): chunks and estimates are DEVICE buffers
};

namespace {

int copy2d(ws_engine* e, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind,
           const char* what) {
  if (width == 0 || height == 0) return WS_OK;
  if (e->dry) return WS_OK;
  if (hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, e->stream) != hipSuccess) {
    set_err("ws_engine_stream: %s failed", what);
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

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

// frames [k, k + Tc) from the first (Tc - 1) s + 160 pending samples; est [rows][Tc s] goes to host columns [col, col + Tc s)
// (a rate stream's inner stream: est is a device buffer, the copy is device to device)
int run_group(ws_stream* st, int Tc, float* host_est, long long host_pitch, int col) {
  ws_engine* e = st->e;
  const TasNet& t = e->tas;
  const int N = t.N, L = t.L, B = t.B, H = t.H, P = t.P, s = L / 2, R = st->rows;
  const long long M = (long long)R * Tc;
  void* q = e->stream;
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* cat = a.alloc(size_t(M) * 3 * N);
  float* st0 = a.alloc(size_t(M) * 2);
  float* xa = a.alloc(size_t(M) * B);
  float* xb = a.alloc(size_t(M) * B);
  float* c = a.alloc(size_t(M) * H);
  float* y2 = a.alloc(size_t(M) * H);
  float* st2 = a.alloc(size_t(M) * 2);
  float* m = a.alloc(size_t(M) * N);
  float* sm = a.alloc(size_t(M) * N);
  float* fr = a.alloc(size_t(M) * L);
  float* est = a.alloc(size_t(R) * Tc * s);
  WS_PTR(cat && st0 && xa && xb && c && y2 && st2 && m && sm && fr && est);
  int rc;
  const int Ls[3] = {L, 80, kLmax};
  const float* x0 = st->pend[st->cur];
  for (int i = 0; i < 3; ++i) {
    TasGemm g;
    g.A = x0, g.a_div = Tc, g.a_s1 = st->pcap, g.lda = s, g.M = M, g.K = Ls[i], g.W = st->enc_w[i], g.ldw = Ls[i], g.N = N;
    g.bias = st->enc_b[i], g.act = 2, g.C = cat + (long long)i * N, g.ldc = 3 * N;
    if ((rc = tas_gemm(e, g)) != WS_OK) return rc;
  }
  if ((rc = tas_row_stats(e, cat, M, 3 * N, st0)) != WS_OK) return rc;
  {
    TasGemm g;
    g.A = cat, g.lda = 3 * N, g.M = M, g.K = 3 * N, g.W = st->proj_w, g.ldw = 3 * N, g.N = B, g.bias = st->proj_b, g.C = xa, g.ldc = B;
    g.stats = st0, g.gamma = st->ln_g, g.beta = st->ln_b, g.st_div1 = 1;
    if ((rc = tas_gemm(e, g)) != WS_OK) return rc;
  }
  float *x = xa, *other = xb;
  for (const StreamBlock& b : st->blocks) {
    if (st->block_kernel) {
      WS_RUN(e, ws_tcn_block_stream_fwd(x, b.rb, b.w1, b.ldw, b.rb ? nullptr : b.b1, b.a1, b.g1, b.be1, b.wd, b.bd, b.a2, b.g2, b.be2,
                                        b.w3, b.b3, R, Tc, B, H, P, b.dil, kLnEps, st->k, b.cap, b.ring, other, q));
      std::swap(x, other);
      continue;
    }
    TasGemm g;
    g.A = x, g.lda = B, g.M = M, g.K = B, g.W = b.w1, g.ldw = b.ldw, g.N = H, g.bias = b.rb ? nullptr : b.b1, g.C = c, g.ldc = H;
    if ((rc = tas_gemm(e, g)) != WS_OK) return rc;
    WS_RUN(e, ws_tcn_mid_stream_fwd(c, b.rb, b.a1, b.g1, b.be1, b.wd, b.bd, b.a2, R, Tc, H, P, b.dil, kLnEps, st->k, b.cap, b.ring,
                                    y2, st2, q));
    TasGemm o;
    o.A = y2, o.lda = H, o.M = M, o.K = H, o.W = b.w3, o.ldw = H, o.N = B, o.bias = b.b3, o.C = other, o.ldc = B, o.R = x;
    o.stats = st2, o.gamma = b.g2, o.beta = b.be2, o.st_div1 = 1;
    if ((rc = tas_gemm(e, o)) != WS_OK) return rc;
    std::swap(x, other);
  }
  {
    TasGemm g;
    g.A = x, g.lda = B, g.M = M, g.K = B, g.W = st->mask_w, g.ldw = B, g.N = N, g.bias = st->mask_b, g.act = 2, g.C = m, g.ldc = N;
    if ((rc = tas_gemm(e, g)) != WS_OK) return rc;
    WS_RUN(e, ws_maskmul_fwd(cat, 3 * N, m, M, N, sm, q));
    TasGemm d;
    d.A = sm, d.lda = N, d.M = M, d.K = N, d.W = t.dec_wt, d.ldw = N, d.N = L, d.C = fr, d.ldc = L;
    if ((rc = tas_gemm(e, d)) != WS_OK) return rc;
    WS_RUN(e, ws_ola_stream_fwd(fr, st->dec_b, R, Tc, L, s, st->carry, est, q));
  }
  if ((rc = copy2d(e, host_est + col, size_t(host_pitch) * 4, est, size_t(Tc) * s * 4, size_t(Tc) * s * 4, R,
                   st->dev_io ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, "device-to-host copy")) != WS_OK)
    return rc;
  // the unconsumed pending samples move to the OTHER buffer (no overlapping copy in place)
  const int keep = st->npend - Tc * s;
  ++e->n_launches;
  if ((rc = copy2d(e, st->pend[1 - st->cur], size_t(st->pcap) * 4, st->pend[st->cur] + Tc * s, size_t(st->pcap) * 4, size_t(keep) * 4, R,
                   hipMemcpyDeviceToDevice, "pending-sample copy")) != WS_OK)
    return rc;
  st->cur ^= 1;
  st->npend = keep;
  st->k += Tc;
  a.release(mk);
  return WS_OK;
}

int sync_stream(ws_engine* e) {
  if (!e->dry && hipStreamSynchronize(e->stream) != hipSuccess) {
    set_err("ws_engine_stream: the device reported an error");
    return WS_ERR_LAUNCH;
  }
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
  const size_t nb = size_t(s->rows) * (e->tas.L - e->tas.L / 2) * 4;
  s->n = s->k = 0, s->npend = 0, s->cur = 0, s->done = s->failed = false;
  if (e->dry) {
    memcpy(s->carry, s->carry0, nb);
  } else if (hipMemcpyAsync(s->carry, s->carry0, nb, hipMemcpyDeviceToDevice, e->stream) != hipSuccess) {
    set_err("ws_engine_stream_reset: device copy failed");
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

void free_stream(ws_stream* s) {
  if (s->state) {
    if (s->e->dry)
      free(s->state);
    else
      (void)hipFree(s->state);
  }
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

// extra_floats > 0: the state allocation gets one more slot of that many floats, returned in *extra, and the stream takes
// and returns DEVICE buffers (stream_push_impl / stream_flush_impl): the inner stream of a rate stream (rate.cc)
int wsrt::stream_open_impl(ws_engine* e, int rows, const void* enroll, int enroll_kind, int enroll_len, int max_chunk_frames,
                           unsigned flags, size_t extra_floats, ws_stream** out, float** extra) {
  int rc = check_engine(e, "ws_engine_stream_open");
  if (rc != WS_OK) return rc;
  if (out) *out = nullptr;
  if (!tas_streamable(e)) return refuse_not_streamable(e, "ws_engine_stream_open");
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
  const TasNet& t = e->tas;
  const int L = t.L, s = L / 2, H = t.H, B = t.B, G = max_chunk_frames;
  if ((long long)rows * G * 3 * t.N > 0x7fffffffLL || (long long)rows * ((long long)(t.P - 1) * (1 << (t.X - 1)) + G) * H > 0x7fffffffLL) {
    set_err("ws_engine_stream_open: rows=%d with max_chunk_frames=%d reaches 2^31 elements in one buffer", rows, G);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  ws_stream* st = new ws_stream();
  st->e = e, st->rows = rows, st->G = G, st->pcap = (G * s + kLmax + 3) / 4 * 4;
  st->block_kernel = (flags & WS_STREAM_BLOCK_KERNEL) != 0;
  // ---- the state block: rings, carry (+ its reset image), two pending buffers, embedding, row biases; 256-byte slots ----
  const int nblocks = t.R * t.X;
  std::vector<size_t> off;
  size_t total = 0;
  auto slot = [&](size_t nfloats) {
    off.push_back(total);
    total += Arena::round_up(nfloats * 4);
  };
  for (int r = 0; r < t.R; ++r)
    for (int k = 0; k < t.X; ++k) slot(size_t(rows) * ((size_t)(t.P - 1) * (1 << k) + G) * H);
  slot(size_t(rows) * (L - s));
  slot(size_t(rows) * (L - s));
  slot(size_t(rows) * st->pcap);
  slot(size_t(rows) * st->pcap);
  slot(size_t(rows) * e->E);
  for (int r = 0; r < t.R; ++r) slot(size_t(rows) * H);
  if (extra_floats) slot(extra_floats);
  st->dev_io = extra_floats != 0;
  st->state_bytes = total;
  if (e->dry) {
    st->state = static_cast<char*>(malloc(total));
  } else if (hipMalloc(reinterpret_cast<void**>(&st->state), total) != hipSuccess) {
    st->state = nullptr;
  }
  if (!st->state) {
    set_err("ws_engine_stream_open: device allocation of %zu bytes failed", total);
    free_stream(st);
    return WS_ERR_LAUNCH;
  }
  if (e->work.poison && !e->dry) {      // WS_ENGINE_POISON (tests): state no launch has written reads as NaN
    (void)hipDeviceSynchronize();
    (void)hipMemset(st->state, 0xFF, total);
    (void)hipDeviceSynchronize();
  }
  auto at = [&](size_t i) { return reinterpret_cast<float*>(st->state + off[i]); };
  size_t si = nblocks;
  st->carry = at(si++), st->carry0 = at(si++), st->pend[0] = at(si++), st->pend[1] = at(si++), st->emb = at(si++);
  for (int r = 0; r < t.R; ++r) st->rb.push_back(at(si++));
  if (extra_floats) *extra = at(si++);
  // ---- weights, resolved once ----
  resolve_stream_weights(e, st);
  for (int r = 0; r < t.R; ++r)
    for (int k = 0; k < t.X; ++k) {
      StreamBlock& b = st->blocks[size_t(r) * t.X + k];
      b.cap = (t.P - 1) * b.dil + G, b.ring = at(size_t(r) * t.X + k), b.rb = k == 0 ? st->rb[r] : nullptr;
    }
  // ---- the speaker stage, once: embedding, SpeakerTransform, the stacks' row biases W_e e + b ----
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* d_emb = a.alloc(size_t(rows) * e->E);
  const float* embp = nullptr;
  rc = d_emb ? WS_OK : WS_ERR_LAUNCH;
  if (rc == WS_OK) rc = speaker_stage(e, enroll, enroll_kind, rows, enroll_len, enroll_len, nullptr, nullptr, d_emb);
  if (rc == WS_OK) rc = spk_transform(e, d_emb, rows, &embp);
  if (rc == WS_OK) {
    if (e->dry)
      memcpy(st->emb, embp, size_t(rows) * e->E * 4);
    else if (hipMemcpyAsync(st->emb, embp, size_t(rows) * e->E * 4, hipMemcpyDeviceToDevice, e->stream) != hipSuccess)
      rc = WS_ERR_LAUNCH;
  }
  for (int r = 0; rc == WS_OK && r < t.R; ++r) {
    const StreamBlock& b = st->blocks[size_t(r) * t.X];
    rc = linear(e, st->emb, rows, e->E, b.w1 + B, B + e->E, H, b.b1, 0, st->rb[r]);
  }
  if (rc == WS_OK) {                    // the reset image of the carry: the decoder bias
    const std::vector<float> c0(size_t(rows) * (L - s), e->host("decoder.decoder_1d_1.bias")[0]);
    rc = to_device(e, st->carry0, c0.data(), c0.size() * 4);
  }
  if (rc == WS_OK) rc = reset_state(st);
  if (rc == WS_OK) rc = sync_stream(e);
  a.release(mk);
  if (rc != WS_OK) {
    free_stream(st);
    return rc;
  }
  e->stream_state_bytes = static_cast<long long>(total);
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
  const long long total = st->n + n;
  const long long target = total >= kLmax ? (total - kLmax) / s + 1 : 0;
  const long long emit = (target - st->k) * s;
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
    // at most G s + 159 pending samples: a piece completes at most G frames, one group (and fewer than 160 stay pending)
    const int take = std::min(n - off, st->G * s + kLmax - 1 - st->npend);
    if ((rc = copy2d(e, st->pend[st->cur] + st->npend, size_t(st->pcap) * 4, chunk + off, size_t(chunk_pitch) * 4, size_t(take) * 4, R,
                     dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, "host-to-device copy")) != WS_OK)
      return rc;
    st->npend += take, off += take, st->n += take;
    while (st->npend >= kLmax) {
      const int Tc = std::min((st->npend - kLmax) / s + 1, st->G);
      if ((rc = run_group(st, Tc, est, est_pitch, col)) != WS_OK) return rc;
      col += Tc * s;
    }
  }
  if (!dev && (rc = sync_stream(e)) != WS_OK) return rc;     // the one host synchronisation of a push
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
  const long long target = (st->n - L) / s + 1;
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
  if ((rc = copy2d(e, est + col, size_t(est_pitch) * 4, st->carry, size_t(L - s) * 4, size_t(L - s) * 4, R,
                   dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, "device-to-host copy")) != WS_OK)
    return rc;
  if (!dev && (rc = sync_stream(e)) != WS_OK) return rc;
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
  return sync_stream(st->e);
}

WS_ENGINE_API void ws_engine_stream_close(ws_stream* st) {
  if (!st) return;
  if (st->e && !st->e->dry) {
    (void)hipSetDevice(st->e->device);
    (void)hipStreamSynchronize(st->e->stream);
  }
  free_stream(st);
}
