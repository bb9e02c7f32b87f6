// =================================================================================================================
// Live windows (ws_engine_live_*): the windows of ws_engine_separate_long, run as their samples arrive.
// Window w starts at w H and is complete once w H + S samples exist; a sample is final once every window that can cover it
// has run.  With N samples pushed, Wr(N) = N < S ? 0 : 1 + (N - S) / H windows have run and E(N) = max(Wr - 1, 0) H samples
// are out: every later window, the end-aligned one of a flush included, starts behind the newest window's start.  Any
// container is taken -- nothing of this needs a causal model -- at the price of S .. S + H samples of latency.
//   * the speaker stage runs once, at open; the K embeddings stay in the handle's state;
//   * the state is ONE device allocation made at open: a ring [K][cap][S] of window estimates (window w in slot w % cap,
//     cap = g_max + 3), the ring of TF-GridNet's per-window factors, the staging span of a group's samples, the group's
//     rows and the embeddings.  It depends on (K, S, O, max_rows) only; the pending samples (fewer than S + H between two
//     pushes) live on the host;
//   * a group is up to g_max = max(1, max_rows / K) new consecutive windows, cut where the ring wraps: the regular layout
//     of a span of (g - 1) H + S samples, so ws_window_rows gathers it and the architecture's rectangular plan runs it;
//     ws_xfade_stream_fwd then emits what the group made final.  Transient activations come from the engine's work arena
//     under an ArenaScope; the arena is never reset here, and nothing of it is held between two calls.
// =================================================================================================================
#include <deque>

#include "engine_internal.h"

using namespace wsrt;

struct ws_live {
  ws_engine* e = nullptr;
  int K = 0, S = 0, O = 0, H = 0, max_rows = 0, g_max = 0, cap = 0;
  char* state = nullptr;
  size_t state_bytes = 0;
  float *ring = nullptr, *scale_ring = nullptr, *span = nullptr, *rows = nullptr, *inv = nullptr, *emb = nullptr, *emb_rows = nullptr;
  int emb_rows_g = 0;                   // the g whose table emb_rows holds: row k g + w = embedding k
  std::vector<float> emb_host;          // [K][E]
  std::vector<float> pend;              // the samples from `base` on
  long long base = 0, N = 0, Wr = 0, E = 0;     // samples pushed, windows run, samples emitted
  bool done = false, failed = false;
  std::deque<std::vector<float>> hold;  // host sources of the call's asynchronous uploads, alive until its synchronisation
};

namespace {

constexpr const char* kWho = "ws_engine_live";

int check_live(const ws_live* s, const char* who) {
  if (!s || !s->e) {
    set_err("%s: null handle", who);
    return WS_ERR_INVALID;
  }
  if (s->failed) {
    set_err("%s: an earlier call on this handle failed half way; call ws_engine_live_reset", who);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

void free_live(ws_live* s) {
  if (s->state) {
    if (s->e->dry)
      free(s->state);
    else
      (void)hipFree(s->state);
  }
  delete s;
}

// g consecutive windows of L samples, the first with index w0, from the host span x [(g - 1) H + L] (g = 1 with L < S: the
// one short window of a flush): upload, gather, the rectangular plan, estimates into ring slots w0 % cap .. (no wrap inside)
int run_group(ws_live* s, const float* x, long long w0, int g, int L) {
  ws_engine* e = s->e;
  Arena& a = e->work;
  const int K = s->K, S = s->S, H = s->H, R = K * g, slot0 = static_cast<int>(w0 % s->cap), n_span = (g - 1) * H + L;
  int rc;
  if ((rc = copy_async(e, kWho, "host-to-device copy", s->span, x, size_t(n_span) * 4, hipMemcpyHostToDevice)) != WS_OK) return rc;
  const float* d_inv = nullptr;
  if (e->arch == 3) {      // TF-GridNet: every window scaled by its own standard deviation, its estimate back (longform.cc)
    s->hold.emplace_back(2 * size_t(g));
    std::vector<float>& tab = s->hold.back();
    for (int w = 0; w < g; ++w) {
      row_std_scale(x + size_t(w) * H, L, &tab[size_t(g) + w], nullptr);
      tab[w] = 1.0f / tab[size_t(g) + w];
    }
    if ((rc = copy_async(e, kWho, "host-to-device copy", s->inv, tab.data(), size_t(g) * 4, hipMemcpyHostToDevice)) != WS_OK ||
        (rc = copy_async(e, kWho, "host-to-device copy", s->scale_ring + slot0, tab.data() + g, size_t(g) * 4, hipMemcpyHostToDevice)) != WS_OK)
      return rc;
    d_inv = s->inv;
  }
  WS_RUN(e, ws_window_rows(s->span, n_span, g, S, H, K, d_inv, s->rows, e->stream));
  const float* d_emb = s->emb;          // g == 1: row k is embedding k
  if (g > 1) {
    if (s->emb_rows_g != g) {
      s->hold.emplace_back(size_t(R) * e->E);
      std::vector<float>& t = s->hold.back();
      for (int r = 0; r < R; ++r) memcpy(t.data() + size_t(r) * e->E, s->emb_host.data() + size_t(r / g) * e->E, size_t(e->E) * 4);
      if ((rc = copy_async(e, kWho, "host-to-device copy", s->emb_rows, t.data(), t.size() * 4, hipMemcpyHostToDevice)) != WS_OK) return rc;
      s->emb_rows_g = g;
    }
    d_emb = s->emb_rows;
  }
  // row (k, w) belongs at ring[k][slot0 + w]: a forward whose rows share one k writes there itself
  const bool direct = K == 1 || s->max_rows == 1;
  float* d_y = nullptr;
  if (!direct) {
    d_y = a.alloc(size_t(R) * L);
    WS_PTR(d_y);
  }
  const int G = R < s->max_rows ? R : s->max_rows;
  const Arena::Mark mk = a.mark();
  for (int r0 = 0; r0 < R; r0 += G) {
    const int Gn = R - r0 < G ? R - r0 : G;
    a.release(mk);
    const float* in = s->rows + size_t(r0) * L;
    float* out = direct ? s->ring + (size_t(r0 / g) * s->cap + slot0 + r0 % g) * S : d_y + size_t(r0) * L;
    rc = e->arch == 1   ? tasnet_device(e, in, Gn, L, d_emb + size_t(r0) * e->E, nullptr, 0, out)
         : e->arch == 2 ? dpccn_device(e, in, Gn, L, d_emb + size_t(r0) * e->E, out)
         : e->arch == 3 ? gridnet_device(e, in, Gn, L, d_emb + size_t(r0) * e->E, out)
                        : separate_device(e, in, Gn, L, d_emb + size_t(r0) * e->E, out);
    if (rc != WS_OK) return rc;
  }
  a.release(mk);
  if (!direct) {
    ++e->n_launches;
    if ((rc = copy_async(e, kWho, "ring copy", s->ring + size_t(slot0) * S, size_t(s->cap) * S * 4, d_y, size_t(g) * L * 4, size_t(g) * L * 4,
                         K, hipMemcpyDeviceToDevice)) != WS_OK)
      return rc;
  }
  ++e->live_groups;
  return WS_OK;
}

// what the windows run make final, or at a flush the rest: positions [s->E, to) into d_out [K][ld] at column col
int emit(ws_live* s, long long to, bool final, long long W, float* d_out, long long ld, long long col) {
  ws_engine* e = s->e;
  WS_RUN(e, ws_xfade_stream_fwd(s->ring, s->K, s->cap, s->S, s->O, e->arch == 3 ? s->scale_ring : nullptr, s->E, to - s->E, s->Wr,
                                final ? 1 : 0, W, s->N, d_out + col, ld, e->stream));
  s->E = to;
  return WS_OK;
}

int finish(ws_live* s, float* est, int est_cap, const float* d_out, long long emitted) {
  ws_engine* e = s->e;
  int rc;
  ++e->n_launches;
  if ((rc = copy_async(e, kWho, "device-to-host copy", est, size_t(est_cap) * 4, d_out, size_t(emitted) * 4, size_t(emitted) * 4, s->K,
                       hipMemcpyDeviceToHost)) != WS_OK)
    return rc;
  unsigned timed_out = 0;                // did a cluster recurrence time out (note_cluster_status)?  read in the same wait
  if (e->cl_status && (rc = copy_async(e, kWho, "device-to-host copy", &timed_out, e->cl_status, 4, hipMemcpyDeviceToHost)) != WS_OK) return rc;
  if ((rc = sync_stream(e, kWho)) != WS_OK) return rc;       // the one host synchronisation of the call
  if (timed_out) {
    ++e->cluster_fallbacks;
    if ((rc = zero_device(e, e->cl_status, 4)) != WS_OK) return rc;
  }
  s->hold.clear();
  e->live_windows = s->Wr;
  return WS_OK;
}

void reset_counters(ws_live* s) {
  s->pend.clear();
  s->base = s->N = s->Wr = s->E = 0;
  s->done = s->failed = false;
  s->hold.clear();
}

}  // namespace

WS_ENGINE_API int ws_engine_live_open(ws_engine* e, int K, const void* enroll, int enroll_kind, int enroll_len, const int* enroll_lengths,
                                      int window, int overlap, int max_rows, ws_live** out) {
  const char* who = "ws_engine_live_open";
  int rc = check_engine(e, who);
  if (rc != WS_OK) return rc;
  if (out) *out = nullptr;
  if (!enroll || !out || K < 1) {
    set_err("ws_engine_live_open: bad arguments (K=%d >= 1, enroll %s, out %s)", K, enroll ? "given" : "NULL", out ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  // exactly what ws_engine_separate_long demands, with its messages
  if ((rc = long_check_window(e, window, overlap, max_rows)) != WS_OK) return rc;
  const int S = window, H = S - overlap, g_max = std::max(1, max_rows / K), cap = g_max + 3;
  const int G = K <= max_rows ? K * g_max : max_rows;
  int Te = enroll_len;
  std::vector<int> te_row;
  if ((rc = long_check_group(e, G, S, K, enroll_kind, enroll_len, enroll_lengths, &Te, &te_row)) != WS_OK) return rc;
  if ((long long)(g_max - 1) * H + S > 0x7fffffffLL || (long long)K * g_max * S > 0x7fffffffLL) {
    set_err("ws_engine_live_open: a group of %d windows of %d samples for %d speakers: more samples than an int holds", g_max, S, K);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  ws_live* s = new ws_live();
  s->e = e, s->K = K, s->S = S, s->O = overlap, s->H = H, s->max_rows = max_rows, s->g_max = g_max, s->cap = cap;
  const size_t parts[7] = {size_t(K) * cap * S, size_t(cap),        size_t(g_max - 1) * H + S,     size_t(K) * g_max * S,
                           size_t(g_max),       size_t(K) * e->E,   size_t(K) * g_max * e->E};
  size_t off[7], total = 0;
  for (int i = 0; i < 7; ++i) off[i] = total, total += Arena::round_up(parts[i] * 4);
  s->state_bytes = total;
  if (e->dry) {
    s->state = static_cast<char*>(malloc(total));
  } else if (hipMalloc(reinterpret_cast<void**>(&s->state), total) != hipSuccess) {
    s->state = nullptr;
  }
  if (!s->state) {
    set_err("ws_engine_live_open: device allocation of %zu bytes failed", total);
    free_live(s);
    return WS_ERR_LAUNCH;
  }
  if (e->work.poison && !e->dry) {      // WS_ENGINE_POISON (tests): state no launch has written reads as NaN
    (void)hipDeviceSynchronize();
    (void)hipMemset(s->state, 0xFF, total);
    (void)hipDeviceSynchronize();
  }
  float** at[7] = {&s->ring, &s->scale_ring, &s->span, &s->rows, &s->inv, &s->emb, &s->emb_rows};
  for (int i = 0; i < 7; ++i) *at[i] = reinterpret_cast<float*>(s->state + off[i]);
  s->emb_host.assign(size_t(K) * e->E, 0.f);
  {
    ArenaScope scope(e->work);           // the speaker stage, once
    rc = speaker_stage(e, enroll, enroll_kind, K, enroll_len, Te, enroll_lengths, te_row.data(), s->emb);
    if (rc == WS_OK) rc = to_host(e, s->emb_host.data(), s->emb, s->emb_host.size() * 4);
  }
  if (rc != WS_OK) {
    free_live(s);
    return rc;
  }
  e->live_state_bytes = static_cast<long long>(s->state_bytes);
  e->live_windows = e->live_groups = 0;
  *out = s;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_live_push(ws_live* s, const float* chunk, int n, float* est, int est_cap, int* n_out) {
  int rc = check_live(s, "ws_engine_live_push");
  if (rc != WS_OK) return rc;
  ws_engine* e = s->e;
  if (s->done) {
    set_err("ws_engine_live_push: the handle was flushed (call ws_engine_live_reset to start another recording)");
    return WS_ERR_INVALID;
  }
  if (!chunk || !n_out || n < 1) {
    set_err("ws_engine_live_push: bad arguments (n=%d >= 1, chunk %s, n_out %s)", n, chunk ? "given" : "NULL", n_out ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  const int S = s->S, H = s->H;
  const long long N_new = s->N + n, Wr_new = live_windows_run(N_new, S, H), E_new = live_emitted(Wr_new, H);
  const long long emitted = E_new - s->E;
  if (emitted > est_cap || (emitted > 0 && !est)) {
    set_err("ws_engine_live_push: this push emits %lld samples a row, est_cap is %d%s (WS_LIVE_PUSH_CAP(n, H) = %lld always suffices)",
            emitted, est_cap, est ? "" : ", est is NULL", (long long)WS_LIVE_PUSH_CAP((long long)n, H));
    return WS_ERR_INVALID;
  }
  e->live_groups = 0;
  s->pend.insert(s->pend.end(), chunk, chunk + n);
  s->N = N_new;
  if (Wr_new == s->Wr) {                // no window became complete: no launch, no synchronisation
    e->n_launches = 0;
    e->live_windows = s->Wr;
    *n_out = 0;
    return WS_OK;
  }
  s->failed = true;                     // until the push is complete
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  ArenaScope scope(e->work);
  float* d_out = e->work.alloc(size_t(s->K) * std::max<long long>(emitted, 1));
  WS_PTR(d_out);
  const long long E0 = s->E;
  while (s->Wr < Wr_new) {
    const long long w0 = s->Wr;
    const int g = live_cut(w0, Wr_new, s->g_max, s->cap);
    if ((rc = run_group(s, s->pend.data() + (w0 * H - s->base), w0, g, S)) != WS_OK) return rc;
    s->Wr += g;
    if ((rc = emit(s, (s->Wr - 1) * H, false, 0, d_out, emitted, s->E - E0)) != WS_OK) return rc;
  }
  if ((rc = finish(s, est, est_cap, d_out, emitted)) != WS_OK) return rc;
  // what a later window can still read starts at the newest window's start
  s->pend.erase(s->pend.begin(), s->pend.begin() + static_cast<ptrdiff_t>(s->E - s->base));
  s->base = s->E;
  s->failed = false;
  *n_out = static_cast<int>(emitted);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_live_flush(ws_live* s, float* est, int est_cap, int* n_out) {
  int rc = check_live(s, "ws_engine_live_flush");
  if (rc != WS_OK) return rc;
  ws_engine* e = s->e;
  if (s->done) {
    set_err("ws_engine_live_flush: the handle was flushed already (call ws_engine_live_reset)");
    return WS_ERR_INVALID;
  }
  const int S = s->S, H = s->H, K = s->K;
  const long long n = s->N, emitted = n - s->E;
  if (n < 1) {
    set_err("ws_engine_live_flush: nothing was pushed");
    return WS_ERR_INVALID;
  }
  if (!est || !n_out || emitted > est_cap) {
    set_err("ws_engine_live_flush: the flush emits %lld samples a row, est_cap is %d%s (WS_LIVE_FLUSH_CAP(S, O) = %d always suffices)",
            emitted, est_cap, est && n_out ? "" : ", est or n_out is NULL", WS_LIVE_FLUSH_CAP(S, s->O));
    return WS_ERR_INVALID;
  }
  // n < S: the whole recording is one short row, the W == 1 branch of ws_engine_separate_long, with the architecture's own
  // lower bound on T; refused before anything runs, so a later push goes on from here
  if (n < S && (rc = check_rows(e, true, K < s->max_rows ? K : s->max_rows, static_cast<int>(n))) != WS_OK) return rc;
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->live_groups = 0;
  e->n_launches = 0;
  s->failed = true;
  ArenaScope scope(e->work);
  float* d_out = e->work.alloc(size_t(K) * emitted);
  WS_PTR(d_out);
  long long W = s->Wr;
  if (n < S) {
    if ((rc = run_group(s, s->pend.data(), 0, 1, static_cast<int>(n))) != WS_OK) return rc;
    W = 1;
  } else if ((n - S) % H != 0) {        // the end-aligned last window, index W - 1
    if ((rc = run_group(s, s->pend.data() + (n - S - s->base), s->Wr, 1, S)) != WS_OK) return rc;
    W = s->Wr + 1;
  }
  s->Wr = W;
  if ((rc = emit(s, n, true, W, d_out, emitted, 0)) != WS_OK) return rc;
  if ((rc = finish(s, est, est_cap, d_out, emitted)) != WS_OK) return rc;
  s->failed = false;
  s->done = true;
  *n_out = static_cast<int>(emitted);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_live_reset(ws_live* s) {
  if (!s || !s->e) {
    set_err("ws_engine_live_reset: null handle");
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(s->e);
  if (turn.rc != WS_OK) return turn.rc;
  const int rc = sync_stream(s->e, kWho);       // a call that failed half way may have left work behind
  reset_counters(s);
  s->e->live_windows = s->e->live_groups = 0;
  return rc;
}

WS_ENGINE_API void ws_engine_live_close(ws_live* s) {
  if (!s) return;
  if (s->e && !s->e->dry) {
    (void)hipSetDevice(s->e->device);
    (void)hipStreamSynchronize(s->e->stream);
  }
  free_live(s);
}
