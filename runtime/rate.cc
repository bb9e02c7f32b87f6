// =================================================================================================================
// Audio at the caller's sample rate (include/wesep_engine.h, "Sample rates"): the device resampler of wesep_hip.h
// (ws_resample_fwd / ws_resample_stream_fwd) in front of and behind what the engine already does.
//   ws_engine_resample       host rows in, host rows out: one upload, one launch, one download
//   ws_engine_separate_rate  resample the mixture (and a waveform enrollment) to the container's rate, ws_engine_separate as it
//                            is, resample the estimate back and crop -- all four architectures
//   ws_engine_rate_stream_*  a causal cLN Conv-TasNet stream whose pushes carry and return samples at the caller's rate:
//                            chunk H2D -> resampler A -> the solo stream of stream.cc on device buffers -> resampler B -> D2H,
//                            one host synchronisation per push.  The resamplers' histories and staging buffers are one more
//                            slot of the stream's ONE state allocation.
// Tap tables are made by ws_resample_taps (the one place) and kept on the device per (rate_in, rate_out).
// The emission rule -- Geom, rs_len, rs_emitted, plan_step, plain_emitted, rate_push_cap -- is engine_internal.h's, shared with
// the rate pool (rate_pool.cc); copies and the synchronisation are its copy_async / sync_stream.
// =================================================================================================================
#include <memory>

#include "engine_internal.h"

using namespace wsrt;

namespace {

// the kernel's limits, by name, before any launch
int rate_geom(const char* who, int rate_in, int rate_out, Geom* g) {
  if (ws_resample_geom(rate_in, rate_out, &g->U, &g->D, &g->w, &g->K) != WS_OK) {
    set_err("%s: %s", who, ws_last_error());
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

int rate_taps(ws_engine* e, int rate_in, int rate_out, const Geom& g, const float** out) {
  auto it = e->rs_taps.find({rate_in, rate_out});
  if (it == e->rs_taps.end()) {
    std::vector<float> t(size_t(g.U) * g.K);
    if (ws_resample_taps(rate_in, rate_out, t.data()) != WS_OK) {
      set_err("ws_engine_resample: %s", ws_last_error());
      return WS_ERR_INVALID;
    }
    const float* d = upload(e, e->persist, t.data(), t.size());
    WS_PTR(d);
    it = e->rs_taps.emplace(std::make_pair(rate_in, rate_out), d).first;
  }
  *out = it->second;
  return WS_OK;
}

// y [R][n_out] (host) = x [R][n] (host) at the other rate; the caller holds the turn and adds up the launches
int resample_rows(ws_engine* e, const float* x, int R, int n, int rate_in, int rate_out, const Geom& g, float* y) {
  const long long n_out = rs_len(g, n);
  const float* taps = nullptr;
  int rc = rate_taps(e, rate_in, rate_out, g, &taps);
  if (rc != WS_OK) return rc;
  ArenaScope scope(e->work);      // the two transient buffers go back to the arena on every path
  float* dx = e->work.alloc(size_t(R) * n);
  float* dy = e->work.alloc(size_t(R) * n_out);
  WS_PTR(dx && dy);
  if ((rc = to_device(e, dx, x, size_t(R) * n * 4)) != WS_OK) return rc;
  WS_RUN(e, ws_resample_fwd(dx, n, R, n, rate_in, rate_out, taps, dy, n_out, e->stream));
  return to_host(e, y, dy, size_t(R) * n_out * 4);
}

int check_resample_sizes(const char* who, const Geom& g, int R, int n) {
  if (R < 1 || R > 65535 || n < 1 || rs_len(g, n) + g.K + g.U >= 0x7fffffffLL || (long long)R * std::max<long long>(n, rs_len(g, n)) >= (1LL << 40)) {
    set_err("%s: bad sizes (R=%d in [1, 65535], n=%d >= 1, %lld samples a row after the conversion)", who, R, n, rs_len(g, n));
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

}  // namespace

int wsrt::resample_host_rows(ws_engine* e, const char* who, const float* x, int R, int n, int rate_in, int rate_out, std::vector<float>* y,
                             int* n_out) {
  Geom g;
  int rc;
  if ((rc = rate_geom(who, rate_in, rate_out, &g)) != WS_OK || (rc = check_resample_sizes(who, g, R, n)) != WS_OK) return rc;
  *n_out = static_cast<int>(rs_len(g, n));
  y->resize(size_t(R) * *n_out);
  return resample_rows(e, x, R, n, rate_in, rate_out, g, y->data());
}

WS_ENGINE_API int ws_engine_resample(ws_engine* e, const float* x, int R, int n, int rate_in, int rate_out, float* y, int y_cap,
                                     int* n_out) {
  int rc = check_engine(e, "ws_engine_resample");
  if (rc != WS_OK) return rc;
  if (!x || !y || !n_out) {
    set_err("ws_engine_resample: x, y or n_out is NULL");
    return WS_ERR_INVALID;
  }
  Geom g;
  if ((rc = rate_geom("ws_engine_resample", rate_in, rate_out, &g)) != WS_OK) return rc;
  if ((rc = check_resample_sizes("ws_engine_resample", g, R, n)) != WS_OK) return rc;
  if (rs_len(g, n) > y_cap) {
    set_err("ws_engine_resample: %d samples at %d Hz are %lld samples a row at %d Hz, y_cap is %d", n, rate_in, rs_len(g, n), rate_out,
            y_cap);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  if ((rc = resample_rows(e, x, R, n, rate_in, rate_out, g, y)) != WS_OK) return rc;
  *n_out = static_cast<int>(rs_len(g, n));
  return WS_OK;
}

WS_ENGINE_API int ws_engine_separate_rate(ws_engine* e, const float* mix, int R, int T, int sample_rate, const void* enroll,
                                          int enroll_kind, int enroll_len, int enroll_rate, float* est) {
  int rc = check_engine(e, "ws_engine_separate_rate");
  if (rc != WS_OK) return rc;
  const bool mix_rs = sample_rate != e->sr;
  const bool enr_rs = enroll_rate != 0 && enroll_rate != e->sr;
  if (enr_rs && enroll_kind != WS_ENROLL_WAVE) {
    set_err("ws_engine_separate_rate: enroll_rate=%d with enrollment kind %d: only a waveform enrollment (WS_ENROLL_WAVE) has a sample "
            "rate; pass 0 or the container's %d", enroll_rate, enroll_kind, e->sr);
    return WS_ERR_INVALID;
  }
  if (!mix_rs && !enr_rs) return ws_engine_separate(e, mix, R, T, enroll, enroll_kind, enroll_len, est);
  Geom ga, gb, ge;
  if (mix_rs && ((rc = rate_geom("ws_engine_separate_rate", sample_rate, e->sr, &ga)) != WS_OK ||
                 (rc = rate_geom("ws_engine_separate_rate", e->sr, sample_rate, &gb)) != WS_OK))
    return rc;
  if (enr_rs && (rc = rate_geom("ws_engine_separate_rate", enroll_rate, e->sr, &ge)) != WS_OK) return rc;
  if (!mix || !enroll || !est || R < 1 || T < 1 || (enr_rs && enroll_len < 1)) {
    set_err("ws_engine_separate_rate: bad arguments (R=%d, T=%d, enroll_len=%d; mix, enroll and est given)", R, T, enroll_len);
    return WS_ERR_INVALID;
  }
  if (mix_rs && (rc = check_resample_sizes("ws_engine_separate_rate", ga, R, T)) != WS_OK) return rc;
  if (enr_rs && (rc = check_resample_sizes("ws_engine_separate_rate", ge, R, enroll_len)) != WS_OK) return rc;
  const int Tm = mix_rs ? static_cast<int>(rs_len(ga, T)) : T;
  const int len_m = enr_rs ? static_cast<int>(rs_len(ge, enroll_len)) : enroll_len;
  // the architecture's own demands on the rectangle at the container's rate, with its own message
  if ((rc = check_rows(e, true, R, Tm)) != WS_OK) return rc;
  int Te = len_m;
  std::vector<int> te_row;
  if ((rc = check_enroll(e, R, enroll_kind, len_m, nullptr, &Te, &te_row)) != WS_OK) return rc;
  // ONE turn over the three steps (ws_engine_separate's own turn nests in it): nothing of another thread runs between them,
  // and the launch figures that are added up are this call's
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  long long launches = 0;
  std::vector<float> mix_m, enr_m, est_m(mix_rs ? size_t(R) * Tm : 0);
  {
    e->n_launches = 0;
    if (mix_rs) {
      mix_m.resize(size_t(R) * Tm);
      if ((rc = resample_rows(e, mix, R, T, sample_rate, e->sr, ga, mix_m.data())) != WS_OK) return rc;
    }
    if (enr_rs) {
      enr_m.resize(size_t(R) * len_m);
      if ((rc = resample_rows(e, static_cast<const float*>(enroll), R, enroll_len, enroll_rate, e->sr, ge, enr_m.data())) != WS_OK)
        return rc;
    }
    launches = e->n_launches;
  }
  rc = ws_engine_separate(e, mix_rs ? mix_m.data() : mix, R, Tm, enr_rs ? enr_m.data() : enroll, enroll_kind, len_m,
                          mix_rs ? est_m.data() : est);
  if (rc != WS_OK) return rc;
  launches += e->n_launches;
  if (mix_rs) {
    e->n_launches = 0;
    const long long n_back = rs_len(gb, Tm);        // >= T: Tm >= U T / D
    std::vector<float> back(size_t(R) * n_back);
    if ((rc = resample_rows(e, est_m.data(), R, Tm, e->sr, sample_rate, gb, back.data())) != WS_OK) return rc;
    launches += e->n_launches;
    if (!e->dry)
      for (int r = 0; r < R; ++r) memcpy(est + size_t(r) * T, back.data() + size_t(r) * n_back, size_t(T) * 4);
  }
  e->n_launches = launches;
  return WS_OK;
}

// ---- the rate stream ---------------------------------------------------------------------------------------------------
namespace {

struct Resampler {           // one direction: its geometry, table, two buffers [rows][ld] used in turn, and the host's counters
  Geom g;
  int rate_in = 0, rate_out = 0, ld = 0, cur = 0, h = 0;
  const float* taps = nullptr;
  float* buf[2] = {nullptr, nullptr};
  long long n = 0, groups = 0;       // samples taken, groups of U outputs returned
  void reset() { cur = h = 0, n = groups = 0; }
};

}  // namespace

struct ws_rate_stream {
  ws_engine* e = nullptr;
  ws_stream* inner = nullptr;
  bool plain = false;                // sample_rate is the container's: the calls ARE the plain stream's
  int rows = 0, sample_rate = 0, max_push = 0;
  Resampler A, B;
  float *a_out = nullptr, *b_out = nullptr;
  int a_cap = 0, m_cap = 0, b_cap = 0;   // floats a row of a_out, of what the inner stream hands B in one step, of b_out
  long long n = 0, returned = 0;     // samples pushed and returned, at sample_rate
  bool done = false, failed = false;
};

namespace {

// One step of a resampler: `n_new` samples were appended behind its history (the caller wrote them to buf[cur] + h); the
// outputs that became final (all the rest at a flush) go to y [rows][ldy]; the launch also moves the new history to the other
// buffer.  Nothing runs when nothing arrived and nothing is owed.
int rs_step(ws_rate_stream* s, Resampler& r, int n_new, bool final, float* y, long long ldy, int* n_out) {
  ws_engine* e = s->e;
  const Step p = plan_step(r.g, r.n, r.groups, r.h, n_new, final);
  *n_out = p.n_out;
  r.n += n_new;
  if (p.n_valid == 0 || (n_new == 0 && !final)) return WS_OK;
  WS_RUN(e, ws_resample_stream_fwd(r.buf[r.cur], r.ld, s->rows, r.rate_in, r.rate_out, r.taps, p.lead, p.n_valid, final ? 1 : 0, 0, p.n_out,
                                   p.n_out ? y : nullptr, ldy, p.hist_from, p.hist_len, p.hist_len ? r.buf[1 - r.cur] : nullptr, r.ld,
                                   e->stream));
  if (!final) r.cur ^= 1, r.h = p.hist_len, r.groups = p.g_new;
  return WS_OK;
}

constexpr const char* kWho = "ws_engine_rate_stream";
constexpr const char* kCopy = "a copy between host and device";

int check_rate_stream(const ws_rate_stream* s, const char* who) {
  if (!s || !s->e || !s->inner) {
    set_err("%s: null stream", who);
    return WS_ERR_INVALID;
  }
  if (s->failed) {
    set_err("%s: an earlier call on this stream failed half way; call ws_engine_rate_stream_reset", who);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

// B's part of a step: m samples of the inner stream arrived behind B's history; B's outputs go to the host at column *col of
// est (row pitch `pitch`), cropped to `pitch` samples in all
int b_step(ws_rate_stream* s, int m, bool final, float* est, long long pitch, long long* col) {
  int nb = 0, rc;
  if ((rc = rs_step(s, s->B, m, final, s->b_out, s->b_cap, &nb)) != WS_OK) return rc;
  const long long take = std::min<long long>(nb, pitch - *col);
  if ((rc = copy_async(s->e, kWho, kCopy, est + *col, size_t(pitch) * 4, s->b_out, size_t(s->b_cap) * 4, size_t(take) * 4, s->rows,
                       hipMemcpyDeviceToHost)) != WS_OK)
    return rc;
  *col += take;
  return WS_OK;
}

}  // namespace

WS_ENGINE_API int ws_engine_rate_stream_open(ws_engine* e, int rows, const void* enroll, int enroll_kind, int enroll_len,
                                             int enroll_rate, int max_chunk_frames, unsigned flags, int sample_rate, int max_push,
                                             ws_rate_stream** out) {
  int rc = check_engine(e, "ws_engine_rate_stream_open");
  if (rc != WS_OK) return rc;
  if (!out) {
    set_err("ws_engine_rate_stream_open: out is NULL");
    return WS_ERR_INVALID;
  }
  *out = nullptr;
  if (!tas_streamable(e)) return refuse_not_streamable(e, "ws_engine_rate_stream_open");
  const bool enr_rs = enroll_rate != 0 && enroll_rate != e->sr;
  if (enr_rs && enroll_kind != WS_ENROLL_WAVE) {
    set_err("ws_engine_rate_stream_open: enroll_rate=%d with enrollment kind %d: only a waveform enrollment (WS_ENROLL_WAVE) has a "
            "sample rate; pass 0 or the container's %d", enroll_rate, enroll_kind, e->sr);
    return WS_ERR_INVALID;
  }
  if (max_push < 1 || max_push > (1 << 24) || rows < 1) {
    set_err("ws_engine_rate_stream_open: bad arguments (rows=%d, max_push=%d in [1, 2^24])", rows, max_push);
    return WS_ERR_INVALID;
  }
  std::unique_ptr<ws_rate_stream> s(new ws_rate_stream());
  s->e = e, s->rows = rows, s->sample_rate = sample_rate, s->max_push = max_push, s->plain = sample_rate == e->sr;
  Geom ge;
  if (!s->plain && ((rc = rate_geom("ws_engine_rate_stream_open", sample_rate, e->sr, &s->A.g)) != WS_OK ||
                    (rc = rate_geom("ws_engine_rate_stream_open", e->sr, sample_rate, &s->B.g)) != WS_OK))
    return rc;
  if (enr_rs && ((rc = rate_geom("ws_engine_rate_stream_open", enroll_rate, e->sr, &ge)) != WS_OK ||
                 (rc = check_resample_sizes("ws_engine_rate_stream_open", ge, rows, enroll_len)) != WS_OK))
    return rc;
  if (enr_rs && !enroll) {
    set_err("ws_engine_rate_stream_open: enroll is NULL");
    return WS_ERR_INVALID;
  }
  // the enrollment at the container's rate
  std::vector<float> enr_m;
  int len_m = enroll_len;
  if (enr_rs) {
    len_m = static_cast<int>(rs_len(ge, enroll_len));
    if ((rc = tasnet_check_enroll(e, enroll_kind, len_m)) != WS_OK) return rc;
    ForwardTurn turn(e);
    if (turn.rc != WS_OK) return turn.rc;
    e->n_launches = 0;
    enr_m.resize(size_t(rows) * len_m);
    if ((rc = resample_rows(e, static_cast<const float*>(enroll), rows, enroll_len, enroll_rate, e->sr, ge, enr_m.data())) != WS_OK)
      return rc;
    enroll = enr_m.data();
  }
  size_t extra = 0;
  const int L = e->tas.L, hop = L / 2;
  if (!s->plain) {
    Resampler &A = s->A, &B = s->B;
    A.rate_in = sample_rate, A.rate_out = e->sr, B.rate_in = e->sr, B.rate_out = sample_rate;
    A.ld = (A.g.K - 1 + max_push + 3) / 4 * 4;
    s->a_cap = static_cast<int>(((long long)(A.g.K - 1 + max_push) / A.g.D + 1) * A.g.U + 3) / 4 * 4;
    s->m_cap = std::max((s->a_cap / hop + 1) * hop, WS_STREAM_FLUSH_CAP);
    B.ld = (B.g.K - 1 + s->m_cap + 3) / 4 * 4;
    s->b_cap = static_cast<int>(((long long)(B.g.K - 1 + s->m_cap) / B.g.D + 1) * B.g.U + 3) / 4 * 4;
    extra = size_t(rows) * (2 * size_t(A.ld) + 2 * size_t(B.ld) + s->a_cap + s->b_cap);
    if (extra >= (size_t(1) << 31)) {
      set_err("ws_engine_rate_stream_open: rows=%d with max_push=%d reaches 2^31 elements of resampler state", rows, max_push);
      return WS_ERR_INVALID;
    }
    ForwardTurn turn(e);              // the tables are made and uploaded on first use: under the turn, as everywhere
    if (turn.rc != WS_OK) return turn.rc;
    if ((rc = rate_taps(e, A.rate_in, A.rate_out, A.g, &A.taps)) != WS_OK || (rc = rate_taps(e, B.rate_in, B.rate_out, B.g, &B.taps)) != WS_OK)
      return rc;
  }
  float* x = nullptr;
  if ((rc = stream_open_impl(e, rows, enroll, enroll_kind, len_m, max_chunk_frames, flags, extra, &s->inner, &x)) != WS_OK) return rc;
  if (!s->plain) {
    s->A.buf[0] = x, x += size_t(rows) * s->A.ld;
    s->A.buf[1] = x, x += size_t(rows) * s->A.ld;
    s->B.buf[0] = x, x += size_t(rows) * s->B.ld;
    s->B.buf[1] = x, x += size_t(rows) * s->B.ld;
    s->a_out = x, x += size_t(rows) * s->a_cap;
    s->b_out = x;
  }
  *out = s.release();
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_stream_push_cap(const ws_rate_stream* s, int n) {
  if (!s || !s->e || n < 0) return -1;
  const int L = s->e->tas.L;
  if (s->plain) return n == 0 ? WS_STREAM_FLUSH_CAP : WS_STREAM_PUSH_CAP(n, L);
  return rate_push_cap(s->A.g, s->B.g, L, n);
}

WS_ENGINE_API int ws_engine_rate_stream_push(ws_rate_stream* s, const float* chunk, int n, float* est, int est_cap, int* n_out) {
  int rc = check_rate_stream(s, "ws_engine_rate_stream_push");
  if (rc != WS_OK) return rc;
  if (s->plain) return ws_engine_stream_push(s->inner, chunk, n, est, est_cap, n_out);
  ws_engine* e = s->e;
  if (s->done) {
    set_err("ws_engine_rate_stream_push: the stream was flushed (call ws_engine_rate_stream_reset to start another)");
    return WS_ERR_INVALID;
  }
  if (!chunk || !n_out || n < 1) {
    set_err("ws_engine_rate_stream_push: bad arguments (n=%d >= 1, chunk %s, n_out %s)", n, chunk ? "given" : "NULL", n_out ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  const int L = e->tas.L;
  // B's emission on the inner stream's emission on A's emission: known before anything runs
  const long long emit = rs_emitted(s->B.g, plain_emitted(rs_emitted(s->A.g, s->n + n), L)) - s->returned;
  if (emit > est_cap || (emit > 0 && !est)) {
    set_err("ws_engine_rate_stream_push: this push emits %lld samples a row, est_cap is %d (ws_engine_rate_stream_push_cap(s, n) = %d "
            "always suffices)", emit, est_cap, ws_engine_rate_stream_push_cap(s, n));
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  s->failed = true;
  long long col = 0;
  for (int off = 0; off < n;) {
    const int take = std::min(n - off, s->max_push);
    Resampler& A = s->A;
    if ((rc = copy_async(e, kWho, kCopy, A.buf[A.cur] + A.h, size_t(A.ld) * 4, chunk + off, size_t(n) * 4, size_t(take) * 4, s->rows,
                         hipMemcpyHostToDevice)) != WS_OK)
      return rc;
    off += take;
    int na = 0, m = 0;
    if ((rc = rs_step(s, A, take, false, s->a_out, s->a_cap, &na)) != WS_OK) return rc;
    if (na > 0) {
      Resampler& B = s->B;
      if ((rc = stream_push_impl(s->inner, s->a_out, s->a_cap, na, B.buf[B.cur] + B.h, B.ld, s->m_cap, &m)) != WS_OK) return rc;
    }
    if ((rc = b_step(s, m, false, est, emit, &col)) != WS_OK) return rc;
  }
  if ((rc = sync_stream(e, "ws_engine_rate_stream_push")) != WS_OK) return rc;      // the one host synchronisation of a push
  if (col != emit) {
    set_err("ws_engine_rate_stream_push: internal error: %lld samples were produced where the rule says %lld", col, emit);
    return WS_ERR_LAUNCH;
  }
  s->n += n, s->returned += emit;
  s->failed = false;
  *n_out = static_cast<int>(emit);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_stream_flush(ws_rate_stream* s, float* est, int est_cap, int* n_out) {
  int rc = check_rate_stream(s, "ws_engine_rate_stream_flush");
  if (rc != WS_OK) return rc;
  if (s->plain) return ws_engine_stream_flush(s->inner, est, est_cap, n_out);
  ws_engine* e = s->e;
  const int L = e->tas.L;
  if (s->done) {
    set_err("ws_engine_rate_stream_flush: the stream was flushed already (call ws_engine_rate_stream_reset)");
    return WS_ERR_INVALID;
  }
  const long long n_model = rs_len(s->A.g, s->n);
  if (n_model < L) {
    set_err("ws_engine_rate_stream_flush: %lld samples were pushed, %lld at the container's rate, fewer than the encoder window L = %d",
            s->n, n_model, L);
    return WS_ERR_INVALID;
  }
  // the composition's length, cropped so that the total is at most the number of samples pushed
  const long long total = std::min(s->n, rs_len(s->B.g, plain_total(n_model, L)));
  const long long emit = std::max<long long>(0, total - s->returned);
  if (!n_out || emit > est_cap || (emit > 0 && !est)) {
    set_err("ws_engine_rate_stream_flush: the flush emits %lld samples a row, est_cap is %d%s (ws_engine_rate_stream_push_cap(s, 0) = %d "
            "always suffices)", emit, est_cap, n_out ? "" : ", n_out is NULL", ws_engine_rate_stream_push_cap(s, 0));
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  s->failed = true;
  long long col = 0;
  int na = 0, m = 0;
  Resampler& B = s->B;
  if ((rc = rs_step(s, s->A, 0, true, s->a_out, s->a_cap, &na)) != WS_OK) return rc;       // A's flush
  if (na > 0) {                                                                             // the inner stream's rest ...
    if ((rc = stream_push_impl(s->inner, s->a_out, s->a_cap, na, B.buf[B.cur] + B.h, B.ld, s->m_cap, &m)) != WS_OK) return rc;
  }
  if ((rc = b_step(s, m, false, est, emit, &col)) != WS_OK) return rc;
  if ((rc = stream_flush_impl(s->inner, B.buf[B.cur] + B.h, B.ld, s->m_cap, &m)) != WS_OK) return rc;   // ... and flush
  if ((rc = b_step(s, m, false, est, emit, &col)) != WS_OK) return rc;
  if ((rc = b_step(s, 0, true, est, emit, &col)) != WS_OK) return rc;                       // B's flush, cropped
  if ((rc = sync_stream(e, "ws_engine_rate_stream_flush")) != WS_OK) return rc;
  if (col != emit) {
    set_err("ws_engine_rate_stream_flush: internal error: %lld samples were produced where the rule says %lld", col, emit);
    return WS_ERR_LAUNCH;
  }
  s->returned += emit;
  s->failed = false, s->done = true;
  *n_out = static_cast<int>(emit);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_stream_reset(ws_rate_stream* s) {
  if (!s || !s->e || !s->inner) {
    set_err("ws_engine_rate_stream_reset: null stream");
    return WS_ERR_INVALID;
  }
  const int rc = ws_engine_stream_reset(s->inner);
  if (rc != WS_OK) return rc;
  s->A.reset(), s->B.reset();
  s->n = s->returned = 0;
  s->done = s->failed = false;
  return WS_OK;
}

WS_ENGINE_API void ws_engine_rate_stream_close(ws_rate_stream* s) {
  if (!s) return;
  ws_engine_stream_close(s->inner);
  delete s;
}
