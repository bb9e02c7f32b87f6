// =================================================================================================================
// Rate tail pool (ws_engine_rate_tail_pool_*; DESIGN 7 "Rate tail pool" and 11b): the tail pool (tail_pool.cc) with a sample
// rate per slot.  A slot carries and returns audio at ITS caller's rate r; the separator runs at the container's rate r0.
// With A the r -> r0 filter and B the r0 -> r filter of the slot's rate:
//   * push appends CALLER-rate samples on the host.  N, the model-rate samples the recording has, is A's streaming emission
//     count, known on the host; the tail pool's rule (tail_pool.cc) applies to N unchanged;
//   * the window [max(0, N - S), N) is kept nowhere at the model's rate: ONE ws_window_resample_rows_fwd computes every row of
//     the tick from the caller-rate span that its taps cover, straight into the rows rectangle -- the bits of ws_resample_fwd on
//     the whole recording, so the pool carries no input-resampler state;
//   * ws_tail_emit_rows_fwd writes what the tick emits straight behind B's history of the same (slot, target); ONE
//     ws_resample_stream_rows_fwd runs B over all (slot, target) rows as streams, histories double-buffered on the device as
//     rate_pool.cc keeps them; its outputs go to one compact block, one copy to the host, ONE synchronisation;
//   * a flush runs the last window with A's final rule (N = ceil(U_A N_c / D_A), taps behind the end skipped), emits [E, N) and
//     ends B's stream in the same launch (final = 1 on `history | new`: the bits of B's step followed by B's flush); the
//     total is cropped so that a slot returns exactly the N_c samples it was given.
// A slot at the container's rate runs the identity table U = D = K = 1 through both filters: the plain tail pool's samples.
// The state is ONE device allocation made at open, a function of (slots, K, S, C, max_rows) and the worst listed geometry.
// =================================================================================================================
#include <deque>
#include <memory>

#include "engine_internal.h"

using namespace wsrt;

namespace {

struct RtRate {              // one accepted sample rate: caller -> container (a) and back (b); tables at state floats
  int rate = 0;
  Geom a, b;
  long long a_taps = 0, b_taps = 0;
};

struct RtSlot {
  enum State { kFree, kAttached, kDone } state = kFree;
  bool failed = false;                  // a tick or flush that named this slot ended half way
  bool fired = false;
  int flip = 0;                         // which of the two hold buffers the last firing wrote
  int ri = -1;                          // its rate, an index into ws_rate_tail_pool::rates
  std::vector<float> pend;              // caller-rate samples from sample c0 of the recording on
  std::vector<float> emb;               // [K][E], host copy of the slot's embeddings
  long long c0 = 0, Nc = 0;             // first kept and pushed samples, at the caller's rate
  long long F = 0, E = 0;               // N at the last firing and samples emitted, at the container's rate
  // B, the same counters for the slot's K targets: the buffer in use, its history, samples taken, groups returned
  int b_cur = 0, b_h = 0;
  long long b_n = 0, b_groups = 0;
  long long returned = 0;               // samples a target returned, at the caller's rate
};

// what one slot gives to one tick or flush: the window [N - L, N) of which m samples from local index p come out (the first h
// cross-faded with the hold) and c_new are held back; B takes the m samples (st) and returns n_ret of its n_out outputs
struct RtPart {
  int slot = 0, entry = 0, L = 0, p = 0, h = 0, m = 0, c_new = 0;
  bool final = false, window = true;
  long long N = 0;
  Step st;
  int n_ret = 0;
  long long out_off = 0;                // floats into B's compact block: [K][st.n_out]
};

}  // namespace

struct ws_rate_tail_pool {
  ws_engine* e = nullptr;
  int slots = 0, K = 0, S = 0, C = 0, warm = 0, max_rows = 0;
  std::vector<RtRate> rates;            // rates[0]: the container's own (identity)
  char* state = nullptr;
  size_t state_bytes = 0, stage_bytes = 0;
  // float offsets into the state of its parts: holds [slots][2][K][C], embeddings [slots][K][E], the staging block, the rows and
  // estimates rectangles [slots K][S], B's buffers [slots][K][2][b_ld], B's compact block [slots K][b_cap], the ramp [C], the taps
  long long hold_off = 0, emb_off = 0, stage_off = 0, rows_off = 0, y_off = 0, b_off = 0, bout_off = 0, ramp_off = 0, taps_off = 0;
  long long span_cap = 0, b_ld = 0, b_cap = 0;
  std::vector<RtSlot> sl;
  std::deque<std::vector<char>> keep;   // host sources of the call's asynchronous uploads, alive until its synchronisation
  std::vector<float> out_host;          // the call's estimates, one block
  long long forwards = 0, rows = 0;

  long long bbuf(int slot, int k, int which) const { return b_off + (((long long)slot * K + k) * 2 + which) * b_ld; }
};

namespace {

constexpr const char* kWho = "ws_engine_rate_tail_pool";

size_t up256(size_t b) { return Arena::round_up(b); }

int check_pool(const ws_rate_tail_pool* p, const char* who) {
  if (!p || !p->e) {
    set_err("%s: null pool", who);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

// attached, not flushed, not the slot of a call that failed half way
int check_slot(const ws_rate_tail_pool* p, const char* who, int id, int entry) {
  char where[48] = "";
  if (entry >= 0) snprintf(where, sizeof where, " (entry %d)", entry);
  if (id < 0 || id >= p->slots || p->sl[id].state == RtSlot::kFree)
    set_err("%s: slot %d%s is not attached (the pool has %d slots)", who, id, where, p->slots);
  else if (p->sl[id].failed)
    set_err("%s: slot %d%s took part in a call that failed half way; detach it", who, id, where);
  else if (p->sl[id].state == RtSlot::kDone)
    set_err("%s: slot %d%s was flushed (detach it, then attach the next recording)", who, id, where);
  else
    return WS_OK;
  return WS_ERR_INVALID;
}

void free_pool(ws_rate_tail_pool* p) {
  if (p->state) {
    if (p->e->dry)
      free(p->state);
    else
      (void)hipFree(p->state);
  }
  delete p;
}

std::string rates_text(const ws_rate_tail_pool* p) {
  std::string s;
  for (const RtRate& r : p->rates) s += (s.empty() ? "" : ", ") + std::to_string(r.rate);
  return s;
}

// est_cap that always suffices for a slot of this rate: what B returns at most for a history below K_B and S new samples
int cap_of(const ws_rate_tail_pool* p, const RtRate& rt) {
  return static_cast<int>(std::min<long long>(0x7fffffff, ((long long)(rt.b.K + p->S) / rt.b.D + 2) * rt.b.U));
}

// does a slot with N model-rate samples fire at a tick?  (the tail pool's condition)
bool fires(const ws_rate_tail_pool* p, const RtSlot& sl, long long N) {
  return N >= p->warm && (!sl.fired || N - sl.F >= std::max(p->C, 1));
}

// the first caller-rate sample that a window starting at model-rate sample a reads
long long span_lo(const Geom& g, long long a) { return std::max<long long>(0, (a / g.U) * g.D - g.w); }

// The parts (ascending slots) through the gather, the separator, the emission and B into B's compact block.  The staging block
// -- spans | embedding rows | gather table | emission table | B's table | the copy table of a flush that only returns the
// hold, each part 256-byte aligned -- is built on the host and uploaded once.  Rows: the full windows first, ordered
// (slot, target); then every warm-up slot's own rows: the tail pool's order, and its forwards.
int run_parts(ws_rate_tail_pool* p, std::vector<RtPart>& parts) {
  ws_engine* e = p->e;
  const int K = p->K, S = p->S, C = p->C, E = e->E;
  float* const state = reinterpret_cast<float*>(p->state);
  const long long state_floats = static_cast<long long>(p->state_bytes / 4);
  std::vector<const RtPart*> order;
  for (const RtPart& q : parts)
    if (q.window && q.L == S) order.push_back(&q);
  const int n_full = static_cast<int>(order.size());
  for (const RtPart& q : parts)
    if (q.window && q.L != S) order.push_back(&q);
  const int R = K * static_cast<int>(order.size());
  const int RB = K * static_cast<int>(parts.size());
  // the spans, at the caller's rate: one a slot, shared by its K rows
  struct Span {
    long long lo = 0;
    int n = 0, lead = 0, g_first = 0, p_first = 0;
    size_t at = 0;
  };
  std::vector<Span> spans(order.size());
  size_t span_floats = 0;
  for (size_t i = 0; i < order.size(); ++i) {
    const RtPart* q = order[i];
    const RtSlot& sl = p->sl[q->slot];
    const Geom& g = p->rates[sl.ri].a;
    const long long a = q->N - q->L, g_a = a / g.U, g_last = (q->N - 1) / g.U;
    Span& s = spans[i];
    s.lo = span_lo(g, a);
    const long long hi = q->final ? sl.Nc : std::min(sl.Nc, g_last * g.D - g.w + g.K);
    s.n = static_cast<int>(hi - s.lo);
    s.p_first = static_cast<int>(a - g_a * g.U);
    if (g_a * g.D >= g.w)               // the span starts at the first tap of the window's first group: the buffer's group 0
      s.lead = 0, s.g_first = 0;
    else                                // the span starts at sample 0 of the recording: the buffer's groups are the signal's
      s.lead = g.w, s.g_first = static_cast<int>(g_a);
    s.at = span_floats;
    span_floats += size_t(s.n);
    if (s.lo < sl.c0 || s.n < 1 || s.n > p->span_cap) {
      set_err("%s: internal error: slot %d: the window needs caller samples [%lld, %lld + %d), kept from %lld on, room for %lld", kWho, q->slot,
              s.lo, s.lo, s.n, sl.c0, p->span_cap);
      return WS_ERR_LAUNCH;
    }
  }
  // the block's layout, in bytes from its start
  const size_t o_span = 0, o_emb = o_span + up256(span_floats * 4), o_gather = o_emb + up256(size_t(R) * E * 4),
               o_emit = o_gather + up256(size_t(R) * sizeof(ws_window_resample_row)), o_b = o_emit + up256(size_t(R) * sizeof(ws_tail_emit_row)),
               o_copy = o_b + up256(size_t(RB) * sizeof(ws_resample_row)),
               total = o_copy + up256(parts[0].window ? 0 : size_t(K) * sizeof(ws_rows_copy_row));
  if (total > p->stage_bytes) {
    set_err("%s: a tick needs %zu bytes of staging, the state holds %zu", kWho, total, p->stage_bytes);
    return WS_ERR_LAUNCH;
  }
  p->keep.emplace_back(total, char(0));
  char* const blk = p->keep.back().data();
  float* const h_span = reinterpret_cast<float*>(blk + o_span);
  float* const h_emb = reinterpret_cast<float*>(blk + o_emb);
  ws_window_resample_row* const gather = reinterpret_cast<ws_window_resample_row*>(blk + o_gather);
  ws_tail_emit_row* const emit = reinterpret_cast<ws_tail_emit_row*>(blk + o_emit);
  const long long stage = p->stage_off;       // floats
  long long at = 0;                           // floats into the rows / estimates rectangles
  int r = 0;
  for (size_t i = 0; i < order.size(); ++i) {
    const RtPart* q = order[i];
    const RtSlot& sl = p->sl[q->slot];
    const RtRate& rt = p->rates[sl.ri];
    const Span& s = spans[i];
    memcpy(h_span + s.at, sl.pend.data() + size_t(s.lo - sl.c0), size_t(s.n) * 4);
    const int in = sl.flip, to = sl.flip ^ 1;
    for (int k = 0; k < K; ++k, ++r, at += q->L) {
      ws_window_resample_row d{};
      d.in_off = stage + (long long)(o_span / 4 + s.at), d.taps_off = rt.a_taps, d.out_off = p->rows_off + at;
      d.U = rt.a.U, d.D = rt.a.D, d.K = rt.a.K, d.lead = s.lead, d.n_valid = s.n, d.final = q->final ? 1 : 0;
      d.g_first = s.g_first, d.p_first = s.p_first, d.L = q->L, d.fill = 0;
      gather[r] = d;
      memcpy(h_emb + size_t(r) * E, sl.emb.data() + size_t(k) * E, size_t(E) * 4);
      emit[r] = ws_tail_emit_row{p->y_off + at,
                                 p->hold_off + (((long long)q->slot * 2 + in) * K + k) * C,
                                 p->hold_off + (((long long)q->slot * 2 + to) * K + k) * C,
                                 p->bbuf(q->slot, k, sl.b_cur) + sl.b_h,
                                 q->L, q->p, q->h, q->m, q->c_new, 1.0f};
    }
  }
  // B's table: every (slot, target) row that has something to run; a flush that only returns the hold copies it behind the history
  std::vector<ws_resample_row> btab;
  std::vector<ws_rows_copy_row> ctab;
  long long bout = 0;
  for (RtPart& q : parts) {
    const RtSlot& sl = p->sl[q.slot];
    const RtRate& rt = p->rates[sl.ri];
    q.out_off = bout;
    for (int k = 0; k < K; ++k) {
      if (!q.window && q.m > 0)
        ctab.push_back(ws_rows_copy_row{p->hold_off + (((long long)q.slot * 2 + sl.flip) * K + k) * C, p->bbuf(q.slot, k, sl.b_cur) + sl.b_h, q.m, 0});
      if (q.st.n_valid == 0 || (q.st.n_out == 0 && q.st.hist_len == 0)) continue;
      ws_resample_row d{};
      d.in_off = p->bbuf(q.slot, k, sl.b_cur), d.taps_off = rt.b_taps, d.out_off = p->bout_off + bout + (long long)k * q.st.n_out;
      d.hist_off = p->bbuf(q.slot, k, 1 - sl.b_cur);
      d.U = rt.b.U, d.D = rt.b.D, d.K = rt.b.K, d.lead = q.st.lead, d.n_valid = q.st.n_valid, d.final = q.final ? 1 : 0, d.n_out = q.st.n_out;
      d.hist_from = q.st.hist_from, d.hist_len = q.st.hist_len;
      btab.push_back(d);
    }
    bout += (long long)K * q.st.n_out;
  }
  ws_resample_row* const h_btab = reinterpret_cast<ws_resample_row*>(blk + o_b);
  ws_rows_copy_row* const h_ctab = reinterpret_cast<ws_rows_copy_row*>(blk + o_copy);
  if (!btab.empty()) memcpy(h_btab, btab.data(), btab.size() * sizeof(ws_resample_row));
  if (!ctab.empty()) memcpy(h_ctab, ctab.data(), ctab.size() * sizeof(ws_rows_copy_row));
  int rc;
  char* const d_blk = p->state + size_t(stage) * 4;
  if ((rc = copy_async(e, kWho, "host-to-device copy", d_blk, blk, total, hipMemcpyHostToDevice)) != WS_OK) return rc;
  if (R > 0) {
    WS_RUN(e, ws_window_resample_rows_fwd(gather, reinterpret_cast<const ws_window_resample_row*>(d_blk + o_gather), R, state, state_floats,
                                          state, state_floats, state, state_floats, e->stream));
    Arena& a = e->work;
    const float* d_emb = reinterpret_cast<const float*>(d_blk + o_emb);
    const Arena::Mark mk = a.mark();
    // the forwards: [r0, r1) are rows of one length L
    auto forward_rows = [&](int r0, int r1, long long at0, int L) -> int {
      for (int g0 = r0; g0 < r1; g0 += p->max_rows) {
        const int Gn = std::min(p->max_rows, r1 - g0);
        a.release(mk);
        const float* in = state + p->rows_off + at0 + (long long)(g0 - r0) * L;
        float* out = state + p->y_off + at0 + (long long)(g0 - r0) * L;
        const int frc = e->arch == 1   ? tasnet_device(e, in, Gn, L, d_emb + size_t(g0) * E, nullptr, 0, out)
                        : e->arch == 2 ? dpccn_device(e, in, Gn, L, d_emb + size_t(g0) * E, out)
                                       : separate_device(e, in, Gn, L, d_emb + size_t(g0) * E, out);
        if (frc != WS_OK) return frc;
        ++p->forwards;
      }
      return WS_OK;
    };
    if (n_full > 0 && (rc = forward_rows(0, n_full * K, 0, S)) != WS_OK) return rc;
    at = (long long)n_full * K * S;
    for (size_t i = size_t(n_full); i < order.size(); ++i) {
      const int r0 = static_cast<int>(i) * K;
      if ((rc = forward_rows(r0, r0 + K, at, order[i]->L)) != WS_OK) return rc;
      at += (long long)K * order[i]->L;
    }
    a.release(mk);
    WS_RUN(e, ws_tail_emit_rows_fwd(emit, reinterpret_cast<const ws_tail_emit_row*>(d_blk + o_emit), R, C, state + p->ramp_off, state,
                                    state_floats, state, state_floats, state, state_floats, e->stream));
    p->rows += R;
  } else if (!ctab.empty()) {
    WS_RUN(e, ws_rows_copy_fwd(h_ctab, reinterpret_cast<const ws_rows_copy_row*>(d_blk + o_copy), static_cast<int>(ctab.size()), state,
                               state_floats, state, state_floats, e->stream));
  }
  if (!btab.empty())
    WS_RUN(e, ws_resample_stream_rows_fwd(h_btab, reinterpret_cast<const ws_resample_row*>(d_blk + o_b), static_cast<int>(btab.size()), state,
                                          state_floats, state, state_floats, state, state_floats, state, state_floats, e->stream));
  return WS_OK;
}

// the call's one copy to the host and its one synchronisation
int finish(ws_rate_tail_pool* p, long long n_out) {
  ws_engine* e = p->e;
  int rc;
  p->out_host.assign(size_t(n_out), 0.f);
  ++e->n_launches;
  if ((rc = copy_async(e, kWho, "device-to-host copy", p->out_host.data(), reinterpret_cast<const float*>(p->state) + p->bout_off,
                       size_t(n_out) * 4, hipMemcpyDeviceToHost)) != WS_OK)
    return rc;
  unsigned timed_out = 0;                // did a cluster recurrence time out (note_cluster_status)?  read in the same wait
  if (e->cl_status && (rc = copy_async(e, kWho, "device-to-host copy", &timed_out, e->cl_status, 4, hipMemcpyDeviceToHost)) != WS_OK) return rc;
  if ((rc = sync_stream(e, kWho)) != WS_OK) return rc;
  if (timed_out) {
    ++e->cluster_fallbacks;
    if ((rc = zero_device(e, e->cl_status, 4)) != WS_OK) return rc;
  }
  p->keep.clear();
  e->rate_tail_pool_forwards = p->forwards, e->rate_tail_pool_rows = p->rows;
  return WS_OK;
}

// after the synchronisation: a part's estimates to its caller's buffer, B's counters one step on
void deliver(ws_rate_tail_pool* p, const RtPart& q, float* est, int est_cap) {
  RtSlot& sl = p->sl[q.slot];
  if (!p->e->dry)
    for (int k = 0; k < p->K && q.n_ret > 0; ++k)
      memcpy(est + size_t(k) * est_cap, p->out_host.data() + q.out_off + (long long)k * q.st.n_out, size_t(q.n_ret) * 4);
  sl.b_n += q.m, sl.returned += q.n_ret;
  if (!q.final && q.st.n_valid > 0 && (q.st.n_out > 0 || q.st.hist_len > 0)) sl.b_cur ^= 1, sl.b_h = q.st.hist_len, sl.b_groups = q.st.g_new;
}

// drop the caller samples that no later window reads: a window's start only moves on
void trim(const ws_rate_tail_pool* p, RtSlot& sl) {
  const Geom& g = p->rates[sl.ri].a;
  const long long lo = span_lo(g, std::max<long long>(0, rs_emitted(g, sl.Nc) - p->S));
  if (lo > sl.c0) sl.pend.erase(sl.pend.begin(), sl.pend.begin() + (lo - sl.c0)), sl.c0 = lo;
}

}  // namespace

WS_ENGINE_API int ws_engine_rate_tail_pool_open(ws_engine* e, int slots, int K, int window, int fade, int warm, int max_rows,
                                                const int* rates, int n_rates, ws_rate_tail_pool** out) {
  const char* who = "ws_engine_rate_tail_pool_open";
  int rc = check_engine(e, who);
  if (rc != WS_OK) return rc;
  if (out) *out = nullptr;
  if (!out || K < 1 || n_rates < 0 || (n_rates > 0 && !rates)) {
    set_err("%s: bad arguments (K=%d >= 1, n_rates=%d >= 0%s, out %s)", who, K, n_rates, n_rates > 0 && !rates ? ", rates is NULL" : "",
            out ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  if (e->arch == 3) {
    set_err("%s: a TF-GridNet container is not taken: its windows are scaled by their standard deviation, computed on the host from "
            "samples at the container's rate, which this pool never has there (ws_engine_tail_pool_open takes it, at %d Hz)", who, e->sr);
    return WS_ERR_INVALID;
  }
  if (slots < 1 || slots > 65535) {
    set_err("%s: slots=%d is outside [1, 65535]", who, slots);
    return WS_ERR_INVALID;
  }
  // what ws_engine_separate_long demands of a window, with its messages (the overlap is this family's fade, checked below)
  if ((rc = long_check_window(e, window, 0, max_rows)) != WS_OK) return rc;
  const int S = window, C = fade;
  if (C < 0 || C > S / 2) {
    set_err("%s: fade = %d outside [0, window / 2 = %d]", who, C, S / 2);
    return WS_ERR_INVALID;
  }
  const long long r_max = (long long)slots * K;
  if (r_max > 65535) {
    set_err("%s: %d slots x %d speakers = %lld rows in a tick, the tables of a launch hold 65535", who, slots, K, r_max);
    return WS_ERR_INVALID;
  }
  if ((rc = check_rows(e, true, static_cast<int>(std::min<long long>(r_max, max_rows)), S)) != WS_OK) return rc;
  if (warm < std::max(C, 1) || warm > S) {
    set_err("%s: warm = %d outside [max(fade, 1) = %d, window = %d]", who, warm, std::max(C, 1), S);
    return WS_ERR_INVALID;
  }
  // the shortest window that may fire, as a mixture of its own: the architecture's lower bound on T, with its message
  if ((rc = check_rows(e, true, 1, warm)) != WS_OK) return rc;
  std::unique_ptr<ws_rate_tail_pool> up(new ws_rate_tail_pool());
  ws_rate_tail_pool* p = up.get();
  p->e = e, p->slots = slots, p->K = K, p->S = S, p->C = C, p->warm = warm, p->max_rows = max_rows;
  RtRate own;
  own.rate = e->sr;
  p->rates.push_back(own);
  for (int i = 0; i < n_rates; ++i) {
    bool seen = false;
    for (const RtRate& r : p->rates) seen = seen || r.rate == rates[i];
    if (seen) continue;
    RtRate r;
    r.rate = rates[i];
    if (ws_resample_geom(r.rate, e->sr, &r.a.U, &r.a.D, &r.a.w, &r.a.K) != WS_OK ||
        ws_resample_geom(e->sr, r.rate, &r.b.U, &r.b.D, &r.b.w, &r.b.K) != WS_OK) {
      set_err("%s: rates[%d]: %s", who, i, ws_last_error());
      return WS_ERR_INVALID;
    }
    p->rates.push_back(r);
  }
  // ---- sizes, from (slots, K, S, C, max_rows) and the worst listed geometry ----
  long long taps = 0;
  for (RtRate& r : p->rates) {
    // a window of S outputs touches at most (S + U - 2) / U + 1 groups; their taps span (groups - 1) D + K input samples
    p->span_cap = std::max<long long>(p->span_cap, ((long long)(S + r.a.U - 2) / r.a.U) * r.a.D + r.a.K);
    p->b_ld = std::max<long long>(p->b_ld, r.b.K - 1 + S);
    p->b_cap = std::max<long long>(p->b_cap, cap_of(p, r));
    r.a_taps = taps, taps += (long long)r.a.U * r.a.K;
    r.b_taps = taps, taps += (long long)r.b.U * r.b.K;
  }
  p->b_ld = (p->b_ld + 3) / 4 * 4, p->b_cap = (p->b_cap + 3) / 4 * 4;
  p->sl.resize(slots);
  // the staging block of the fullest tick: every slot with a full window; the tables of a flush that only returns the hold
  p->stage_bytes = up256(size_t(slots) * p->span_cap * 4) + up256(size_t(r_max) * e->E * 4) + up256(size_t(r_max) * sizeof(ws_window_resample_row)) +
                   up256(size_t(r_max) * sizeof(ws_tail_emit_row)) + up256(size_t(r_max) * sizeof(ws_resample_row)) +
                   up256(size_t(K) * sizeof(ws_rows_copy_row));
  const size_t parts[9] = {size_t(slots) * 2 * K * C * 4, size_t(slots) * K * e->E * 4, p->stage_bytes, size_t(r_max) * S * 4, size_t(r_max) * S * 4,
                           size_t(r_max) * 2 * p->b_ld * 4, size_t(r_max) * p->b_cap * 4, size_t(C) * 4, size_t(taps) * 4};
  long long* at[9] = {&p->hold_off, &p->emb_off, &p->stage_off, &p->rows_off, &p->y_off, &p->b_off, &p->bout_off, &p->ramp_off, &p->taps_off};
  size_t total = 0;
  for (int i = 0; i < 9; ++i) *at[i] = static_cast<long long>(total / 4), total += up256(parts[i]);
  total = std::max<size_t>(total, 256);
  if (total / 4 >= (1ULL << 40)) {
    set_err("%s: slots=%d with window=%d reaches 2^40 elements of state", who, slots, S);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  p->state_bytes = total;
  if (e->dry) {
    p->state = static_cast<char*>(malloc(total));
  } else if (hipMalloc(reinterpret_cast<void**>(&p->state), total) != hipSuccess) {
    p->state = nullptr;
  }
  if (!p->state) {
    set_err("%s: device allocation of %zu bytes failed", who, total);
    return WS_ERR_LAUNCH;
  }
  up.release();
  if (e->work.poison && !e->dry) {      // WS_ENGINE_POISON (tests): state no launch has written reads as NaN
    (void)hipDeviceSynchronize();
    (void)hipMemset(p->state, 0xFF, total);
    (void)hipDeviceSynchronize();
  }
  // the ramp of the cross-fade, ramp[j] = float(j + 1) / float(C + 1), and every tap table, made in the one place: one upload
  std::vector<float> host(size_t(p->taps_off - p->ramp_off) + size_t(taps), 0.f);
  for (int j = 0; j < C; ++j) host[j] = static_cast<float>(j + 1) / static_cast<float>(C + 1);
  float* const h_taps = host.data() + size_t(p->taps_off - p->ramp_off);
  for (RtRate& r : p->rates) {
    if (r.rate == e->sr) {
      h_taps[r.a_taps] = h_taps[r.b_taps] = 1.f;       // the identity table
    } else if (ws_resample_taps(r.rate, e->sr, h_taps + r.a_taps) != WS_OK || ws_resample_taps(e->sr, r.rate, h_taps + r.b_taps) != WS_OK) {
      set_err("%s: %s", who, ws_last_error());
      free_pool(p);
      return WS_ERR_INVALID;
    }
    r.a_taps += p->taps_off, r.b_taps += p->taps_off;
  }
  if ((rc = to_device(e, reinterpret_cast<float*>(p->state) + p->ramp_off, host.data(), host.size() * 4)) != WS_OK) {
    free_pool(p);
    return rc;
  }
  e->rate_tail_pool_state_bytes = static_cast<long long>(total);
  e->rate_tail_pool_forwards = e->rate_tail_pool_rows = 0;
  *out = p;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_tail_pool_attach(ws_rate_tail_pool* p, const void* enroll, int enroll_kind, int enroll_len,
                                                  const int* enroll_lengths, int enroll_rate, int sample_rate, int* slot) {
  const char* who = "ws_engine_rate_tail_pool_attach";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  int ri = -1;
  for (size_t i = 0; i < p->rates.size(); ++i)
    if (p->rates[i].rate == sample_rate) ri = static_cast<int>(i);
  if (ri < 0) {
    set_err("%s: sample_rate=%d is not one of the rates this pool was opened with (accepted: %s)", who, sample_rate, rates_text(p).c_str());
    return WS_ERR_INVALID;
  }
  {
    // the most container-rate samples a slot of this rate can have while a push is still taken (ceil(U N_c / D) <= S before the
    // first firing): below warm, the slot would never fire
    const Geom& g = p->rates[ri].a;
    const long long nc_max = (long long)g.D * p->S / g.U, n_max = rs_emitted(g, nc_max);
    if (n_max < p->warm) {
      set_err("%s: sample_rate=%d: a slot at this rate never fires: warm = %d, and the %lld samples a window of %d lets it push are %lld at the "
              "container's rate once the filter has its %d samples of look-ahead (open the pool with warm <= %lld)", who, sample_rate, p->warm,
              nc_max, p->S, n_max, g.w, n_max);
      return WS_ERR_INVALID;
    }
  }
  const bool enr_rs = enroll_rate != 0 && enroll_rate != e->sr;
  if (enr_rs && enroll_kind != WS_ENROLL_WAVE) {
    set_err("%s: enroll_rate=%d with enrollment kind %d: only a waveform enrollment (WS_ENROLL_WAVE) has a sample rate; pass 0 or the "
            "container's %d", who, enroll_rate, enroll_kind, e->sr);
    return WS_ERR_INVALID;
  }
  if (!enroll || !slot) {
    set_err("%s: bad arguments (enroll %s, slot %s)", who, enroll ? "given" : "NULL", slot ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  const int K = p->K;
  // a waveform enrollment at another rate: every row resampled over its own length, into a rectangle at the container's rate
  std::vector<float> enr_m;
  std::vector<int> len_m;
  int pitch_m = enroll_len;
  Geom ge;
  if (enr_rs) {
    if (ws_resample_geom(enroll_rate, e->sr, &ge.U, &ge.D, &ge.w, &ge.K) != WS_OK) {
      set_err("%s: %s", who, ws_last_error());
      return WS_ERR_INVALID;
    }
    if (enroll_len < 1) {
      set_err("%s: enroll_len=%d, a waveform enrollment has at least one sample", who, enroll_len);
      return WS_ERR_INVALID;
    }
    for (int k = 0; k < K && enroll_lengths; ++k)
      if (enroll_lengths[k] < 1 || enroll_lengths[k] > enroll_len) {
        set_err("%s: enroll_lengths[%d]=%d is outside [1, enroll_len=%d]", who, k, enroll_lengths[k], enroll_len);
        return WS_ERR_INVALID;
      }
    pitch_m = static_cast<int>(rs_len(ge, enroll_len));
    if (enroll_lengths)
      for (int k = 0; k < K; ++k) len_m.push_back(static_cast<int>(rs_len(ge, enroll_lengths[k])));
  }
  const int* lengths = enr_rs && enroll_lengths ? len_m.data() : enroll_lengths;
  int Te = pitch_m;
  std::vector<int> te_row;
  if ((rc = long_check_group(e, static_cast<int>(std::min<long long>((long long)p->slots * K, p->max_rows)), p->S, K, enroll_kind, pitch_m, lengths,
                             &Te, &te_row)) != WS_OK)
    return rc;
  int id = 0;
  while (id < p->slots && p->sl[id].state != RtSlot::kFree) ++id;
  if (id == p->slots) {
    set_err("%s: the pool is full: all %d slots are attached (detach one, or open a larger pool)", who, p->slots);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  if (enr_rs) {
    const float* x = static_cast<const float*>(enroll);
    enr_m.assign(size_t(K) * pitch_m, 0.f);
    std::vector<float> row;
    for (int k = 0; k < K; ++k) {
      int got = 0;
      const int n_k = enroll_lengths ? enroll_lengths[k] : enroll_len;
      if ((rc = resample_host_rows(e, who, x + size_t(k) * enroll_len, 1, n_k, enroll_rate, e->sr, &row, &got)) != WS_OK) return rc;
      memcpy(enr_m.data() + size_t(k) * pitch_m, row.data(), size_t(got) * 4);
    }
    enroll = enr_m.data();
  }
  RtSlot fresh;
  fresh.emb.assign(size_t(K) * e->E, 0.f);
  float* d_emb = reinterpret_cast<float*>(p->state) + p->emb_off + size_t(id) * K * e->E;
  {
    ArenaScope scope(e->work);           // the speaker stage, once for this slot's K enrollments
    rc = speaker_stage(e, enroll, enroll_kind, K, pitch_m, Te, lengths, te_row.data(), d_emb);
    if (rc == WS_OK) rc = to_host(e, fresh.emb.data(), d_emb, fresh.emb.size() * 4);
  }
  if (rc != WS_OK) return rc;
  fresh.state = RtSlot::kAttached;
  fresh.ri = ri;
  p->sl[id] = std::move(fresh);         // at sample 0; holds and B's buffers need no clearing (read only after a launch wrote them)
  *slot = id;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_tail_pool_cap(const ws_rate_tail_pool* p, int slot) {
  if (!p || !p->e || slot < 0 || slot >= p->slots || p->sl[slot].ri < 0) return -1;
  return cap_of(p, p->rates[p->sl[slot].ri]);
}

WS_ENGINE_API int ws_engine_rate_tail_pool_room(const ws_rate_tail_pool* p, int slot) {
  if (!p || !p->e || slot < 0 || slot >= p->slots || p->sl[slot].state != RtSlot::kAttached) return -1;
  const RtSlot& sl = p->sl[slot];
  const Geom& g = p->rates[sl.ri].a;
  // ceil(U (N_c + n) / D) - E <= S  <=>  n <= floor(D (S + E) / U) - N_c
  return static_cast<int>(std::max<long long>(0, std::min<long long>(0x7fffffff, (long long)g.D * (p->S + sl.E) / g.U - sl.Nc)));
}

WS_ENGINE_API int ws_engine_rate_tail_pool_push(ws_rate_tail_pool* p, int n_active, const int* slots, const float* const* chunks,
                                                const int* n) {
  const char* who = "ws_engine_rate_tail_pool_push";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  if (n_active < 1 || !slots || !chunks || !n) {
    set_err("%s: bad arguments (n_active=%d >= 1%s)", who, n_active, slots && chunks && n ? "" : ", a NULL array");
    return WS_ERR_INVALID;
  }
  const int S = p->S;
  std::vector<char> seen(p->slots, 0);
  for (int i = 0; i < n_active; ++i) {
    const int id = slots[i];
    if ((rc = check_slot(p, who, id, i)) != WS_OK) return rc;
    if (seen[id]) {
      set_err("%s: slot %d is named twice (entry %d): one packet a slot in a push", who, id, i);
      return WS_ERR_INVALID;
    }
    if (n[i] < 1 || !chunks[i]) {
      set_err("%s: entry %d (slot %d): n=%d >= 1, chunk %s", who, i, id, n[i], chunks[i] ? "given" : "NULL");
      return WS_ERR_INVALID;
    }
    seen[id] = 1;
    const RtSlot& sl = p->sl[id];
    const RtRate& rt = p->rates[sl.ri];
    const long long waiting = rs_len(rt.a, sl.Nc + n[i]) - sl.E;      // what a flush right after this push would have to emit
    if (waiting > S) {
      set_err("%s: entry %d (slot %d): %d more samples at %d Hz make %lld at the container's rate that have not come out, a window holds "
              "%d: tick first", who, i, id, n[i], rt.rate, waiting, S);
      return WS_ERR_INVALID;
    }
  }
  for (int i = 0; i < n_active; ++i) {  // no launch, no synchronisation: the samples wait on the host for the next tick
    RtSlot& sl = p->sl[slots[i]];
    sl.pend.insert(sl.pend.end(), chunks[i], chunks[i] + n[i]);
    sl.Nc += n[i];
    trim(p, sl);
  }
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_tail_pool_tick(ws_rate_tail_pool* p, int n_active, const int* slots, float* const* est, const int* est_cap,
                                                int* n_out) {
  const char* who = "ws_engine_rate_tail_pool_tick";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  if (n_active < 1 || !slots || !est || !est_cap || !n_out) {
    set_err("%s: bad arguments (n_active=%d >= 1%s)", who, n_active, slots && est && est_cap && n_out ? "" : ", a NULL array");
    return WS_ERR_INVALID;
  }
  const int S = p->S, C = p->C;
  std::vector<char> seen(p->slots, 0);
  std::vector<RtPart> parts;
  for (int i = 0; i < n_active; ++i) {
    const int id = slots[i];
    if ((rc = check_slot(p, who, id, i)) != WS_OK) return rc;
    if (seen[id]) {
      set_err("%s: slot %d is named twice (entry %d)", who, id, i);
      return WS_ERR_INVALID;
    }
    seen[id] = 1;
    const RtSlot& sl = p->sl[id];
    const RtRate& rt = p->rates[sl.ri];
    const long long N = rs_emitted(rt.a, sl.Nc);
    if (!fires(p, sl, N)) continue;
    RtPart q;
    q.slot = id, q.entry = i, q.N = N;
    q.L = static_cast<int>(std::min<long long>(N, S));
    q.m = static_cast<int>(N - C - sl.E), q.c_new = C, q.h = sl.fired ? C : 0;
    q.p = static_cast<int>(sl.E - (N - q.L));
    q.st = plan_step(rt.b, sl.b_n, sl.b_groups, sl.b_h, q.m, false);
    if (q.m == 0) q.st = Step();        // nothing reaches B (a first firing with warm == fade)
    q.n_ret = q.st.n_out;
    if (q.n_ret > est_cap[i] || (q.n_ret > 0 && !est[i])) {
      set_err("%s: entry %d (slot %d) emits %d samples a row, est_cap is %d%s (ws_engine_rate_tail_pool_cap(pool, %d) = %d always suffices)",
              who, i, id, q.n_ret, est_cap[i], est[i] ? "" : ", est is NULL", id, cap_of(p, rt));
      return WS_ERR_INVALID;
    }
    parts.push_back(q);
  }
  p->forwards = p->rows = 0;
  for (int i = 0; i < n_active; ++i) n_out[i] = 0;
  if (parts.empty()) {                  // no slot fires: no launch, no synchronisation
    e->n_launches = 0;
    e->rate_tail_pool_forwards = e->rate_tail_pool_rows = 0;
    return WS_OK;
  }
  std::sort(parts.begin(), parts.end(), [](const RtPart& a, const RtPart& b) { return a.slot < b.slot; });
  for (int i = 0; i < n_active; ++i) p->sl[slots[i]].failed = true;      // until the tick is complete
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  ArenaScope scope(e->work);
  if ((rc = run_parts(p, parts)) != WS_OK) return rc;
  long long total = 0;
  for (const RtPart& q : parts) total += (long long)p->K * q.st.n_out;
  if ((rc = finish(p, total)) != WS_OK) return rc;
  for (const RtPart& q : parts) {
    RtSlot& sl = p->sl[q.slot];
    deliver(p, q, est[q.entry], est_cap[q.entry]);
    sl.F = q.N, sl.E = q.N - C, sl.fired = true, sl.flip ^= 1;
    n_out[q.entry] = q.n_ret;
  }
  for (int i = 0; i < n_active; ++i) p->sl[slots[i]].failed = false;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_tail_pool_flush(ws_rate_tail_pool* p, int slot, float* est, int est_cap, int* n_out) {
  const char* who = "ws_engine_rate_tail_pool_flush";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  if ((rc = check_slot(p, who, slot, -1)) != WS_OK) return rc;
  RtSlot& sl = p->sl[slot];
  const RtRate& rt = p->rates[sl.ri];
  const int S = p->S, C = p->C, K = p->K;
  if (sl.Nc < 1) {
    set_err("%s: slot %d: nothing was pushed", who, slot);
    return WS_ERR_INVALID;
  }
  RtPart q;
  q.slot = slot, q.final = true;
  q.N = rs_len(rt.a, sl.Nc);            // the whole recording at the container's rate
  const long long emitted = q.N - sl.E;
  q.window = !sl.fired || q.N > sl.F;
  q.L = static_cast<int>(std::min<long long>(q.N, S));
  q.m = static_cast<int>(emitted), q.c_new = 0, q.h = sl.fired ? C : 0;
  q.p = static_cast<int>(sl.E - (q.N - q.L));
  q.st = plan_step(rt.b, sl.b_n, sl.b_groups, sl.b_h, q.m, true);
  q.n_ret = static_cast<int>(std::max<long long>(0, std::min<long long>(q.st.n_out, sl.Nc - sl.returned)));      // cropped to the samples pushed
  if (!n_out || q.n_ret > est_cap || (q.n_ret > 0 && !est)) {
    set_err("%s: slot %d: the flush emits %d samples a row, est_cap is %d%s (ws_engine_rate_tail_pool_cap(pool, %d) = %d always suffices)", who,
            slot, q.n_ret, est_cap, est && n_out ? "" : ", est or n_out is NULL", slot, cap_of(p, rt));
    return WS_ERR_INVALID;
  }
  // a last window shorter than S has the architecture's own lower bound on T; refused before anything runs, so a later push
  // goes on from here
  if (q.window && q.L < S && (rc = check_rows(e, true, K < p->max_rows ? K : p->max_rows, q.L)) != WS_OK) return rc;
  p->forwards = p->rows = 0;
  if (q.st.n_valid == 0 || q.st.n_out == 0) {      // nothing is left to come out: no launch
    e->n_launches = 0;
    e->rate_tail_pool_forwards = e->rate_tail_pool_rows = 0;
    sl.pend.clear();
    sl.state = RtSlot::kDone;
    *n_out = 0;
    return WS_OK;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  sl.failed = true;
  ArenaScope scope(e->work);
  std::vector<RtPart> parts(1, q);
  if ((rc = run_parts(p, parts)) != WS_OK) return rc;
  if ((rc = finish(p, (long long)K * parts[0].st.n_out)) != WS_OK) return rc;
  deliver(p, parts[0], est, est_cap);
  sl.E = sl.F = q.N;
  sl.pend.clear();
  sl.failed = false;
  sl.state = RtSlot::kDone;
  *n_out = q.n_ret;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_tail_pool_detach(ws_rate_tail_pool* p, int slot) {
  const char* who = "ws_engine_rate_tail_pool_detach";
  const int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  if (slot < 0 || slot >= p->slots || p->sl[slot].state == RtSlot::kFree) {
    set_err("%s: slot %d is not attached (the pool has %d slots)", who, slot, p->slots);
    return WS_ERR_INVALID;
  }
  if (p->sl[slot].failed) {              // a call that failed half way may have left work behind that reads this slot's buffers
    ForwardTurn turn(p->e);
    if (turn.rc != WS_OK) return turn.rc;
    (void)sync_stream(p->e, kWho);
    p->keep.clear();
  }
  p->sl[slot] = RtSlot();               // free, and no longer the slot of a half-finished call
  return WS_OK;
}

WS_ENGINE_API void ws_engine_rate_tail_pool_close(ws_rate_tail_pool* p) {
  if (!p) return;
  if (p->e && !p->e->dry) {
    (void)hipSetDevice(p->e->device);
    (void)hipStreamSynchronize(p->e->stream);
  }
  free_pool(p);
}
