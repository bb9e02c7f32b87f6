// =================================================================================================================
// Tail pool (ws_engine_tail_pool_*; DESIGN 7 "Tail pool" and 11b): MANY live recordings on one engine, separated on their
// TRAILING windows.  A tick runs, for every named slot that has enough new audio, the window of its newest S samples and emits
// the newest part of it; the last C samples of a window are held back and cross-faded into the next window's estimate of the
// same positions.  The clock is the caller's, not the recordings': however the calls are staggered, every slot with new audio
// fires on the same tick and its rows share the forwards.  Latency: the tick period plus C samples.  Price: one full window a
// slot a tick.  The output is a rule of its own (include/wesep_engine.h), not ws_engine_separate_long.
//   * the state is ONE device allocation made at open, a function of (slots, K, S, C, max_rows): per slot the two hold buffers
//     [2][K][C] and the K embeddings; per tick the staging block (the slots' spans of at most S samples, the embedding rows, the
//     gather, emission and copy tables), the rows, estimates and output rectangles (slots K rows of pitch S); the ramp [C].
//     Pending samples (at most S a slot) live on the host;
//   * a tick is one upload of its staging block, ONE ws_window_slots_fwd for all rows, the architecture's rectangular plan --
//     full windows ordered (slot, target) in forwards of at most max_rows rows whichever slots they came from, a slot still in
//     warm-up (L < S) in forwards of its own rows -- ONE ws_tail_emit_rows_fwd, one copy to the host, ONE synchronisation;
//   * transient activations come from the engine's work arena under an ArenaScope; nothing of it is held between two calls.
// No launch mixes rows: a slot's samples do not depend on what the other slots carry.
// =================================================================================================================
#include <deque>

#include "engine_internal.h"

using namespace wsrt;

namespace {

struct TpSlot {
  enum State { kFree, kAttached, kDone } state = kFree;
  bool failed = false;                  // a tick or flush that named this slot ended half way
  bool fired = false;
  int flip = 0;                         // which of the two hold buffers the last firing wrote
  std::vector<float> pend;              // the newest samples, at most S: pend.back() is sample N - 1
  std::vector<float> emb;               // [K][E], host copy of the slot's embeddings
  long long N = 0, F = 0, E = 0;        // samples pushed, N at the last firing, samples emitted
};

// what one slot gives to one tick or flush: the window [N - L, N), of which m samples from local index p come out (the first h
// cross-faded with the hold) and c_new are held back
struct TpPart {
  int slot = 0, entry = 0, L = 0, p = 0, h = 0, m = 0, c_new = 0;
  long long out_off = 0;                // floats into the output rectangle: [K][m]
};

}  // namespace

struct ws_tail_pool {
  ws_engine* e = nullptr;
  int slots = 0, K = 0, S = 0, C = 0, warm = 0, max_rows = 0;
  char* state = nullptr;
  size_t state_bytes = 0, stage_bytes = 0;
  // float offsets into the state of its parts: holds [slots][2][K][C], embeddings [slots][K][E], the staging block, the rows,
  // estimates and output rectangles [slots K][S], the ramp [C]
  long long hold_off = 0, emb_off = 0, stage_off = 0, rows_off = 0, y_off = 0, out_off = 0, ramp_off = 0;
  std::vector<TpSlot> sl;
  std::deque<std::vector<char>> keep;   // host sources of the call's asynchronous uploads, alive until its synchronisation
  std::vector<float> out_host;          // the call's estimates, one block
  long long forwards = 0, rows = 0;
};

namespace {

constexpr const char* kWho = "ws_engine_tail_pool";

size_t up256(size_t b) { return Arena::round_up(b); }

int check_pool(const ws_tail_pool* p, const char* who) {
  if (!p || !p->e) {
    set_err("%s: null pool", who);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

// attached, not flushed, not the slot of a call that failed half way
int check_slot(const ws_tail_pool* p, const char* who, int id, int entry) {
  char where[48] = "";
  if (entry >= 0) snprintf(where, sizeof where, " (entry %d)", entry);
  if (id < 0 || id >= p->slots || p->sl[id].state == TpSlot::kFree)
    set_err("%s: slot %d%s is not attached (the pool has %d slots)", who, id, where, p->slots);
  else if (p->sl[id].failed)
    set_err("%s: slot %d%s took part in a call that failed half way; detach it", who, id, where);
  else if (p->sl[id].state == TpSlot::kDone)
    set_err("%s: slot %d%s was flushed (detach it, then attach the next recording)", who, id, where);
  else
    return WS_OK;
  return WS_ERR_INVALID;
}

void free_pool(ws_tail_pool* p) {
  if (p->state) {
    if (p->e->dry)
      free(p->state);
    else
      (void)hipFree(p->state);
  }
  delete p;
}

// does the slot fire at a tick?
bool fires(const ws_tail_pool* p, const TpSlot& sl) {
  return sl.N >= p->warm && (!sl.fired || sl.N - sl.F >= std::max(p->C, 1));
}

// The windows of `parts` (ascending slots) through the separator and the emission kernel into the output rectangle.  The
// staging block -- spans | embedding rows | gather table | emission table, each part 256-byte aligned -- is built on the host and
// uploaded once.  Rows: the full windows first, ordered (slot, target); then every warm-up slot's own rows.
int run_windows(ws_tail_pool* p, const std::vector<TpPart>& parts) {
  ws_engine* e = p->e;
  const int K = p->K, S = p->S, C = p->C, E = e->E;
  const bool grid = e->arch == 3;
  float* const state = reinterpret_cast<float*>(p->state);
  const long long state_floats = static_cast<long long>(p->state_bytes / 4);
  std::vector<const TpPart*> order;
  for (const TpPart& q : parts)
    if (q.L == S) order.push_back(&q);
  const int n_full = static_cast<int>(order.size());
  for (const TpPart& q : parts)
    if (q.L != S) order.push_back(&q);
  const int R = K * static_cast<int>(order.size());
  size_t span_floats = 0;
  for (const TpPart* q : order) span_floats += size_t(q->L);
  // the block's layout, in bytes from its start
  const size_t o_span = 0, o_emb = o_span + up256(span_floats * 4), o_gather = o_emb + up256(size_t(R) * E * 4),
               o_emit = o_gather + up256(size_t(R) * sizeof(ws_window_slot_row)), total = o_emit + up256(size_t(R) * sizeof(ws_tail_emit_row));
  if (total > p->stage_bytes) {
    set_err("%s: a tick needs %zu bytes of staging, the state holds %zu", kWho, total, p->stage_bytes);
    return WS_ERR_LAUNCH;
  }
  p->keep.emplace_back(total, char(0));
  char* const blk = p->keep.back().data();
  float* const h_span = reinterpret_cast<float*>(blk + o_span);
  float* const h_emb = reinterpret_cast<float*>(blk + o_emb);
  ws_window_slot_row* const gather = reinterpret_cast<ws_window_slot_row*>(blk + o_gather);
  ws_tail_emit_row* const emit = reinterpret_cast<ws_tail_emit_row*>(blk + o_emit);
  const long long stage = p->stage_off;       // floats
  size_t sp = 0;
  long long at = 0;                           // floats into the rows / estimates rectangles
  int r = 0;
  for (const TpPart* q : order) {
    const TpSlot& sl = p->sl[q->slot];
    const float* x = sl.pend.data() + (sl.pend.size() - size_t(q->L));
    memcpy(h_span + sp, x, size_t(q->L) * 4);
    float std_w = 1.0f;                       // TF-GridNet: the window scaled by its own standard deviation, its estimate back
    if (grid) row_std_scale(x, q->L, &std_w, nullptr);
    const int in = sl.flip, to = sl.flip ^ 1;
    for (int k = 0; k < K; ++k, ++r, at += q->L) {
      gather[r] = ws_window_slot_row{stage + (long long)(o_span / 4 + sp), p->rows_off + at, q->L, grid ? 1.0f / std_w : 1.0f};
      memcpy(h_emb + size_t(r) * E, sl.emb.data() + size_t(k) * E, size_t(E) * 4);
      emit[r] = ws_tail_emit_row{p->y_off + at,
                                 p->hold_off + (((long long)q->slot * 2 + in) * K + k) * C,
                                 p->hold_off + (((long long)q->slot * 2 + to) * K + k) * C,
                                 p->out_off + q->out_off + (long long)k * q->m,
                                 q->L, q->p, q->h, q->m, q->c_new, std_w};
    }
    sp += size_t(q->L);
  }
  int rc;
  char* const d_blk = p->state + size_t(stage) * 4;
  if ((rc = copy_async(e, kWho, "host-to-device copy", d_blk, blk, total, hipMemcpyHostToDevice)) != WS_OK) return rc;
  WS_RUN(e, ws_window_slots_fwd(gather, reinterpret_cast<const ws_window_slot_row*>(d_blk + o_gather), R, state, state_floats, state,
                                state_floats, e->stream));
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
                      : e->arch == 3 ? gridnet_device(e, in, Gn, L, d_emb + size_t(g0) * E, out)
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
  return WS_OK;
}

// the call's one copy to the host and its one synchronisation
int finish(ws_tail_pool* p, long long n_out) {
  ws_engine* e = p->e;
  int rc;
  p->out_host.assign(size_t(n_out), 0.f);
  ++e->n_launches;
  if ((rc = copy_async(e, kWho, "device-to-host copy", p->out_host.data(), reinterpret_cast<const float*>(p->state) + p->out_off,
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
  e->tail_pool_forwards = p->forwards, e->tail_pool_rows = p->rows;
  return WS_OK;
}

}  // namespace

WS_ENGINE_API int ws_engine_tail_pool_open(ws_engine* e, int slots, int K, int window, int fade, int warm, int max_rows,
                                           ws_tail_pool** out) {
  const char* who = "ws_engine_tail_pool_open";
  int rc = check_engine(e, who);
  if (rc != WS_OK) return rc;
  if (out) *out = nullptr;
  if (!out || K < 1) {
    set_err("%s: bad arguments (K=%d >= 1, out %s)", who, K, out ? "given" : "NULL");
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
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  ws_tail_pool* p = new ws_tail_pool();
  p->e = e, p->slots = slots, p->K = K, p->S = S, p->C = C, p->warm = warm, p->max_rows = max_rows;
  p->sl.resize(slots);
  // the staging block of the fullest tick: every slot with a full window; the copy table of a flush that only returns the hold
  p->stage_bytes = up256(size_t(slots) * S * 4) + up256(size_t(r_max) * e->E * 4) + up256(size_t(r_max) * sizeof(ws_window_slot_row)) +
                   up256(size_t(r_max) * sizeof(ws_tail_emit_row));
  p->stage_bytes = std::max(p->stage_bytes, up256(size_t(K) * sizeof(ws_rows_copy_row)));
  const size_t parts[7] = {size_t(slots) * 2 * K * C * 4, size_t(slots) * K * e->E * 4, p->stage_bytes,  size_t(r_max) * S * 4,
                           size_t(r_max) * S * 4,         size_t(r_max) * S * 4,        size_t(C) * 4};
  long long* at[7] = {&p->hold_off, &p->emb_off, &p->stage_off, &p->rows_off, &p->y_off, &p->out_off, &p->ramp_off};
  size_t total = 0;
  for (int i = 0; i < 7; ++i) *at[i] = static_cast<long long>(total / 4), total += up256(parts[i]);
  total = std::max<size_t>(total, 256);
  p->state_bytes = total;
  if (e->dry) {
    p->state = static_cast<char*>(malloc(total));
  } else if (hipMalloc(reinterpret_cast<void**>(&p->state), total) != hipSuccess) {
    p->state = nullptr;
  }
  if (!p->state) {
    set_err("%s: device allocation of %zu bytes failed", who, total);
    free_pool(p);
    return WS_ERR_LAUNCH;
  }
  if (e->work.poison && !e->dry) {      // WS_ENGINE_POISON (tests): state no launch has written reads as NaN
    (void)hipDeviceSynchronize();
    (void)hipMemset(p->state, 0xFF, total);
    (void)hipDeviceSynchronize();
  }
  // the ramp of the cross-fade, computed once: ramp[j] = float(j + 1) / float(C + 1)
  std::vector<float> ramp(static_cast<size_t>(C), 0.f);
  for (int j = 0; j < C; ++j) ramp[j] = static_cast<float>(j + 1) / static_cast<float>(C + 1);
  if (C > 0 && (rc = to_device(e, reinterpret_cast<float*>(p->state) + p->ramp_off, ramp.data(), size_t(C) * 4)) != WS_OK) {
    free_pool(p);
    return rc;
  }
  e->tail_pool_state_bytes = static_cast<long long>(total);
  e->tail_pool_forwards = e->tail_pool_rows = 0;
  *out = p;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_tail_pool_attach(ws_tail_pool* p, const void* enroll, int enroll_kind, int enroll_len, const int* enroll_lengths,
                                             int* slot) {
  const char* who = "ws_engine_tail_pool_attach";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  if (!enroll || !slot) {
    set_err("%s: bad arguments (enroll %s, slot %s)", who, enroll ? "given" : "NULL", slot ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  const int K = p->K;
  int Te = enroll_len;
  std::vector<int> te_row;
  if ((rc = long_check_group(e, static_cast<int>(std::min<long long>((long long)p->slots * K, p->max_rows)), p->S, K, enroll_kind, enroll_len,
                             enroll_lengths, &Te, &te_row)) != WS_OK)
    return rc;
  int id = 0;
  while (id < p->slots && p->sl[id].state != TpSlot::kFree) ++id;
  if (id == p->slots) {
    set_err("%s: the pool is full: all %d slots are attached (detach one, or open a larger pool)", who, p->slots);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  TpSlot fresh;
  fresh.emb.assign(size_t(K) * e->E, 0.f);
  float* d_emb = reinterpret_cast<float*>(p->state) + p->emb_off + size_t(id) * K * e->E;
  {
    ArenaScope scope(e->work);           // the speaker stage, once for this slot's K enrollments
    rc = speaker_stage(e, enroll, enroll_kind, K, enroll_len, Te, enroll_lengths, te_row.data(), d_emb);
    if (rc == WS_OK) rc = to_host(e, fresh.emb.data(), d_emb, fresh.emb.size() * 4);
  }
  if (rc != WS_OK) return rc;
  fresh.state = TpSlot::kAttached;
  p->sl[id] = std::move(fresh);         // at sample 0; the holds need no clearing (a hold is read after a firing wrote it)
  *slot = id;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_tail_pool_push(ws_tail_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n) {
  const char* who = "ws_engine_tail_pool_push";
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
    const TpSlot& sl = p->sl[id];
    if (sl.N + n[i] - sl.E > S) {        // what has not come out must fit one window
      set_err("%s: entry %d (slot %d): %d more samples make %lld that have not come out, a window holds %d: tick first", who, i, id, n[i],
              sl.N + n[i] - sl.E, S);
      return WS_ERR_INVALID;
    }
  }
  for (int i = 0; i < n_active; ++i) {  // no launch, no synchronisation: the samples wait on the host for the next tick
    TpSlot& sl = p->sl[slots[i]];
    sl.pend.insert(sl.pend.end(), chunks[i], chunks[i] + n[i]);
    sl.N += n[i];
    if (sl.pend.size() > size_t(S)) sl.pend.erase(sl.pend.begin(), sl.pend.end() - S);      // a window is the newest S samples
  }
  return WS_OK;
}

WS_ENGINE_API int ws_engine_tail_pool_tick(ws_tail_pool* p, int n_active, const int* slots, float* const* est, const int* est_cap,
                                           int* n_out) {
  const char* who = "ws_engine_tail_pool_tick";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  if (n_active < 1 || !slots || !est || !est_cap || !n_out) {
    set_err("%s: bad arguments (n_active=%d >= 1%s)", who, n_active, slots && est && est_cap && n_out ? "" : ", a NULL array");
    return WS_ERR_INVALID;
  }
  const int S = p->S, C = p->C, K = p->K;
  std::vector<char> seen(p->slots, 0);
  std::vector<TpPart> parts;
  long long total = 0;
  for (int i = 0; i < n_active; ++i) {
    const int id = slots[i];
    if ((rc = check_slot(p, who, id, i)) != WS_OK) return rc;
    if (seen[id]) {
      set_err("%s: slot %d is named twice (entry %d)", who, id, i);
      return WS_ERR_INVALID;
    }
    seen[id] = 1;
    const TpSlot& sl = p->sl[id];
    if (!fires(p, sl)) continue;
    TpPart q;
    q.slot = id, q.entry = i;
    q.L = static_cast<int>(std::min<long long>(sl.N, S));
    q.m = static_cast<int>(sl.N - C - sl.E), q.c_new = C, q.h = sl.fired ? C : 0;
    q.p = static_cast<int>(sl.E - (sl.N - q.L));
    if (q.m > est_cap[i] || (q.m > 0 && !est[i])) {
      set_err("%s: entry %d (slot %d) emits %d samples a row, est_cap is %d%s (WS_TAIL_CAP(S) = %d always suffices)", who, i, id, q.m,
              est_cap[i], est[i] ? "" : ", est is NULL", WS_TAIL_CAP(S));
      return WS_ERR_INVALID;
    }
    parts.push_back(q);
  }
  p->forwards = p->rows = 0;
  for (int i = 0; i < n_active; ++i) n_out[i] = 0;
  if (parts.empty()) {                  // no slot fires: no launch, no synchronisation
    e->n_launches = 0;
    e->tail_pool_forwards = e->tail_pool_rows = 0;
    return WS_OK;
  }
  std::sort(parts.begin(), parts.end(), [](const TpPart& a, const TpPart& b) { return a.slot < b.slot; });
  for (TpPart& q : parts) q.out_off = total, total += (long long)K * q.m;
  for (int i = 0; i < n_active; ++i) p->sl[slots[i]].failed = true;      // until the tick is complete
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  ArenaScope scope(e->work);
  if ((rc = run_windows(p, parts)) != WS_OK) return rc;
  if ((rc = finish(p, total)) != WS_OK) return rc;
  for (const TpPart& q : parts) {
    TpSlot& sl = p->sl[q.slot];
    if (!e->dry)
      for (int k = 0; k < K && q.m > 0; ++k)
        memcpy(est[q.entry] + size_t(k) * est_cap[q.entry], p->out_host.data() + q.out_off + (long long)k * q.m, size_t(q.m) * 4);
    sl.F = sl.N, sl.E = sl.N - C, sl.fired = true, sl.flip ^= 1;
    n_out[q.entry] = q.m;
  }
  for (int i = 0; i < n_active; ++i) p->sl[slots[i]].failed = false;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_tail_pool_flush(ws_tail_pool* p, int slot, float* est, int est_cap, int* n_out) {
  const char* who = "ws_engine_tail_pool_flush";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  if ((rc = check_slot(p, who, slot, -1)) != WS_OK) return rc;
  TpSlot& sl = p->sl[slot];
  const int S = p->S, C = p->C, K = p->K;
  const long long emitted = sl.N - sl.E;
  if (sl.N < 1) {
    set_err("%s: slot %d: nothing was pushed", who, slot);
    return WS_ERR_INVALID;
  }
  if (!est || !n_out || emitted > est_cap) {
    set_err("%s: slot %d: the flush emits %lld samples a row, est_cap is %d%s (WS_TAIL_CAP(S) = %d always suffices)", who, slot, emitted,
            est_cap, est && n_out ? "" : ", est or n_out is NULL", WS_TAIL_CAP(S));
    return WS_ERR_INVALID;
  }
  const bool window_due = !sl.fired || sl.N > sl.F;
  const int L = static_cast<int>(std::min<long long>(sl.N, S));
  // a last window shorter than S has the architecture's own lower bound on T; refused before anything runs, so a later push
  // goes on from here
  if (window_due && L < S && (rc = check_rows(e, true, K < p->max_rows ? K : p->max_rows, L)) != WS_OK) return rc;
  p->forwards = p->rows = 0;
  if (emitted == 0) {                   // fade 0 and nothing new since the last firing: nothing is left to come out
    e->n_launches = 0;
    e->tail_pool_forwards = e->tail_pool_rows = 0;
    sl.pend.clear();
    sl.state = TpSlot::kDone;
    *n_out = 0;
    return WS_OK;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  sl.failed = true;
  ArenaScope scope(e->work);
  if (window_due) {                     // one last window, all of it from E on comes out; no new hold
    TpPart q;
    q.slot = slot, q.L = L, q.m = static_cast<int>(emitted), q.c_new = 0, q.h = sl.fired ? C : 0;
    q.p = static_cast<int>(sl.E - (sl.N - L));
    if ((rc = run_windows(p, std::vector<TpPart>(1, q))) != WS_OK) return rc;
  } else {                              // N == F: the hold as it is -- a copy, no forward
    p->keep.emplace_back(size_t(K) * sizeof(ws_rows_copy_row), char(0));
    ws_rows_copy_row* tab = reinterpret_cast<ws_rows_copy_row*>(p->keep.back().data());
    for (int k = 0; k < K; ++k)
      tab[k] = ws_rows_copy_row{p->hold_off + (((long long)slot * 2 + sl.flip) * K + k) * C, p->out_off + (long long)k * C, C, 0};
    char* const d_blk = p->state + size_t(p->stage_off) * 4;
    float* const state = reinterpret_cast<float*>(p->state);
    const long long state_floats = static_cast<long long>(p->state_bytes / 4);
    if ((rc = copy_async(e, kWho, "host-to-device copy", d_blk, tab, size_t(K) * sizeof(ws_rows_copy_row), hipMemcpyHostToDevice)) != WS_OK)
      return rc;
    WS_RUN(e, ws_rows_copy_fwd(tab, reinterpret_cast<const ws_rows_copy_row*>(d_blk), K, state, state_floats, state, state_floats, e->stream));
  }
  if ((rc = finish(p, (long long)K * emitted)) != WS_OK) return rc;
  if (!e->dry)
    for (int k = 0; k < K; ++k) memcpy(est + size_t(k) * est_cap, p->out_host.data() + k * emitted, size_t(emitted) * 4);
  sl.E = sl.F = sl.N;
  sl.pend.clear();
  sl.failed = false;
  sl.state = TpSlot::kDone;
  *n_out = static_cast<int>(emitted);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_tail_pool_detach(ws_tail_pool* p, int slot) {
  const char* who = "ws_engine_tail_pool_detach";
  const int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  if (slot < 0 || slot >= p->slots || p->sl[slot].state == TpSlot::kFree) {
    set_err("%s: slot %d is not attached (the pool has %d slots)", who, slot, p->slots);
    return WS_ERR_INVALID;
  }
  if (p->sl[slot].failed) {              // a call that failed half way may have left work behind that reads this slot's holds
    ForwardTurn turn(p->e);
    if (turn.rc != WS_OK) return turn.rc;
    (void)sync_stream(p->e, kWho);
    p->keep.clear();
  }
  p->sl[slot] = TpSlot();               // free, and no longer the slot of a half-finished call
  return WS_OK;
}

WS_ENGINE_API void ws_engine_tail_pool_close(ws_tail_pool* p) {
  if (!p) return;
  if (p->e && !p->e->dry) {
    (void)hipSetDevice(p->e->device);
    (void)hipStreamSynchronize(p->e->stream);
  }
  free_pool(p);
}
