// =================================================================================================================
// Live pool (ws_engine_live_pool_*; DESIGN 7 "Live pool" and 11b): MANY live recordings (live.cc) on one engine, the windows
// that one push completes -- in whatever slot -- through the separator in the same forwards.  A slot is a live handle's
// bookkeeping: its own position, its own packet sizes, its own K enrollments, the emission rule of ws_engine_live_*.
//   * the state is ONE device allocation made at open, a function of (slots, K, S, O, max_rows): per slot the ring
//     [K][cap][S] of window estimates (cap = g_max + 3, g_max = max(1, max_rows / K)), the ring of TF-GridNet's factors and the
//     K embeddings; per round the staging block (the slots' spans, the factors, the embedding rows, the three tables), the
//     rows rectangle and the estimates rectangle.  Pending samples (fewer than S + H a slot between pushes) live on the host;
//   * a push appends every packet, then works in rounds: in ascending slot order every slot that still owes windows gives
//     min(owed, g_max, cap - Wr % cap) consecutive windows -- the solo handle's cut.  A round is one upload of its staging
//     block, ONE ws_window_slots_fwd for all of its rows (ordered slot, target, window), the architecture's rectangular plan
//     in forwards of at most max_rows rows whichever slots they came from, ONE ws_rows_copy_fwd of the estimates (and
//     factors) into the rings and ONE ws_xfade_stream_rows_fwd for what the round made final.  After the last round one copy
//     to the host and ONE synchronisation;
//   * transient activations come from the engine's work arena under an ArenaScope; nothing of it is held between two calls.
//   * store / run / due: store appends packets and launches nothing, run works off every complete window of the slots it names
//     (and ends the recordings marked final) in the same rounds, due tells a scheduler what waits.  push is store + run of its
//     slots, flush is run with its slot final: one path, run_jobs, serves all of them.  A final recording's end-aligned last
//     window is a row of S samples like any other; a short one (n < S) gets forwards of its own rows behind the round's S rows.
// No launch mixes rows: a slot's samples do not depend on what the other slots carry.
// =================================================================================================================
#include <deque>

#include "engine_internal.h"

using namespace wsrt;

namespace {

struct LpSlot {
  enum State { kFree, kAttached, kDone } state = kFree;
  bool failed = false;                  // a push or flush that named this slot ended half way
  std::vector<float> pend;              // the samples from `base` on
  std::vector<float> emb;               // [K][E], host copy of the slot's embeddings
  long long base = 0, N = 0, Wr = 0, E = 0;     // samples pushed, windows run, samples emitted
};

// what one slot gives to one round: g windows of L samples from the host span x, the first with index w0 (g = 0: none), and
// the range [i0, i0 + count) that the round makes final, written at d_out + out_off with row pitch ld
struct LpPart {
  int slot = 0, g = 0, L = 0;
  long long w0 = 0;
  const float* x = nullptr;
  long long i0 = 0, count = 0, windows_run = 0, W = 0, n = 0, out_off = 0, ld = 0;
  int final = 0, job = 0;
};

// what a call does for one slot it names: the regular windows up to wr_new, then (final) the end of the recording; `emitted`
// samples a target come out, into est [K][cap], at out_base of the call's block
struct LpJob {
  int slot = 0, final = 0, cap = 0;
  bool ended = false;
  long long wr_new = 0, e0 = 0, emitted = 0, out_base = 0;
  float* est = nullptr;
};

}  // namespace

struct ws_live_pool {
  ws_engine* e = nullptr;
  int slots = 0, K = 0, S = 0, O = 0, H = 0, max_rows = 0, g_max = 0, cap = 0;
  long long r_max = 0;                  // rows of the fullest round: slots K g_max
  char* state = nullptr;
  size_t state_bytes = 0, stage_bytes = 0;
  // float offsets into the state of its parts: rings [slots][K][cap][S], factor rings [slots][cap], embeddings [slots][K][E],
  // the staging block, the rows rectangle [r_max][S], the estimates rectangle [r_max][S]
  long long ring_off = 0, scale_off = 0, emb_off = 0, stage_off = 0, rows_off = 0, y_off = 0;
  std::vector<LpSlot> sl;
  std::deque<std::vector<char>> hold;   // host sources of the call's asynchronous uploads, alive until its synchronisation
  std::vector<float> out_host;          // the call's estimates, one block
  long long rounds = 0, forwards = 0;
};

namespace {

constexpr const char* kWho = "ws_engine_live_pool";

size_t up256(size_t b) { return Arena::round_up(b); }

int check_pool(const ws_live_pool* p, const char* who) {
  if (!p || !p->e) {
    set_err("%s: null pool", who);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

// attached, not flushed, not the slot of a call that failed half way
int check_slot(const ws_live_pool* p, const char* who, int id, int entry) {
  char where[48] = "";
  if (entry >= 0) snprintf(where, sizeof where, " (entry %d)", entry);
  if (id < 0 || id >= p->slots || p->sl[id].state == LpSlot::kFree)
    set_err("%s: slot %d%s is not attached (the pool has %d slots)", who, id, where, p->slots);
  else if (p->sl[id].failed)
    set_err("%s: slot %d%s took part in a call that failed half way; detach it", who, id, where);
  else if (p->sl[id].state == LpSlot::kDone)
    set_err("%s: slot %d%s was flushed (detach it, then attach the next recording)", who, id, where);
  else
    return WS_OK;
  return WS_ERR_INVALID;
}

void free_pool(ws_live_pool* p) {
  if (p->state) {
    if (p->e->dry)
      free(p->state);
    else
      (void)hipFree(p->state);
  }
  delete p;
}

// One round.  The staging block -- spans | factors | embedding rows | gather table | scatter table | cross-fade table, each
// part 256-byte aligned -- is built on the host and uploaded once.  The rows of S samples come first, ordered (slot, target,
// window), and go through the separator in forwards of at most max_rows rows whichever slots they came from; the rows of a
// short final recording (L < S) follow, each recording's in forwards of their own (one length a forward).
int run_round(ws_live_pool* p, const std::vector<LpPart>& parts, float* d_out, long long n_out) {
  ws_engine* e = p->e;
  const int K = p->K, S = p->S, H = p->H, cap = p->cap, E = e->E;
  const bool grid = e->arch == 3;
  float* const state = reinterpret_cast<float*>(p->state);
  const long long state_floats = static_cast<long long>(p->state_bytes / 4);
  int R = 0, n_fac = 0, n_scatter = 0, n_fade = 0;
  size_t span_floats = 0;
  std::vector<const LpPart*> ord;         // full-length parts (and those without a window), then the short ones
  for (const LpPart& q : parts)
    if (q.g == 0 || q.L == S) ord.push_back(&q);
  for (const LpPart& q : parts)
    if (q.g > 0 && q.L != S) ord.push_back(&q);
  for (const LpPart& q : parts) {
    if (q.g > 0) {
      R += K * q.g, n_fac += q.g, n_scatter += K + (grid ? 1 : 0);
      span_floats += size_t(q.g - 1) * H + q.L;
    }
    n_fade += K;
  }
  // the block's layout, in bytes from its start
  const size_t o_span = 0, o_fac = o_span + up256(span_floats * 4), o_emb = o_fac + up256(size_t(n_fac) * 4),
               o_gather = o_emb + up256(size_t(R) * E * 4), o_scatter = o_gather + up256(size_t(R) * sizeof(ws_window_slot_row)),
               o_fade = o_scatter + up256(size_t(n_scatter) * sizeof(ws_rows_copy_row)),
               total = o_fade + up256(size_t(n_fade) * sizeof(ws_xfade_stream_row));
  if (total > p->stage_bytes) {
    set_err("%s: a round needs %zu bytes of staging, the state holds %zu", kWho, total, p->stage_bytes);
    return WS_ERR_LAUNCH;
  }
  p->hold.emplace_back(total, char(0));
  char* const blk = p->hold.back().data();
  float* const h_span = reinterpret_cast<float*>(blk + o_span);
  float* const h_fac = reinterpret_cast<float*>(blk + o_fac);
  float* const h_emb = reinterpret_cast<float*>(blk + o_emb);
  ws_window_slot_row* const gather = reinterpret_cast<ws_window_slot_row*>(blk + o_gather);
  ws_rows_copy_row* const scatter = reinterpret_cast<ws_rows_copy_row*>(blk + o_scatter);
  ws_xfade_stream_row* const fade = reinterpret_cast<ws_xfade_stream_row*>(blk + o_fade);
  const long long stage = p->stage_off;       // floats
  struct Seg { int r0, rows, L; long long at; };      // a run of rows of one length: first row, count, float offset in the rectangles
  std::vector<Seg> segs;
  size_t sp = 0;
  long long at = 0;                            // floats of the rows and estimates rectangles used so far
  int r = 0, fc = 0, sc = 0, fd = 0;
  for (const LpPart* qp : ord) {
    const LpPart& q = *qp;
    const LpSlot& sl = p->sl[q.slot];
    const long long ring0 = p->ring_off + (long long)q.slot * K * cap * S, fac_ring = p->scale_off + (long long)q.slot * cap;
    if (q.g > 0) {
      const int slot0 = static_cast<int>(q.w0 % cap);
      const size_t n_span = size_t(q.g - 1) * H + q.L;
      if (q.L == S && !segs.empty())
        segs.back().rows += K * q.g;
      else
        segs.push_back(Seg{r, K * q.g, q.L, at});
      memcpy(h_span + sp, q.x, n_span * 4);
      for (int w = 0; w < q.g; ++w) {      // TF-GridNet: every window scaled by its own standard deviation, its estimate back
        if (grid) row_std_scale(q.x + size_t(w) * H, q.L, &h_fac[fc + w], nullptr);
      }
      for (int k = 0; k < K; ++k) {
        scatter[sc++] = ws_rows_copy_row{p->y_off + at, ring0 + ((long long)k * cap + slot0) * S, q.g * q.L, 0};
        for (int w = 0; w < q.g; ++w, ++r, at += q.L) {
          gather[r] = ws_window_slot_row{stage + (long long)(o_span / 4 + sp) + (long long)w * H, p->rows_off + at, q.L,
                                         grid ? 1.0f / h_fac[fc + w] : 1.0f};
          memcpy(h_emb + size_t(r) * E, sl.emb.data() + size_t(k) * E, size_t(E) * 4);
        }
      }
      if (grid) scatter[sc++] = ws_rows_copy_row{stage + (long long)(o_fac / 4) + fc, fac_ring + slot0, q.g, 0};
      sp += n_span, fc += q.g;
    }
    for (int k = 0; k < K; ++k)
      fade[fd++] = ws_xfade_stream_row{ring0 + (long long)k * cap * S, grid ? fac_ring : -1LL, q.out_off + k * q.ld, q.i0, q.count,
                                       q.windows_run, q.W, q.n, q.final};
  }
  int rc;
  char* const d_blk = p->state + size_t(stage) * 4;
  if ((rc = copy_async(e, kWho, "host-to-device copy", d_blk, blk, total, hipMemcpyHostToDevice)) != WS_OK) return rc;
  if (R > 0) {
    WS_RUN(e, ws_window_slots_fwd(gather, reinterpret_cast<const ws_window_slot_row*>(d_blk + o_gather), R, state, state_floats, state,
                                  state_floats, e->stream));
    Arena& a = e->work;
    const float* d_emb = reinterpret_cast<const float*>(d_blk + o_emb);
    const Arena::Mark mk = a.mark();
    for (const Seg& sg : segs) {
      const float* d_rows = state + p->rows_off + sg.at;
      float* d_y = state + p->y_off + sg.at;
      const int L = sg.L, G = sg.rows < p->max_rows ? sg.rows : p->max_rows;
      for (int r0 = 0; r0 < sg.rows; r0 += G) {
        const int Gn = sg.rows - r0 < G ? sg.rows - r0 : G;
        a.release(mk);
        const float* in = d_rows + size_t(r0) * L;
        float* out = d_y + size_t(r0) * L;
        const float* emb = d_emb + size_t(sg.r0 + r0) * E;
        rc = e->arch == 1   ? tasnet_device(e, in, Gn, L, emb, nullptr, 0, out)
             : e->arch == 2 ? dpccn_device(e, in, Gn, L, emb, out)
             : e->arch == 3 ? gridnet_device(e, in, Gn, L, emb, out)
                            : separate_device(e, in, Gn, L, emb, out);
        if (rc != WS_OK) return rc;
        ++p->forwards;
      }
    }
    a.release(mk);
    WS_RUN(e, ws_rows_copy_fwd(scatter, reinterpret_cast<const ws_rows_copy_row*>(d_blk + o_scatter), n_scatter, state, state_floats, state,
                               state_floats, e->stream));
  }
  WS_RUN(e, ws_xfade_stream_rows_fwd(fade, reinterpret_cast<const ws_xfade_stream_row*>(d_blk + o_fade), n_fade, S, p->O, cap, state,
                                     state_floats, state, state_floats, d_out, n_out, e->stream));
  ++p->rounds;
  return WS_OK;
}

// the call's one copy to the host and its one synchronisation
int finish(ws_live_pool* p, const float* d_out, long long n_out) {
  ws_engine* e = p->e;
  int rc;
  p->out_host.assign(size_t(n_out), 0.f);
  ++e->n_launches;
  if ((rc = copy_async(e, kWho, "device-to-host copy", p->out_host.data(), d_out, size_t(n_out) * 4, hipMemcpyDeviceToHost)) != WS_OK) return rc;
  unsigned timed_out = 0;                // did a cluster recurrence time out (note_cluster_status)?  read in the same wait
  if (e->cl_status && (rc = copy_async(e, kWho, "device-to-host copy", &timed_out, e->cl_status, 4, hipMemcpyDeviceToHost)) != WS_OK) return rc;
  if ((rc = sync_stream(e, kWho)) != WS_OK) return rc;
  if (timed_out) {
    ++e->cluster_fallbacks;
    if ((rc = zero_device(e, e->cl_status, 4)) != WS_OK) return rc;
  }
  p->hold.clear();
  e->live_pool_rounds = p->rounds, e->live_pool_forwards = p->forwards;
  return WS_OK;
}

}  // namespace

WS_ENGINE_API int ws_engine_live_pool_open(ws_engine* e, int slots, int K, int window, int overlap, int max_rows, ws_live_pool** out) {
  const char* who = "ws_engine_live_pool_open";
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
  // exactly what ws_engine_separate_long demands, with its messages
  if ((rc = long_check_window(e, window, overlap, max_rows)) != WS_OK) return rc;
  const int S = window, H = S - overlap, g_max = std::max(1, max_rows / K), cap = g_max + 3;
  const long long r_max = (long long)slots * K * g_max;
  if (r_max + slots > 65535) {
    set_err("%s: %d slots x %d speakers x %d windows = %lld rows in a round, the tables of a launch hold 65535 with one more a slot", who,
            slots, K, g_max, r_max);
    return WS_ERR_INVALID;
  }
  if ((rc = check_rows(e, true, static_cast<int>(std::min<long long>(r_max, max_rows)), S)) != WS_OK) return rc;
  if ((long long)(g_max - 1) * H + S > 0x7fffffffLL || (long long)K * g_max * S > 0x7fffffffLL) {
    set_err("%s: a group of %d windows of %d samples for %d speakers: more samples than an int holds", who, g_max, S, K);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  ws_live_pool* p = new ws_live_pool();
  p->e = e, p->slots = slots, p->K = K, p->S = S, p->O = overlap, p->H = H, p->max_rows = max_rows, p->g_max = g_max, p->cap = cap;
  p->r_max = r_max;
  p->sl.resize(slots);
  // the staging block of the fullest round: every slot with g_max windows
  p->stage_bytes = up256(size_t(slots) * (size_t(g_max - 1) * H + S) * 4) + up256(size_t(slots) * g_max * 4) + up256(size_t(r_max) * e->E * 4) +
                   up256(size_t(r_max) * sizeof(ws_window_slot_row)) + up256(size_t(slots) * (K + 1) * sizeof(ws_rows_copy_row)) +
                   up256(size_t(slots) * K * sizeof(ws_xfade_stream_row));
  const size_t parts[6] = {size_t(slots) * K * cap * S * 4, size_t(slots) * cap * 4, size_t(slots) * K * e->E * 4,
                           p->stage_bytes,                   size_t(r_max) * S * 4,   size_t(r_max) * S * 4};
  long long* at[6] = {&p->ring_off, &p->scale_off, &p->emb_off, &p->stage_off, &p->rows_off, &p->y_off};
  size_t total = 0;
  for (int i = 0; i < 6; ++i) *at[i] = static_cast<long long>(total / 4), total += up256(parts[i]);
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
  e->live_pool_state_bytes = static_cast<long long>(total);
  e->live_pool_rounds = e->live_pool_forwards = 0;
  *out = p;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_live_pool_attach(ws_live_pool* p, const void* enroll, int enroll_kind, int enroll_len, const int* enroll_lengths,
                                             int* slot) {
  const char* who = "ws_engine_live_pool_attach";
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
  if ((rc = long_check_group(e, static_cast<int>(std::min<long long>(p->r_max, p->max_rows)), p->S, K, enroll_kind, enroll_len, enroll_lengths,
                             &Te, &te_row)) != WS_OK)
    return rc;
  int id = 0;
  while (id < p->slots && p->sl[id].state != LpSlot::kFree) ++id;
  if (id == p->slots) {
    set_err("%s: the pool is full: all %d slots are attached (detach one, or open a larger pool)", who, p->slots);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  LpSlot fresh;
  fresh.emb.assign(size_t(K) * e->E, 0.f);
  float* d_emb = reinterpret_cast<float*>(p->state) + p->emb_off + size_t(id) * K * e->E;
  {
    ArenaScope scope(e->work);           // the speaker stage, once for this slot's K enrollments
    rc = speaker_stage(e, enroll, enroll_kind, K, enroll_len, Te, enroll_lengths, te_row.data(), d_emb);
    if (rc == WS_OK) rc = to_host(e, fresh.emb.data(), d_emb, fresh.emb.size() * 4);
  }
  if (rc != WS_OK) return rc;
  fresh.state = LpSlot::kAttached;
  p->sl[id] = std::move(fresh);         // at sample 0; the rings need no clearing (a slot is read for a covering window only)
  *slot = id;
  return WS_OK;
}

namespace {

// one entry of a push or a store: an attached slot named once, a packet of n >= 1 samples
int check_packet(const ws_live_pool* p, const char* who, int i, int id, std::vector<char>& seen, const float* chunk, int n) {
  int rc;
  if ((rc = check_slot(p, who, id, i)) != WS_OK) return rc;
  if (seen[id]) {
    set_err("%s: slot %d is named twice (entry %d): one packet a slot in a push", who, id, i);
    return WS_ERR_INVALID;
  }
  if (n < 1 || !chunk) {
    set_err("%s: entry %d (slot %d): n=%d >= 1, chunk %s", who, i, id, n, chunk ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  seen[id] = 1;
  return WS_OK;
}

void append(ws_live_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n) {
  for (int i = 0; i < n_active; ++i) {
    LpSlot& sl = p->sl[slots[i]];
    sl.pend.insert(sl.pend.end(), chunks[i], chunks[i] + n[i]);
    sl.N += n[i];
  }
}

// The one path of push, flush and run.  Every job is checked by its caller.  Rounds: in ascending slot order a job that still
// owes regular windows gives the solo cut of them; a final job that owes none gives the end of its recording -- the short
// window, the end-aligned last window or no window at all -- with the final cross-fade, once.  Nothing to do in any job: no
// launch, no synchronisation.
int run_jobs(ws_live_pool* p, std::vector<LpJob>& jobs, int* n_out) {
  ws_engine* e = p->e;
  const int S = p->S, H = p->H, K = p->K, A = static_cast<int>(jobs.size());
  int rc;
  long long total = 0;
  bool any = false;
  for (LpJob& j : jobs) {
    j.out_base = total;
    total += (long long)K * j.emitted;
    any = any || j.final || j.wr_new > p->sl[j.slot].Wr;
  }
  p->rounds = p->forwards = 0;
  if (!any) {                           // no window became complete in any slot: no launch, no synchronisation
    e->n_launches = 0;
    e->live_pool_rounds = e->live_pool_forwards = 0;
    for (int i = 0; i < A; ++i) n_out[i] = 0;
    return WS_OK;
  }
  std::vector<int> order(A);
  for (int i = 0; i < A; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return jobs[a].slot < jobs[b].slot; });
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  for (const LpJob& j : jobs) p->sl[j.slot].failed = true;      // until the call is complete
  e->n_launches = 0;
  ArenaScope scope(e->work);
  const long long n_dev = std::max<long long>(total, 1);
  float* d_out = e->work.alloc(size_t(n_dev));
  WS_PTR(d_out);
  while (true) {
    std::vector<LpPart> parts;
    for (int i : order) {
      LpJob& j = jobs[i];
      LpSlot& sl = p->sl[j.slot];
      LpPart q;
      q.slot = j.slot, q.job = i, q.L = S;
      q.i0 = sl.E, q.ld = j.emitted, q.out_off = j.out_base + (sl.E - j.e0);
      if (sl.Wr < j.wr_new) {
        q.w0 = sl.Wr;
        q.g = live_cut(sl.Wr, j.wr_new, p->g_max, p->cap);
        q.x = sl.pend.data() + (sl.Wr * H - sl.base);
        q.windows_run = sl.Wr + q.g;
        q.count = (q.windows_run - 1) * H - sl.E;
      } else if (j.final && !j.ended) {
        const long long n = sl.N;
        q.W = sl.Wr;
        if (n < S) {
          q.g = 1, q.w0 = 0, q.L = static_cast<int>(n), q.x = sl.pend.data(), q.W = 1;
        } else if ((n - S) % H != 0) {    // the end-aligned last window, index W - 1
          q.g = 1, q.w0 = sl.Wr, q.x = sl.pend.data() + (n - S - sl.base), q.W = sl.Wr + 1;
        }
        q.windows_run = q.W, q.n = n, q.final = 1;
        q.count = n - sl.E;
      } else {
        continue;
      }
      parts.push_back(q);
    }
    if (parts.empty()) break;
    if ((rc = run_round(p, parts, d_out, n_dev)) != WS_OK) return rc;
    for (const LpPart& q : parts) {
      LpSlot& sl = p->sl[q.slot];
      sl.Wr = q.windows_run;
      sl.E = q.final ? q.n : (sl.Wr - 1) * H;
      if (q.final) jobs[q.job].ended = true;
    }
  }
  if ((rc = finish(p, d_out, total)) != WS_OK) return rc;
  for (int i = 0; i < A; ++i) {
    const LpJob& j = jobs[i];
    LpSlot& sl = p->sl[j.slot];
    if (!e->dry)
      for (int k = 0; k < K && j.emitted > 0; ++k)
        memcpy(j.est + size_t(k) * j.cap, p->out_host.data() + j.out_base + k * j.emitted, size_t(j.emitted) * 4);
    if (j.final) {
      sl.pend.clear();
      sl.state = LpSlot::kDone;
    } else {                            // what a later window can still read starts at the newest window's start
      sl.pend.erase(sl.pend.begin(), sl.pend.begin() + static_cast<ptrdiff_t>(sl.E - sl.base));
      sl.base = sl.E;
    }
    sl.failed = false;
    n_out[i] = static_cast<int>(j.emitted);
  }
  return WS_OK;
}

// the end of slot id's recording as a job: flush's checks, under who's name
int final_job(const ws_live_pool* p, const char* who, int id, int entry, float* est, int est_cap, bool outs, LpJob* j) {
  const LpSlot& sl = p->sl[id];
  const int S = p->S, H = p->H, K = p->K;
  const long long n = sl.N, emitted = n - sl.E;
  int rc;
  if (n < 1) {
    set_err("%s: slot %d: nothing was pushed", who, id);
    return WS_ERR_INVALID;
  }
  if (entry >= 0 && (!est || emitted > est_cap)) {      // a run: its backlog may exceed what a flush after pushes emits
    set_err("%s: entry %d (slot %d) emits %lld samples a row, est_cap is %d%s (WS_LIVE_POOL_RUN_CAP(S, H) = %lld always suffices)", who, entry,
            id, emitted, est_cap, est ? "" : ", est is NULL", (long long)WS_LIVE_POOL_RUN_CAP((long long)S, H));
    return WS_ERR_INVALID;
  }
  if (!est || !outs || emitted > est_cap) {
    set_err("%s: slot %d: the flush emits %lld samples a row, est_cap is %d%s (WS_LIVE_FLUSH_CAP(S, O) = %d always suffices)", who, id,
            emitted, est_cap, est && outs ? "" : ", est or n_out is NULL", WS_LIVE_FLUSH_CAP(S, p->O));
    return WS_ERR_INVALID;
  }
  // n < S: the whole recording is one short row with the architecture's own lower bound on T; refused before anything runs,
  // so a later push goes on from here
  if (n < S && (rc = check_rows(p->e, true, K < p->max_rows ? K : p->max_rows, static_cast<int>(n))) != WS_OK) return rc;
  j->slot = id, j->final = 1, j->cap = est_cap, j->est = est;
  j->wr_new = live_windows_run(n, S, H), j->e0 = sl.E, j->emitted = emitted;
  return WS_OK;
}

}  // namespace

WS_ENGINE_API int ws_engine_live_pool_push(ws_live_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n,
                                           float* const* est, const int* est_cap, int* n_out) {
  const char* who = "ws_engine_live_pool_push";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  if (n_active < 1 || !slots || !chunks || !n || !est || !est_cap || !n_out) {
    set_err("%s: bad arguments (n_active=%d >= 1%s)", who, n_active, slots && chunks && n && est && est_cap && n_out ? "" : ", a NULL array");
    return WS_ERR_INVALID;
  }
  const int S = p->S, H = p->H;
  std::vector<char> seen(p->slots, 0);
  std::vector<LpJob> jobs(n_active);
  for (int i = 0; i < n_active; ++i) {
    const int id = slots[i];
    if ((rc = check_packet(p, who, i, id, seen, chunks[i], n[i])) != WS_OK) return rc;
    const LpSlot& sl = p->sl[id];
    LpJob& j = jobs[i];
    j.slot = id, j.cap = est_cap[i], j.est = est[i];
    j.wr_new = live_windows_run(sl.N + n[i], S, H);
    j.e0 = sl.E;
    j.emitted = live_emitted(j.wr_new, H) - sl.E;
    if (j.emitted > est_cap[i] || (j.emitted > 0 && !est[i])) {
      set_err("%s: entry %d (slot %d) emits %lld samples a row, est_cap is %d%s (WS_LIVE_PUSH_CAP(n, H) = %lld always suffices)", who, i, id,
              j.emitted, est_cap[i], est[i] ? "" : ", est is NULL", (long long)WS_LIVE_PUSH_CAP((long long)n[i], H));
      return WS_ERR_INVALID;
    }
  }
  append(p, n_active, slots, chunks, n);       // all packets first
  return run_jobs(p, jobs, n_out);
}

WS_ENGINE_API int ws_engine_live_pool_store(ws_live_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n) {
  const char* who = "ws_engine_live_pool_store";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  if (n_active < 1 || !slots || !chunks || !n) {
    set_err("%s: bad arguments (n_active=%d >= 1%s)", who, n_active, slots && chunks && n ? "" : ", a NULL array");
    return WS_ERR_INVALID;
  }
  const long long limit = WS_LIVE_POOL_STORE_LIMIT((long long)p->S, p->H);
  std::vector<char> seen(p->slots, 0);
  for (int i = 0; i < n_active; ++i) {
    const int id = slots[i];
    if ((rc = check_packet(p, who, i, id, seen, chunks[i], n[i])) != WS_OK) return rc;
    const long long pending = (long long)p->sl[id].pend.size() + n[i];
    if (pending >= limit) {              // the backlog is bounded: what a run gives back fits WS_LIVE_POOL_RUN_CAP
      set_err("%s: entry %d (slot %d): %d more samples make %lld pending, WS_LIVE_POOL_STORE_LIMIT(S, H) = %lld: run first", who, i, id, n[i],
              pending, limit);
      return WS_ERR_INVALID;
    }
  }
  append(p, n_active, slots, chunks, n);       // no launch, no synchronisation: the samples wait on the host for a run
  p->rounds = p->forwards = 0;
  p->e->n_launches = 0;
  p->e->live_pool_rounds = p->e->live_pool_forwards = 0;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_live_pool_run(ws_live_pool* p, int n_active, const int* slots, const int* final, float* const* est,
                                          const int* est_cap, int* n_out) {
  const char* who = "ws_engine_live_pool_run";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  if (n_active < 1 || !slots || !est || !est_cap || !n_out) {
    set_err("%s: bad arguments (n_active=%d >= 1%s)", who, n_active, slots && est && est_cap && n_out ? "" : ", a NULL array");
    return WS_ERR_INVALID;
  }
  const int S = p->S, H = p->H;
  std::vector<char> seen(p->slots, 0);
  std::vector<LpJob> jobs(n_active);
  for (int i = 0; i < n_active; ++i) {
    const int id = slots[i];
    if ((rc = check_slot(p, who, id, i)) != WS_OK) return rc;
    if (seen[id]) {
      set_err("%s: slot %d is named twice (entry %d): one entry a slot in a run", who, id, i);
      return WS_ERR_INVALID;
    }
    seen[id] = 1;
    const LpSlot& sl = p->sl[id];
    LpJob& j = jobs[i];
    if (final && final[i]) {
      if ((rc = final_job(p, who, id, i, est[i], est_cap[i], true, &j)) != WS_OK) return rc;
      continue;
    }
    j.slot = id, j.cap = est_cap[i], j.est = est[i];
    j.wr_new = live_windows_run(sl.N, S, H);
    j.e0 = sl.E;
    j.emitted = live_emitted(j.wr_new, H) - sl.E;
    if (j.emitted > est_cap[i] || (j.emitted > 0 && !est[i])) {
      set_err("%s: entry %d (slot %d) emits %lld samples a row, est_cap is %d%s (WS_LIVE_POOL_RUN_CAP(S, H) = %lld always suffices)", who, i, id,
              j.emitted, est_cap[i], est[i] ? "" : ", est is NULL", (long long)WS_LIVE_POOL_RUN_CAP((long long)S, H));
      return WS_ERR_INVALID;
    }
  }
  return run_jobs(p, jobs, n_out);
}

WS_ENGINE_API int ws_engine_live_pool_due(ws_live_pool* p, long long* rows_ready, long long* oldest_age) {
  const char* who = "ws_engine_live_pool_due";
  const int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  long long windows = 0, age = 0;
  for (const LpSlot& sl : p->sl) {       // the slots a run takes: attached, not ended, not part of a failed call
    if (sl.state != LpSlot::kAttached || sl.failed) continue;
    const long long ready = live_windows_run(sl.N, p->S, p->H) - sl.Wr;
    if (ready < 1) continue;
    windows += ready;
    age = std::max(age, sl.N - (sl.Wr * p->H + p->S));
  }
  if (rows_ready) *rows_ready = p->K * windows;
  if (oldest_age) *oldest_age = age;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_live_pool_flush(ws_live_pool* p, int slot, float* est, int est_cap, int* n_out) {
  const char* who = "ws_engine_live_pool_flush";
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  if ((rc = check_slot(p, who, slot, -1)) != WS_OK) return rc;
  std::vector<LpJob> jobs(1);
  if ((rc = final_job(p, who, slot, -1, est, est_cap, n_out != nullptr, &jobs[0])) != WS_OK) return rc;
  return run_jobs(p, jobs, n_out);
}

WS_ENGINE_API int ws_engine_live_pool_detach(ws_live_pool* p, int slot) {
  const char* who = "ws_engine_live_pool_detach";
  const int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  if (slot < 0 || slot >= p->slots || p->sl[slot].state == LpSlot::kFree) {
    set_err("%s: slot %d is not attached (the pool has %d slots)", who, slot, p->slots);
    return WS_ERR_INVALID;
  }
  if (p->sl[slot].failed) {              // a call that failed half way may have left work behind that reads this slot's rings
    ForwardTurn turn(p->e);
    if (turn.rc != WS_OK) return turn.rc;
    (void)sync_stream(p->e, kWho);
    p->hold.clear();
  }
  p->sl[slot] = LpSlot();               // free, and no longer the slot of a half-finished call
  return WS_OK;
}

WS_ENGINE_API void ws_engine_live_pool_close(ws_live_pool* p) {
  if (!p) return;
  if (p->e && !p->e->dry) {
    (void)hipSetDevice(p->e->device);
    (void)hipStreamSynchronize(p->e->stream);
  }
  free_pool(p);
}
