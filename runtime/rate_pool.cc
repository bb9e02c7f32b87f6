// =================================================================================================================
// ws_engine_rate_pool_*: the stream pool (stream_pool.cc) with a sample rate per slot.  One round carries one packet for any
// set of slots at any mix of rates through ONE launch chain per piece:
//   host: per slot A's emission, the frames owed, B's emission (the emission rule of engine_internal.h, the rate stream's too),
//         est_cap checked before any launch; the slots checked by the plain pool's helpers (pool_check_*)
//   A     one ws_resample_stream_rows_fwd over all slots of the piece: caller rate -> the container's.  A's history is caller
//         samples, which the host has: it stays on the HOST; the staging block [A][history | new] is uploaded once with the
//         table.  A's outputs land behind each slot's pending samples, which live in the state allocation
//   groups  cut as the pool cuts them; a group's rectangle is gathered from the pending samples and its estimates are
//         scattered behind each slot's B history by ws_rows_copy_fwd (pool_run_group on device buffers)
//   compaction  one ws_rows_copy_fwd moves every slot's unconsumed pending samples to the front of its other buffer
//   B     one ws_resample_stream_rows_fwd: container rate -> caller rate; histories on the device, two buffers a slot in turn;
//         outputs to one compact block, one device-to-host copy of it
// and ONE hipStreamSynchronize per push.  A slot at the container's rate runs the identity table U = D = K = 1 through both
// resamplers: no delay, no filter, the plain pool's samples.  Everything -- the pool's state, both pending buffers, B's buffers,
// the output block and every tap table -- is ONE device allocation made at open, sized from max_push and the worst listed
// geometry; it never grows.
// =================================================================================================================
#include <memory>

#include "engine_internal.h"

using namespace wsrt;

namespace {

struct Rate {                // one accepted sample rate: caller -> container (a) and back (b); tables at state floats
  int rate = 0;
  Geom a, b;
  long long a_taps = 0, b_taps = 0;
};

struct RateSlot {
  int ri = -1;                        // its rate, an index into ws_rate_pool::rates
  std::vector<float> a_hist;          // A's history: caller samples, on the host
  long long a_n = 0, a_groups = 0;
  int p_cur = 0, have = 0;            // the pending buffer in use and the samples in it (from frame k's first one on)
  long long n_model = 0;              // samples at the container's rate that A has delivered
  int b_cur = 0, b_h = 0;             // B's buffer in use and its history
  long long b_n = 0, b_groups = 0;
  long long n = 0, returned = 0;      // samples pushed and returned, at the slot's rate
};

struct PieceRow {                     // one slot in one piece
  int slot = 0, entry = 0;
  const float* chunk = nullptr;
  int take = 0;
  int m = 0, consumed = 0;            // samples the groups wrote behind B's history; pending samples the groups consumed
};

struct OutRec {                       // one device-to-host copy of B's compact block: (entry, offset, count) per row
  std::vector<float> host;
  std::vector<int> entry, off, count;
};

}  // namespace

struct ws_rate_pool {
  ws_engine* e = nullptr;
  ws_pool* inner = nullptr;
  int max_push = 0;
  std::vector<Rate> rates;            // rates[0]: the container's own (identity)
  std::vector<RateSlot> slots;
  float* state = nullptr;             // the inner pool's allocation as one arena of floats
  long long state_floats = 0;
  long long pend0 = 0, b0 = 0, bout0 = 0;
  int pend_cap = 0, b_ld = 0, b_cap = 0, a_ld = 0;
  // host memory of the call in hand, alive until its synchronisation
  std::vector<std::vector<float>> stage;
  std::vector<std::vector<ws_resample_row>> tabs;
  std::vector<std::vector<ws_rows_copy_row>> ctabs;
  std::vector<OutRec> outs;

  long long pend(int slot, int which) const { return pend0 + ((long long)slot * 2 + which) * pend_cap; }
  long long bbuf(int slot, int which) const { return b0 + ((long long)slot * 2 + which) * b_ld; }
  void clear_call() { stage.clear(), tabs.clear(), ctabs.clear(), outs.clear(), inner->groups.clear(); }
};

namespace {

constexpr const char* kWho = "ws_engine_rate_pool";

// the table goes up behind everything the launch reads; `buf` is the staging block (A) or the state (B)
int rows_launch(ws_rate_pool* rp, const float* buf, long long n_buf, bool with_hist) {
  ws_engine* e = rp->e;
  const std::vector<ws_resample_row>& tab = rp->tabs.back();
  const int A = static_cast<int>(tab.size());
  ws_resample_row* d_tab = reinterpret_cast<ws_resample_row*>(e->work.alloc(size_t(A) * sizeof(ws_resample_row) / 4));
  WS_PTR(d_tab);
  int rc;
  if ((rc = copy_async(e, kWho, "table upload", d_tab, tab.data(), size_t(A) * sizeof(ws_resample_row), hipMemcpyHostToDevice)) != WS_OK) return rc;
  WS_RUN(e, ws_resample_stream_rows_fwd(tab.data(), d_tab, A, buf, n_buf, rp->state, rp->state_floats, rp->state, rp->state_floats,
                                        with_hist ? rp->state : nullptr, with_hist ? rp->state_floats : 0, e->stream));
  return WS_OK;
}

// Resampler A over the rows of a piece (final: the flush of one slot, nothing new): one upload, one launch
int a_step(ws_rate_pool* rp, std::vector<PieceRow>& rows, bool final) {
  ws_engine* e = rp->e;
  const int A = static_cast<int>(rows.size());
  rp->stage.emplace_back(size_t(A) * rp->a_ld, 0.f);
  rp->tabs.emplace_back();
  std::vector<float>& stage = rp->stage.back();
  for (int r = 0; r < A; ++r) {
    PieceRow& row = rows[r];
    RateSlot& sl = rp->slots[row.slot];
    const Rate& rt = rp->rates[sl.ri];
    const int h = static_cast<int>(sl.a_hist.size()), n_new = final ? 0 : row.take;
    const Step st = plan_step(rt.a, sl.a_n, sl.a_groups, h, n_new, final);
    sl.a_n += n_new;
    if (st.n_valid == 0 || (n_new == 0 && !final)) continue;
    float* x = stage.data() + size_t(r) * rp->a_ld;
    if (h) memcpy(x, sl.a_hist.data(), size_t(h) * 4);
    if (n_new) memcpy(x + h, row.chunk, size_t(n_new) * 4);
    if (st.n_out > 0) {
      ws_resample_row d{};
      d.in_off = (long long)r * rp->a_ld, d.taps_off = rt.a_taps, d.out_off = rp->pend(row.slot, sl.p_cur) + sl.have;
      d.U = rt.a.U, d.D = rt.a.D, d.K = rt.a.K, d.lead = st.lead, d.n_valid = st.n_valid, d.final = final ? 1 : 0, d.n_out = st.n_out;
      rp->tabs.back().push_back(d);
      sl.have += st.n_out, sl.n_model += st.n_out;
    }
    if (!final) {
      sl.a_hist.assign(x + st.hist_from, x + st.hist_from + st.hist_len);
      sl.a_groups = st.g_new;
    }
  }
  if (rp->tabs.back().empty()) return WS_OK;
  float* d_stage = e->work.alloc(stage.size());
  WS_PTR(d_stage);
  int rc;
  if ((rc = copy_async(e, kWho, "host-to-device copy", d_stage, stage.data(), stage.size() * 4, hipMemcpyHostToDevice)) != WS_OK) return rc;
  return rows_launch(rp, d_stage, static_cast<long long>(stage.size()), false);
}

// The frames the rows owe (flush: by the flush rule, on the zero-extended pending samples), cut into groups as the pool cuts
// them; each group gathers from the pending buffers and scatters behind B's history
int run_frames(ws_rate_pool* rp, std::vector<PieceRow>& rows, bool flush) {
  ws_pool* p = rp->inner;
  const int L = rp->e->tas.L, s = L / 2;
  std::vector<long long> owed(rows.size());
  for (size_t r = 0; r < rows.size(); ++r) {
    const RateSlot& sl = rp->slots[rows[r].slot];
    PoolSlot& isl = p->slots[rows[r].slot];
    const long long nm = sl.n_model;
    owed[r] = plain_frames(nm, L, flush) - isl.k;
    isl.n = nm;
  }
  int rc;
  while (true) {
    PoolGroup g;
    for (size_t r = 0; r < rows.size(); ++r) {
      if (owed[r] <= 0) continue;
      PieceRow& row = rows[r];
      const RateSlot& sl = rp->slots[row.slot];
      const int tc = static_cast<int>(std::min<long long>(owed[r], p->G));
      g.slot.push_back(row.slot), g.tc.push_back(tc), g.col.push_back(0);
      g.src_off.push_back(rp->pend(row.slot, sl.p_cur) + std::min(row.consumed, sl.have));
      g.src_have.push_back(std::max(0, sl.have - row.consumed));
      g.dst_off.push_back(rp->bbuf(row.slot, sl.b_cur) + sl.b_h + row.m);
      g.Tc = std::max(g.Tc, tc);
      owed[r] -= tc, row.consumed += tc * s, row.m += tc * s;
    }
    if (g.slot.empty()) return WS_OK;
    p->groups.push_back(std::move(g));
    if ((rc = pool_run_group(p, p->groups.back())) != WS_OK) return rc;
  }
}

// what the groups left of every row's pending samples moves to the front of the row's other buffer: one launch
int compact(ws_rate_pool* rp, std::vector<PieceRow>& rows) {
  ws_engine* e = rp->e;
  rp->ctabs.emplace_back();
  std::vector<ws_rows_copy_row>& tab = rp->ctabs.back();
  for (PieceRow& row : rows) {
    if (row.consumed == 0) continue;
    RateSlot& sl = rp->slots[row.slot];
    const int left = std::max(0, sl.have - row.consumed);
    if (left > 0) tab.push_back(ws_rows_copy_row{rp->pend(row.slot, sl.p_cur) + row.consumed, rp->pend(row.slot, 1 - sl.p_cur), left, 0});
    sl.p_cur ^= 1, sl.have = left, row.consumed = 0;
  }
  if (tab.empty()) return WS_OK;
  const int A = static_cast<int>(tab.size());
  ws_rows_copy_row* d_tab = reinterpret_cast<ws_rows_copy_row*>(e->work.alloc(size_t(A) * sizeof(ws_rows_copy_row) / 4));
  WS_PTR(d_tab);
  int rc;
  if ((rc = copy_async(e, kWho, "table upload", d_tab, tab.data(), size_t(A) * sizeof(ws_rows_copy_row), hipMemcpyHostToDevice)) != WS_OK) return rc;
  WS_RUN(e, ws_rows_copy_fwd(tab.data(), d_tab, A, rp->state, rp->state_floats, rp->state, rp->state_floats, e->stream));
  return WS_OK;
}

// Resampler B over the rows of a piece: row.m samples arrived behind its history; outputs to the compact block, one copy down
int b_step(ws_rate_pool* rp, std::vector<PieceRow>& rows, bool final) {
  ws_engine* e = rp->e;
  rp->tabs.emplace_back();
  rp->outs.emplace_back();
  OutRec& rec = rp->outs.back();
  int off = 0;
  for (PieceRow& row : rows) {
    RateSlot& sl = rp->slots[row.slot];
    const Rate& rt = rp->rates[sl.ri];
    const int n_new = final ? 0 : row.m;
    const Step st = plan_step(rt.b, sl.b_n, sl.b_groups, sl.b_h, n_new, final);
    sl.b_n += n_new;
    row.m = 0;
    if (st.n_valid == 0 || (n_new == 0 && !final) || (st.n_out == 0 && st.hist_len == 0)) continue;
    ws_resample_row d{};
    d.in_off = rp->bbuf(row.slot, sl.b_cur), d.taps_off = rt.b_taps, d.out_off = rp->bout0 + off, d.hist_off = rp->bbuf(row.slot, 1 - sl.b_cur);
    d.U = rt.b.U, d.D = rt.b.D, d.K = rt.b.K, d.lead = st.lead, d.n_valid = st.n_valid, d.final = final ? 1 : 0, d.n_out = st.n_out;
    d.hist_from = st.hist_from, d.hist_len = st.hist_len;
    rp->tabs.back().push_back(d);
    if (st.n_out > 0) rec.entry.push_back(row.entry), rec.off.push_back(off), rec.count.push_back(st.n_out);
    off += st.n_out;
    if (!final) sl.b_cur ^= 1, sl.b_h = st.hist_len, sl.b_groups = st.g_new;
  }
  if (rp->tabs.back().empty()) return WS_OK;
  int rc;
  if ((rc = rows_launch(rp, rp->state, rp->state_floats, true)) != WS_OK) return rc;
  rec.host.assign(size_t(off), 0.f);
  return copy_async(e, kWho, "device-to-host copy", rec.host.data(), rp->state + rp->bout0, size_t(off) * 4, hipMemcpyDeviceToHost);
}

// after the synchronisation: B's blocks to the callers' buffers, in order, cropped to what each entry emits
void deliver(ws_rate_pool* rp, float* const* est, const std::vector<long long>& emit, std::vector<long long>& col) {
  for (const OutRec& rec : rp->outs)
    for (size_t i = 0; i < rec.entry.size(); ++i) {
      const int en = rec.entry[i];
      const long long take = std::min<long long>(rec.count[i], emit[en] - col[en]);
      if (take > 0 && !rp->e->dry) memcpy(est[en] + col[en], rec.host.data() + rec.off[i], size_t(take) * 4);
      col[en] += std::max<long long>(take, 0);
    }
}

int check_rate_pool(const ws_rate_pool* rp, const char* who) {
  if (!rp || !rp->e || !rp->inner) {
    set_err("%s: null pool", who);
    return WS_ERR_INVALID;
  }
  return pool_check(rp->inner, who);
}

int push_cap_of(const ws_rate_pool* rp, const Rate& rt, int n) { return rate_push_cap(rt.a, rt.b, rp->e->tas.L, n); }

std::string rates_text(const ws_rate_pool* rp) {
  std::string s;
  for (const Rate& r : rp->rates) s += (s.empty() ? "" : ", ") + std::to_string(r.rate);
  return s;
}

}  // namespace

WS_ENGINE_API int ws_engine_rate_pool_open(ws_engine* e, int slots, int max_chunk_frames, unsigned flags, const int* rates, int n_rates,
                                           int max_push, ws_rate_pool** out) {
  const char* who = "ws_engine_rate_pool_open";
  int rc = check_engine(e, who);
  if (rc != WS_OK) return rc;
  if (!out) {
    set_err("%s: out is NULL", who);
    return WS_ERR_INVALID;
  }
  *out = nullptr;
  if (!tas_streamable(e)) return refuse_not_streamable(e, who);
  if (flags & ~unsigned(WS_STREAM_BLOCK_KERNEL)) {
    set_err("%s: unknown flag bits 0x%x (known: WS_STREAM_BLOCK_KERNEL = 1)", who, flags & ~unsigned(WS_STREAM_BLOCK_KERNEL));
    return WS_ERR_INVALID;
  }
  if (slots < 1 || slots > 65535 || max_push < 1 || max_push > (1 << 24) || n_rates < 0 || (n_rates > 0 && !rates)) {
    set_err("%s: bad arguments (slots=%d in [1, 65535], max_push=%d in [1, 2^24], n_rates=%d >= 0%s)", who, slots, max_push, n_rates,
            n_rates > 0 && !rates ? ", rates is NULL" : "");
    return WS_ERR_INVALID;
  }
  std::unique_ptr<ws_rate_pool> rp(new ws_rate_pool());
  rp->e = e, rp->max_push = max_push;
  Rate own;
  own.rate = e->sr;
  rp->rates.push_back(own);
  for (int i = 0; i < n_rates; ++i) {
    bool seen = false;
    for (const Rate& r : rp->rates) seen = seen || r.rate == rates[i];
    if (seen) continue;
    Rate r;
    r.rate = rates[i];
    if (ws_resample_geom(r.rate, e->sr, &r.a.U, &r.a.D, &r.a.w, &r.a.K) != WS_OK ||
        ws_resample_geom(e->sr, r.rate, &r.b.U, &r.b.D, &r.b.w, &r.b.K) != WS_OK) {
      set_err("%s: rates[%d]: %s", who, i, ws_last_error());
      return WS_ERR_INVALID;
    }
    rp->rates.push_back(r);
  }
  // ---- sizes, from max_push and the worst listed geometry ----
  const int L = e->tas.L, s = L / 2;
  long long a_ld = 0, a_cap = 0, taps = 0;
  for (Rate& r : rp->rates) {
    a_ld = std::max<long long>(a_ld, r.a.K - 1 + max_push);
    a_cap = std::max<long long>(a_cap, ((long long)(r.a.K - 1 + max_push) / r.a.D + 1) * r.a.U);
    r.a_taps = taps, taps += (long long)r.a.U * r.a.K;
    r.b_taps = taps, taps += (long long)r.b.U * r.b.K;
  }
  const long long pend_cap = (kEncLmax + s + a_cap + 3) / 4 * 4;
  const long long m_cap = (pend_cap / s + 1) * s + L;
  long long b_ld = 0, b_cap = 0;
  for (const Rate& r : rp->rates) {
    b_ld = std::max<long long>(b_ld, r.b.K - 1 + m_cap);
    b_cap = std::max<long long>(b_cap, ((long long)(r.b.K - 1 + m_cap) / r.b.D + 1) * r.b.U);
  }
  b_ld = (b_ld + 3) / 4 * 4, b_cap = (b_cap + 3) / 4 * 4, taps = (taps + 3) / 4 * 4;
  const long long extra = taps + (long long)slots * (2 * pend_cap + 2 * b_ld + b_cap);
  if (extra >= (1LL << 31)) {
    set_err("%s: slots=%d with max_push=%d reaches 2^31 elements of resampler state", who, slots, max_push);
    return WS_ERR_INVALID;
  }
  float* x = nullptr;
  if ((rc = pool_open_impl(e, who, slots, max_chunk_frames, flags, static_cast<size_t>(extra), &rp->inner, &x)) != WS_OK) return rc;
  rp->slots.resize(slots);
  rp->state = reinterpret_cast<float*>(rp->inner->state), rp->state_floats = static_cast<long long>(rp->inner->state_bytes / 4);
  rp->a_ld = static_cast<int>(a_ld), rp->pend_cap = static_cast<int>(pend_cap), rp->b_ld = static_cast<int>(b_ld), rp->b_cap = static_cast<int>(b_cap);
  const long long x0 = x - rp->state;
  rp->pend0 = x0 + taps, rp->b0 = rp->pend0 + (long long)slots * 2 * pend_cap, rp->bout0 = rp->b0 + (long long)slots * 2 * b_ld;
  // ---- every tap table, made in the one place and uploaded once ----
  std::vector<float> host(static_cast<size_t>(taps), 0.f);
  for (Rate& r : rp->rates) {
    if (r.rate == e->sr) {
      host[r.a_taps] = host[r.b_taps] = 1.f;       // the identity table
    } else if (ws_resample_taps(r.rate, e->sr, host.data() + r.a_taps) != WS_OK || ws_resample_taps(e->sr, r.rate, host.data() + r.b_taps) != WS_OK) {
      set_err("%s: %s", who, ws_last_error());
      pool_free(rp->inner);
      return WS_ERR_INVALID;
    }
    r.a_taps += x0, r.b_taps += x0;
  }
  {
    ForwardTurn turn(e);
    rc = turn.rc != WS_OK ? turn.rc : to_device(e, x, host.data(), host.size() * 4);
  }
  if (rc != WS_OK) {
    pool_free(rp->inner);
    return rc;
  }
  *out = rp.release();
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_pool_attach(ws_rate_pool* rp, const void* enroll, int enroll_kind, int enroll_len, int enroll_rate,
                                             int sample_rate, int* slot) {
  const char* who = "ws_engine_rate_pool_attach";
  int rc = check_rate_pool(rp, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = rp->e;
  int ri = -1;
  for (size_t i = 0; i < rp->rates.size(); ++i)
    if (rp->rates[i].rate == sample_rate) ri = static_cast<int>(i);
  if (ri < 0) {
    set_err("%s: sample_rate=%d is not one of the rates this pool was opened with (accepted: %s)", who, sample_rate, rates_text(rp).c_str());
    return WS_ERR_INVALID;
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
  std::vector<float> enr_m;
  int len_m = enroll_len;
  long long launches = 0;
  if (enr_rs) {
    Geom ge;
    if (ws_resample_geom(enroll_rate, e->sr, &ge.U, &ge.D, &ge.w, &ge.K) != WS_OK) {
      set_err("%s: %s", who, ws_last_error());
      return WS_ERR_INVALID;
    }
    if (enroll_len < 1) {
      set_err("%s: enroll_len=%d, a waveform enrollment has at least one sample", who, enroll_len);
      return WS_ERR_INVALID;
    }
    if ((rc = tasnet_check_enroll(e, enroll_kind, static_cast<int>(rs_len(ge, enroll_len)))) != WS_OK) return rc;
    ForwardTurn turn(e);
    if (turn.rc != WS_OK) return turn.rc;
    e->n_launches = 0;
    if ((rc = resample_host_rows(e, who, static_cast<const float*>(enroll), 1, enroll_len, enroll_rate, e->sr, &enr_m, &len_m)) != WS_OK) return rc;
    launches = e->n_launches;
    enroll = enr_m.data();
  }
  int id = -1;
  if ((rc = pool_attach_impl(rp->inner, who, enroll, enroll_kind, len_m, &id)) != WS_OK) return rc;
  e->n_launches += launches;
  rp->slots[id] = RateSlot();
  rp->slots[id].ri = ri;
  *slot = id;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_pool_push_cap(const ws_rate_pool* rp, int slot, int n) {
  if (!rp || !rp->e || n < 0 || slot < 0 || slot >= static_cast<int>(rp->slots.size()) || rp->slots[slot].ri < 0) return -1;
  return push_cap_of(rp, rp->rates[rp->slots[slot].ri], n);
}

WS_ENGINE_API int ws_engine_rate_pool_push(ws_rate_pool* rp, int n_active, const int* slots, const float* const* chunks, const int* n,
                                           float* const* est, const int* est_cap, int* n_out) {
  const char* who = "ws_engine_rate_pool_push";
  int rc = check_rate_pool(rp, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = rp->e;
  ws_pool* p = rp->inner;
  const int L = e->tas.L;
  if ((rc = pool_check_push_args(who, n_active, slots, chunks, n, est, est_cap, n_out)) != WS_OK) return rc;
  std::vector<char> seen(p->rows, 0);
  std::vector<long long> emit(n_active), col(n_active, 0);
  int pieces = 0;
  for (int i = 0; i < n_active; ++i) {
    const int id = slots[i];
    if ((rc = pool_check_entry(p, who, seen, i, id, n[i], chunks[i])) != WS_OK) return rc;
    const RateSlot& sl = rp->slots[id];
    const Rate& rt = rp->rates[sl.ri];
    emit[i] = rs_emitted(rt.b, plain_emitted(rs_emitted(rt.a, sl.n + n[i]), L)) - sl.returned;
    if (emit[i] > est_cap[i] || (emit[i] > 0 && !est[i])) {
      set_err("%s: entry %d (slot %d) emits %lld samples, est_cap is %d (ws_engine_rate_pool_push_cap(pool, %d, %d) = %d always suffices)", who, i,
              id, emit[i], est_cap[i], id, n[i], push_cap_of(rp, rt, n[i]));
      return WS_ERR_INVALID;
    }
    pieces = std::max(pieces, (n[i] + rp->max_push - 1) / rp->max_push);
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  for (int i = 0; i < n_active; ++i) p->slots[slots[i]].failed = true;      // until the push is complete
  rp->clear_call();
  ArenaScope scope(e->work);
  for (int j = 0; j < pieces && rc == WS_OK; ++j) {
    std::vector<PieceRow> rows;
    for (int i = 0; i < n_active; ++i) {
      const long long lo = (long long)j * rp->max_push;
      if (lo >= n[i]) continue;
      PieceRow row;
      row.slot = slots[i], row.entry = i, row.chunk = chunks[i] + lo, row.take = static_cast<int>(std::min<long long>(n[i] - lo, rp->max_push));
      rows.push_back(row);
    }
    if ((rc = a_step(rp, rows, false)) != WS_OK) break;
    if ((rc = run_frames(rp, rows, false)) != WS_OK) break;
    if ((rc = compact(rp, rows)) != WS_OK) break;
    rc = b_step(rp, rows, false);
  }
  if (rc == WS_OK) rc = sync_stream(e, kWho);                 // the one host synchronisation of a push
  if (rc != WS_OK) return rc;
  deliver(rp, est, emit, col);
  rp->clear_call();
  for (int i = 0; i < n_active; ++i)
    if (col[i] != emit[i]) {
      set_err("%s: internal error: entry %d: %lld samples were produced where the rule says %lld", who, i, col[i], emit[i]);
      return WS_ERR_LAUNCH;
    }
  for (int i = 0; i < n_active; ++i) {
    RateSlot& sl = rp->slots[slots[i]];
    sl.n += n[i], sl.returned += emit[i];
    p->slots[slots[i]].failed = false;
    n_out[i] = static_cast<int>(emit[i]);
  }
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_pool_flush(ws_rate_pool* rp, int slot, float* est, int est_cap, int* n_out) {
  const char* who = "ws_engine_rate_pool_flush";
  int rc = check_rate_pool(rp, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = rp->e;
  ws_pool* p = rp->inner;
  const int L = e->tas.L, s = L / 2;
  if ((rc = pool_check_slot(p, who, slot, true)) != WS_OK) return rc;
  PoolSlot& isl = p->slots[slot];
  RateSlot& sl = rp->slots[slot];
  const Rate& rt = rp->rates[sl.ri];
  const long long n_model = rs_len(rt.a, sl.n);
  if (n_model < L) {
    set_err("%s: slot %d: %lld samples were pushed, %lld at the container's rate, fewer than the encoder window L = %d", who, slot, sl.n, n_model,
            L);
    return WS_ERR_INVALID;
  }
  const long long total = std::min(sl.n, rs_len(rt.b, plain_total(n_model, L)));
  std::vector<long long> emit(1, std::max<long long>(0, total - sl.returned)), col(1, 0);
  if (!n_out || emit[0] > est_cap || (emit[0] > 0 && !est)) {
    set_err("%s: the flush emits %lld samples, est_cap is %d%s (ws_engine_rate_pool_push_cap(pool, %d, 0) = %d always suffices)", who, emit[0],
            est_cap, n_out ? "" : ", n_out is NULL", slot, push_cap_of(rp, rt, 0));
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  isl.failed = true;
  rp->clear_call();
  ArenaScope scope(e->work);
  std::vector<PieceRow> rows(1);
  rows[0].slot = slot;
  do {
    if ((rc = a_step(rp, rows, true)) != WS_OK) break;                 // A's flush
    if ((rc = run_frames(rp, rows, false)) != WS_OK) break;            // the frames that are complete now
    if ((rc = compact(rp, rows)) != WS_OK) break;
    if ((rc = b_step(rp, rows, false)) != WS_OK) break;
    if ((rc = run_frames(rp, rows, true)) != WS_OK) break;             // the inner flush: the rest on the zero extension ...
    {                                                                  // ... and the overlap-add carry behind it
      rp->ctabs.emplace_back(1, ws_rows_copy_row{static_cast<long long>(p->carry + size_t(slot) * (L - s) - rp->state),
                                                 rp->bbuf(slot, sl.b_cur) + sl.b_h + rows[0].m, L - s, 0});
      ws_rows_copy_row* d_tab = reinterpret_cast<ws_rows_copy_row*>(e->work.alloc(sizeof(ws_rows_copy_row) / 4));
      if (!d_tab) {
        rc = WS_ERR_LAUNCH;
        break;
      }
      if ((rc = copy_async(e, kWho, "table upload", d_tab, rp->ctabs.back().data(), sizeof(ws_rows_copy_row), hipMemcpyHostToDevice)) != WS_OK) break;
      const int crc = ws_rows_copy_fwd(rp->ctabs.back().data(), d_tab, 1, rp->state, rp->state_floats, rp->state, rp->state_floats, e->stream);
      if (!passes(e, crc, "ws_rows_copy_fwd")) {
        rc = crc ? crc : WS_ERR_LAUNCH;
        break;
      }
      rows[0].m += L - s;
    }
    if ((rc = b_step(rp, rows, false)) != WS_OK) break;
    rc = b_step(rp, rows, true);                                       // B's flush, cropped below
  } while (false);
  if (rc == WS_OK) rc = sync_stream(e, kWho);
  if (rc != WS_OK) return rc;
  float* const ests[1] = {est};
  deliver(rp, ests, emit, col);
  rp->clear_call();
  if (col[0] != emit[0]) {
    set_err("%s: internal error: %lld samples were produced where the rule says %lld", who, col[0], emit[0]);
    return WS_ERR_LAUNCH;
  }
  sl.returned += emit[0];
  sl.have = 0;
  isl.failed = false;
  isl.state = PoolSlot::kDone;
  *n_out = static_cast<int>(emit[0]);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_rate_pool_detach(ws_rate_pool* rp, int slot) {
  const int rc = pool_detach_impl(rp && rp->e ? rp->inner : nullptr, "ws_engine_rate_pool_detach", slot);
  if (rc == WS_OK) rp->slots[slot] = RateSlot();
  return rc;
}

WS_ENGINE_API void ws_engine_rate_pool_close(ws_rate_pool* rp) {
  if (!rp) return;
  ws_engine_pool_close(rp->inner);
  delete rp;
}
