// =================================================================================================================
// ws_engine_pool_*: MANY independent streams of a causal cLN Conv-TasNet / SpEx+ container through ONE launch chain per
// round.  A solo stream (stream.cc) has rows that all sit at the same sample position; the calls of a server start at
// different times and deliver packets of different sizes.  Every frame of every layer of a causal cLN model depends on
// earlier frames of its own row only, and only two kernels look across time; their pool forms (wesep_hip.h:
// ws_tcn_mid_stream_rows_fwd, ws_ola_stream_rows_fwd) take a per-row (state slot, first frame, frame count), so any set of
// streams shares one [A][Tc] rectangle: row i carries tc_i <= Tc new frames of its stream, the rest of the row is computed
// on zeros and consumed by nothing.
// State: the StreamCore of stream.cc with a row per slot -- the rings, the overlap-add carry, the embedding after
// SpeakerTransform and the stacks' row biases; one carry reset image.  The samples that have not completed a frame live on
// the HOST, per slot: a group's staging block is built there and uploaded once, so there is no pending-sample copy on the
// device.  Per group: the three-table upload and stream_chain (stream.cc) in its rows form -- 3 R X + 9 entry-point calls
// (WS_POOL_GROUP_LAUNCHES), whatever A is; R X + 9 with WS_STREAM_BLOCK_KERNEL (WS_POOL_BLOCK_GROUP_LAUNCHES); a slot's samples
// are then the same bits whatever else shares its rectangle.
// A rate pool (rate_pool.cc) opens, attaches and runs its groups through the same functions (pool_open_impl, pool_attach_impl,
// pool_run_group) and checks its slots with the same helpers (pool_check_*): its pending samples and its estimates'
// destination live in one more part of the state allocation, so a group gathers its rectangle and scatters its estimates with
// ws_rows_copy_fwd in place of the upload and the download.
// =================================================================================================================
#include "engine_internal.h"

using namespace wsrt;

namespace {

constexpr const char* kWho = "ws_engine_pool";

// Cuts what the named slots still owe into groups and runs them.  owed[i] frames of slots[i]; a row joins a group with
// min(owed, G) frames, a row that owes nothing stays out.  col[i]: the row's next sample in its caller's buffer.
int run_owed(ws_pool* p, const std::vector<int>& slots, std::vector<long long> owed) {
  const int s = p->e->tas.L / 2;
  std::vector<int> col(slots.size(), 0);
  int rc;
  while (true) {
    PoolGroup g;
    for (size_t i = 0; i < slots.size(); ++i) {
      if (owed[i] <= 0) continue;
      const int tc = static_cast<int>(std::min<long long>(owed[i], p->G));
      g.slot.push_back(slots[i]), g.tc.push_back(tc), g.col.push_back(col[i]);
      g.Tc = std::max(g.Tc, tc);
      owed[i] -= tc, col[i] += tc * s;
    }
    if (g.slot.empty()) return WS_OK;
    p->groups.push_back(std::move(g));
    if ((rc = pool_run_group(p, p->groups.back())) != WS_OK) return rc;
  }
}

}  // namespace

// One group: row i of the rectangle is slot g.slot[i] with g.tc[i] >= 1 frames from its frame k on; Tc = max tc.  The
// staging block is zero-filled, so a flush's frames read zeros behind the slot's last sample, as the whole-utterance
// encoder does.  The slots' positions move here; their pending samples are dropped by the caller.
int wsrt::pool_run_group(ws_pool* p, PoolGroup& g) {
  ws_engine* e = p->e;
  const int s = e->tas.L / 2, A = static_cast<int>(g.slot.size()), Tc = g.Tc;
  const int pitch = (Tc - 1) * s + kEncLmax;
  void* q = e->stream;
  const bool dio = p->device_io;
  if (!dio) g.stage.assign(size_t(A) * pitch, 0.f);
  g.t0.resize(A);
  for (int i = 0; i < A; ++i) {
    const PoolSlot& sl = p->slots[g.slot[i]];
    const size_t want = size_t(g.tc[i] - 1) * s + kEncLmax;
    if (!dio) memcpy(g.stage.data() + size_t(i) * pitch, sl.pend.data(), std::min(want, sl.pend.size()) * 4);
    g.t0[i] = sl.k;
  }
  if (!dio) g.est.assign(size_t(A) * Tc * s, 0.f);
  Arena& a = e->work;
  ArenaScope scope(a);
  float* x0 = a.alloc(size_t(A) * pitch);
  // the three tables in one block: t0 (8-byte entries) first, then slot and tc
  char* tab = reinterpret_cast<char*>(a.alloc(size_t(A) * 4));
  ws_rows_copy_row* d_rows = dio ? reinterpret_cast<ws_rows_copy_row*>(a.alloc(size_t(A) * 2 * sizeof(ws_rows_copy_row) / 4)) : nullptr;
  WS_PTR(x0 && tab && (!dio || d_rows));
  long long* d_t0 = reinterpret_cast<long long*>(tab);
  int* d_slot = reinterpret_cast<int*>(tab + size_t(A) * 8);
  int* d_tc = d_slot + A;
  int rc;
  float* const state = reinterpret_cast<float*>(p->state);
  const long long state_floats = static_cast<long long>(p->state_bytes / 4);
  const auto up = [&](void* dst, const void* src, size_t bytes, const char* what) {
    return copy_async(e, kWho, what, dst, src, bytes, hipMemcpyHostToDevice);
  };
  if (dio) {
    // the rectangle is gathered from the slots' pending samples on the device, zeros behind them (the staging block's zero fill);
    // the estimates are scattered behind each slot's destination: two table-driven copies in place of the upload and download
    g.gather.resize(A), g.scatter.resize(A);
    for (int i = 0; i < A; ++i) {
      const int want = (g.tc[i] - 1) * s + kEncLmax, len = std::min(want, g.src_have[i]);
      g.gather[i] = ws_rows_copy_row{g.src_off[i], (long long)i * pitch, len, pitch - len};
      g.scatter[i] = ws_rows_copy_row{(long long)i * Tc * s, g.dst_off[i], g.tc[i] * s, 0};
    }
    if ((rc = up(d_rows, g.gather.data(), size_t(A) * sizeof(ws_rows_copy_row), "table upload")) != WS_OK) return rc;
    if ((rc = up(d_rows + A, g.scatter.data(), size_t(A) * sizeof(ws_rows_copy_row), "table upload")) != WS_OK) return rc;
    WS_RUN(e, ws_rows_copy_fwd(g.gather.data(), d_rows, A, state, state_floats, x0, (long long)A * pitch, q));
  } else if ((rc = up(x0, g.stage.data(), g.stage.size() * 4, "host-to-device copy")) != WS_OK) {
    return rc;
  }
  if ((rc = up(d_t0, g.t0.data(), size_t(A) * 8, "table upload")) != WS_OK) return rc;
  if ((rc = up(d_slot, g.slot.data(), size_t(A) * 4, "table upload")) != WS_OK) return rc;
  if ((rc = up(d_tc, g.tc.data(), size_t(A) * 4, "table upload")) != WS_OK) return rc;
  ChainRows rows;
  rows.rows = A, rows.Tc = Tc, rows.nslots = p->rows, rows.d_slot = d_slot, rows.d_tc = d_tc, rows.d_t0 = d_t0;
  float* est = nullptr;
  if ((rc = stream_chain(e, *p, p->block_kernel, x0, pitch, rows, p->carry, &est)) != WS_OK) return rc;
  if (dio) {
    WS_RUN(e, ws_rows_copy_fwd(g.scatter.data(), d_rows + A, A, est, (long long)A * Tc * s, state, state_floats, q));
  } else if ((rc = copy_async(e, kWho, "device-to-host copy", g.est.data(), est, g.est.size() * 4, hipMemcpyDeviceToHost)) != WS_OK) {
    return rc;
  }
  for (int i = 0; i < A; ++i) {
    PoolSlot& sl = p->slots[g.slot[i]];
    const size_t used = std::min(size_t(g.tc[i]) * s, sl.pend.size());
    sl.pend.erase(sl.pend.begin(), sl.pend.begin() + used);
    sl.k += g.tc[i];
  }
  return WS_OK;
}

int wsrt::pool_check(const ws_pool* p, const char* who) {
  if (!p || !p->e) {
    set_err("%s: null pool", who);
    return WS_ERR_INVALID;
  }
  for (int i = 0; i < p->rows; ++i)
    if (p->slots[i].failed) {
      set_err("%s: an earlier call on this pool failed half way with slot %d in it; detach the slots of that call (or close the pool)",
              who, i);
      return WS_ERR_INVALID;
    }
  return WS_OK;
}

int wsrt::pool_check_push_args(const char* who, int n_active, const void* slots, const void* chunks, const void* n, const void* est,
                               const void* est_cap, const void* n_out) {
  if (n_active >= 1 && slots && chunks && n && est && est_cap && n_out) return WS_OK;
  set_err("%s: bad arguments (n_active=%d >= 1%s)", who, n_active, slots && chunks && n && est && est_cap && n_out ? "" : ", a NULL array");
  return WS_ERR_INVALID;
}

int wsrt::pool_check_entry(const ws_pool* p, const char* who, std::vector<char>& seen, int i, int id, int n, const float* chunk) {
  if (id < 0 || id >= p->rows || p->slots[id].state == PoolSlot::kFree)
    set_err("%s: slot %d (entry %d) is not attached (the pool has %d slots)", who, id, i, p->rows);
  else if (p->slots[id].state == PoolSlot::kDone)
    set_err("%s: slot %d (entry %d) was flushed (detach it, then attach the next stream)", who, id, i);
  else if (seen[id])
    set_err("%s: slot %d is named twice (entry %d): one packet a slot in a push", who, id, i);
  else if (n < 1 || !chunk)
    set_err("%s: entry %d (slot %d): n=%d >= 1, chunk %s", who, i, id, n, chunk ? "given" : "NULL");
  else {
    seen[id] = 1;
    return WS_OK;
  }
  return WS_ERR_INVALID;
}

int wsrt::pool_check_slot(const ws_pool* p, const char* who, int slot, bool flush) {
  if (slot < 0 || slot >= p->rows || p->slots[slot].state == PoolSlot::kFree)
    set_err("%s: slot %d is not attached (the pool has %d slots)", who, slot, p->rows);
  else if (flush && p->slots[slot].state == PoolSlot::kDone)
    set_err("%s: slot %d was flushed already (detach it, then attach the next stream)", who, slot);
  else
    return WS_OK;
  return WS_ERR_INVALID;
}

int wsrt::pool_detach_impl(ws_pool* p, const char* who, int slot) {
  if (!p || !p->e) {
    set_err("%s: null pool", who);
    return WS_ERR_INVALID;
  }
  const int rc = pool_check_slot(p, who, slot, false);
  if (rc == WS_OK) p->slots[slot] = PoolSlot();       // free, and no longer the slot of a half-finished call
  return rc;
}

void wsrt::pool_free(ws_pool* p) {
  stream_core_free(p);
  delete p;
}

WS_ENGINE_API int ws_engine_pool_open(ws_engine* e, int slots, int max_chunk_frames, ws_pool** out) {
  return ws_engine_pool_open_ex(e, slots, max_chunk_frames, 0, out);
}

WS_ENGINE_API int ws_engine_pool_open_ex(ws_engine* e, int slots, int max_chunk_frames, unsigned flags, ws_pool** out) {
  return pool_open_impl(e, "ws_engine_pool_open", slots, max_chunk_frames, flags, 0, out, nullptr);
}

int wsrt::pool_open_impl(ws_engine* e, const char* who, int slots, int max_chunk_frames, unsigned flags, size_t extra_floats, ws_pool** out,
                         float** extra) {
  int rc = check_engine(e, who);
  if (rc != WS_OK) return rc;
  if (out) *out = nullptr;
  if (!tas_streamable(e)) return refuse_not_streamable(e, who);
  if (flags & ~unsigned(WS_STREAM_BLOCK_KERNEL)) {
    set_err("%s%s: unknown flag bits 0x%x (known: WS_STREAM_BLOCK_KERNEL = 1)", who, extra_floats ? "" : "_ex", flags & ~unsigned(WS_STREAM_BLOCK_KERNEL));
    return WS_ERR_INVALID;
  }
  if (!out) {
    set_err("%s: out is NULL", who);
    return WS_ERR_INVALID;
  }
  if (slots < 1) {
    set_err("%s: slots=%d, a pool has at least one", who, slots);
    return WS_ERR_INVALID;
  }
  if (max_chunk_frames < 1 || max_chunk_frames > 65536) {
    set_err("%s: max_chunk_frames=%d is outside [1, 65536]", who, max_chunk_frames);
    return WS_ERR_INVALID;
  }
  const int L = e->tas.L, s = L / 2;
  if ((rc = stream_core_check(e, who, "slots", slots, max_chunk_frames)) != WS_OK) return rc;
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  ws_pool* p = new ws_pool();
  p->slots.resize(slots);
  p->device_io = extra_floats != 0;
  // the pool's parts of the state block: carry, its reset image (one row), embedding
  std::vector<float*> at;
  if ((rc = stream_core_open(p, who, e, slots, max_chunk_frames, flags, {size_t(slots) * (L - s), size_t(L - s), size_t(slots) * e->E},
                             extra_floats, &at)) == WS_OK) {
    p->carry = at[0], p->carry0 = at[1], p->emb = at[2];
    if (extra_floats && extra) *extra = at[3];
    const std::vector<float> c0(size_t(L - s), e->host("decoder.decoder_1d_1.bias")[0]);   // the carry's reset image: the decoder bias
    rc = to_device(e, p->carry0, c0.data(), c0.size() * 4);
  }
  if (rc != WS_OK) {
    pool_free(p);
    return rc;
  }
  e->stream_state_bytes = static_cast<long long>(p->state_bytes);
  *out = p;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_pool_attach(ws_pool* p, const void* enroll, int enroll_kind, int enroll_len, int* slot) {
  return pool_attach_impl(p, "ws_engine_pool_attach", enroll, enroll_kind, enroll_len, slot);
}

int wsrt::pool_attach_impl(ws_pool* p, const char* who, const void* enroll, int enroll_kind, int enroll_len, int* slot) {
  int rc = pool_check(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  if (!enroll || !slot) {
    set_err("%s: bad arguments (enroll %s, slot %s)", who, enroll ? "given" : "NULL", slot ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  if ((rc = tasnet_check_enroll(e, enroll_kind, enroll_len)) != WS_OK) return rc;
  int id = 0;
  while (id < p->rows && p->slots[id].state != PoolSlot::kFree) ++id;
  if (id == p->rows) {
    set_err("%s: the pool is full: all %d slots are attached (detach one, or open a larger pool)", who, p->rows);
    return WS_ERR_INVALID;
  }
  const int nc = e->tas.L - e->tas.L / 2;
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  if ((rc = stream_enroll(p, kWho, enroll, enroll_kind, enroll_len, id, 1)) != WS_OK) return rc;     // the speaker stage for this slot
  // position 0: the carry is the bias image; the rings need no clearing (no term reads a frame before the start)
  if ((rc = copy_async(e, kWho, "device copy", p->carry + size_t(id) * nc, p->carry0, size_t(nc) * 4, hipMemcpyDeviceToDevice)) != WS_OK)
    return rc;
  if ((rc = sync_stream(e, kWho)) != WS_OK) return rc;
  PoolSlot& sl = p->slots[id];
  sl = PoolSlot();
  sl.state = PoolSlot::kAttached;
  *slot = id;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_pool_push(ws_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n,
                                      float* const* est, const int* est_cap, int* n_out) {
  const char* who = "ws_engine_pool_push";
  int rc = pool_check(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  const int L = e->tas.L, s = L / 2;
  if ((rc = pool_check_push_args(who, n_active, slots, chunks, n, est, est_cap, n_out)) != WS_OK) return rc;
  std::vector<char> seen(p->rows, 0);
  std::vector<long long> owed(n_active);
  for (int i = 0; i < n_active; ++i) {
    const int id = slots[i];
    if ((rc = pool_check_entry(p, who, seen, i, id, n[i], chunks[i])) != WS_OK) return rc;
    const PoolSlot& sl = p->slots[id];
    owed[i] = plain_frames(sl.n + n[i], L) - sl.k;
    const long long emit = owed[i] * s;
    if (emit > est_cap[i] || (emit > 0 && !est[i])) {
      set_err("ws_engine_pool_push: entry %d (slot %d) emits %lld samples, est_cap is %d (WS_STREAM_PUSH_CAP(n, L) = %d always suffices)",
              i, id, emit, est_cap[i], WS_STREAM_PUSH_CAP(n[i], L));
      return WS_ERR_INVALID;
    }
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  const std::vector<int> ids(slots, slots + n_active);
  for (int i = 0; i < n_active; ++i) {
    PoolSlot& sl = p->slots[ids[i]];
    sl.failed = true;                   // until the push is complete
    sl.pend.insert(sl.pend.end(), chunks[i], chunks[i] + n[i]);
    sl.n += n[i];
  }
  p->groups.clear();
  if ((rc = run_owed(p, ids, owed)) != WS_OK) return rc;
  if ((rc = sync_stream(e, kWho)) != WS_OK) return rc;       // the one host synchronisation of a push
  if (!e->dry)
    for (const PoolGroup& g : p->groups)
      for (size_t i = 0; i < g.slot.size(); ++i) {
        const int row = static_cast<int>(std::find(ids.begin(), ids.end(), g.slot[i]) - ids.begin());
        memcpy(est[row] + g.col[i], g.est.data() + i * size_t(g.Tc) * s, size_t(g.tc[i]) * s * 4);
      }
  p->groups.clear();
  for (int i = 0; i < n_active; ++i) {
    p->slots[ids[i]].failed = false;
    n_out[i] = static_cast<int>(owed[i] * s);
  }
  return WS_OK;
}

WS_ENGINE_API int ws_engine_pool_flush(ws_pool* p, int slot, float* est, int est_cap, int* n_out) {
  const char* who = "ws_engine_pool_flush";
  int rc = pool_check(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  const int L = e->tas.L, s = L / 2;
  if ((rc = pool_check_slot(p, who, slot, true)) != WS_OK) return rc;
  PoolSlot& sl = p->slots[slot];
  if (sl.n < L) {
    set_err("ws_engine_pool_flush: slot %d: %lld samples were pushed, fewer than the encoder window L = %d", slot, sl.n, L);
    return WS_ERR_INVALID;
  }
  const long long target = plain_frames(sl.n, L, true);
  const long long tail = (target - sl.k) * s, emit = tail + (L - s);
  if (!est || !n_out || emit > est_cap) {
    set_err("ws_engine_pool_flush: the flush emits %lld samples, est_cap is %d%s (WS_STREAM_FLUSH_CAP = %d always suffices)", emit,
            est_cap, est && n_out ? "" : ", est or n_out is NULL", WS_STREAM_FLUSH_CAP);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  sl.failed = true;
  p->groups.clear();
  // the remaining frames, A = 1: the zero-filled staging block is the zero extension of the whole-utterance encoder
  if ((rc = run_owed(p, std::vector<int>(1, slot), std::vector<long long>(1, target - sl.k))) != WS_OK) return rc;
  if ((rc = copy_async(e, kWho, "device-to-host copy", est + tail, p->carry + size_t(slot) * (L - s), size_t(L - s) * 4,
                       hipMemcpyDeviceToHost)) != WS_OK)
    return rc;
  if ((rc = sync_stream(e, kWho)) != WS_OK) return rc;
  if (!e->dry)
    for (const PoolGroup& g : p->groups) memcpy(est + g.col[0], g.est.data(), size_t(g.tc[0]) * s * 4);
  p->groups.clear();
  sl.pend.clear();
  sl.failed = false;
  sl.state = PoolSlot::kDone;
  *n_out = static_cast<int>(emit);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_pool_detach(ws_pool* p, int slot) { return pool_detach_impl(p, "ws_engine_pool_detach", slot); }

WS_ENGINE_API void ws_engine_pool_close(ws_pool* p) {
  if (!p) return;
  if (p->e && !p->e->dry) {
    (void)hipSetDevice(p->e->device);
    (void)hipStreamSynchronize(p->e->stream);
  }
  pool_free(p);
}
