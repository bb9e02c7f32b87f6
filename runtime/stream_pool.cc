// =================================================================================================================
// ws_engine_pool_*: MANY independent streams of a causal cLN Conv-TasNet / SpEx+ container through ONE launch chain per
// round.  A solo stream (stream.cc) has rows that all sit at the same sample position; the calls of a server start at
// different times and deliver packets of different sizes.  Every frame of every layer of a causal cLN model depends on
// earlier frames of its own row only, and only two kernels look across time; their pool forms (wesep_hip.h:
// ws_tcn_mid_stream_rows_fwd, ws_ola_stream_rows_fwd) take a per-row (state slot, first frame, frame count), so any set of
// streams shares one [A][Tc] rectangle: row i carries tc_i <= Tc new frames of its stream, the rest of the row is computed
// on zeros and consumed by nothing.
// State: ONE device allocation made at open -- per slot the rings, the overlap-add carry, the embedding after
// SpeakerTransform and the stacks' row biases; one carry reset image.  The samples that have not completed a frame live on
// the HOST, per slot: a group's staging block is built there and uploaded once, so there is no pending-sample copy on the
// device.  Per group: 3 framing GEMMs, row statistics, projection; per block GEMM, the fused middle, GEMM; mask GEMM, mask
// product, synthesis GEMM, overlap-add -- 3 R X + 9 entry-point calls (WS_POOL_GROUP_LAUNCHES), whatever A is.  A pool opened
// with WS_STREAM_BLOCK_KERNEL runs every block as ONE call, ws_tcn_block_stream_rows_fwd: R X + 9
// (WS_POOL_BLOCK_GROUP_LAUNCHES); a slot's samples are then the same bits whatever else shares its rectangle.
// A rate pool (rate_pool.cc) opens, attaches and runs its groups through the same functions (pool_open_impl, pool_attach_impl,
// pool_run_group): its pending samples and its estimates' destination live in one more part of the state allocation, so a
// group gathers its rectangle and scatters its estimates with ws_rows_copy_fwd in place of the upload and the download.
// =================================================================================================================
#include "engine_internal.h"

using namespace wsrt;

namespace {

constexpr int kLmax = kPoolLmax;

int async_copy(ws_engine* e, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* what) {
  if (bytes == 0) return WS_OK;
  if (e->dry) {
    if (kind != hipMemcpyDeviceToHost) memcpy(dst, src, bytes);      // nothing was computed: a caller's buffer stays untouched
    return WS_OK;
  }
  if (hipMemcpyAsync(dst, src, bytes, kind, e->stream) != hipSuccess) {
    set_err("ws_engine_pool: %s failed", what);
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

int sync_pool(ws_engine* e) {
  if (!e->dry && hipStreamSynchronize(e->stream) != hipSuccess) {
    set_err("ws_engine_pool: the device reported an error");
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

// One group: row i of the rectangle is slot g.slot[i] with g.tc[i] >= 1 frames from its frame k on; Tc = max tc.  The
// staging block is zero-filled, so a flush's frames read zeros behind the slot's last sample, as the whole-utterance
// encoder does.  The slots' positions move here; their pending samples are dropped by the caller.
int run_group(ws_pool* p, PoolGroup& g) {
  ws_engine* e = p->e;
  const TasNet& t = e->tas;
  const int N = t.N, L = t.L, B = t.B, H = t.H, P = t.P, s = L / 2, A = static_cast<int>(g.slot.size()), Tc = g.Tc;
  const int pitch = (Tc - 1) * s + kLmax;
  const long long M = (long long)A * Tc;
  void* q = e->stream;
  const bool dio = p->device_io;
  if (!dio) g.stage.assign(size_t(A) * pitch, 0.f);
  g.t0.resize(A);
  for (int i = 0; i < A; ++i) {
    const PoolSlot& sl = p->slots[g.slot[i]];
    const size_t want = size_t(g.tc[i] - 1) * s + kLmax;
    if (!dio) memcpy(g.stage.data() + size_t(i) * pitch, sl.pend.data(), std::min(want, sl.pend.size()) * 4);
    g.t0[i] = sl.k;
  }
  if (!dio) g.est.assign(size_t(A) * Tc * s, 0.f);
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* x0 = a.alloc(size_t(A) * pitch);
  // the three tables in one block: t0 (8-byte entries) first, then slot and tc
  char* tab = reinterpret_cast<char*>(a.alloc(size_t(A) * 4));
  ws_rows_copy_row* d_rows = dio ? reinterpret_cast<ws_rows_copy_row*>(a.alloc(size_t(A) * 2 * sizeof(ws_rows_copy_row) / 4)) : nullptr;
  WS_PTR(!dio || d_rows);
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
  float* est = a.alloc(size_t(A) * Tc * s);
  WS_PTR(x0 && tab && cat && st0 && xa && xb && c && y2 && st2 && m && sm && fr && est);
  long long* d_t0 = reinterpret_cast<long long*>(tab);
  int* d_slot = reinterpret_cast<int*>(tab + size_t(A) * 8);
  int* d_tc = d_slot + A;
  int rc;
  float* const state = reinterpret_cast<float*>(p->state);
  const long long state_floats = static_cast<long long>(p->state_bytes / 4);
  if (dio) {
    // the rectangle is gathered from the slots' pending samples on the device, zeros behind them (the staging block's zero fill);
    // the estimates are scattered behind each slot's destination: two table-driven copies in place of the upload and download
    g.gather.resize(A), g.scatter.resize(A);
    for (int i = 0; i < A; ++i) {
      const int want = (g.tc[i] - 1) * s + kLmax, len = std::min(want, g.src_have[i]);
      g.gather[i] = ws_rows_copy_row{g.src_off[i], (long long)i * pitch, len, pitch - len};
      g.scatter[i] = ws_rows_copy_row{(long long)i * Tc * s, g.dst_off[i], g.tc[i] * s, 0};
    }
    if ((rc = async_copy(e, d_rows, g.gather.data(), size_t(A) * sizeof(ws_rows_copy_row), hipMemcpyHostToDevice, "table upload")) != WS_OK) return rc;
    if ((rc = async_copy(e, d_rows + A, g.scatter.data(), size_t(A) * sizeof(ws_rows_copy_row), hipMemcpyHostToDevice, "table upload")) != WS_OK) return rc;
    WS_RUN(e, ws_rows_copy_fwd(g.gather.data(), d_rows, A, state, state_floats, x0, (long long)A * pitch, q));
  } else if ((rc = async_copy(e, x0, g.stage.data(), g.stage.size() * 4, hipMemcpyHostToDevice, "host-to-device copy")) != WS_OK) {
    return rc;
  }
  if ((rc = async_copy(e, d_t0, g.t0.data(), size_t(A) * 8, hipMemcpyHostToDevice, "table upload")) != WS_OK) return rc;
  if ((rc = async_copy(e, d_slot, g.slot.data(), size_t(A) * 4, hipMemcpyHostToDevice, "table upload")) != WS_OK) return rc;
  if ((rc = async_copy(e, d_tc, g.tc.data(), size_t(A) * 4, hipMemcpyHostToDevice, "table upload")) != WS_OK) return rc;
  const int Ls[3] = {L, 80, kLmax};
  for (int i = 0; i < 3; ++i) {
    TasGemm gm;
    gm.A = x0, gm.a_div = Tc, gm.a_s1 = pitch, gm.lda = s, gm.M = M, gm.K = Ls[i], gm.W = p->enc_w[i], gm.ldw = Ls[i], gm.N = N;
    gm.bias = p->enc_b[i], gm.act = 2, gm.C = cat + (long long)i * N, gm.ldc = 3 * N;
    if ((rc = tas_gemm(e, gm)) != WS_OK) return rc;
  }
  if ((rc = tas_row_stats(e, cat, M, 3 * N, st0)) != WS_OK) return rc;
  {
    TasGemm gm;
    gm.A = cat, gm.lda = 3 * N, gm.M = M, gm.K = 3 * N, gm.W = p->proj_w, gm.ldw = 3 * N, gm.N = B, gm.bias = p->proj_b, gm.C = xa, gm.ldc = B;
    gm.stats = st0, gm.gamma = p->ln_g, gm.beta = p->ln_b, gm.st_div1 = 1;
    if ((rc = tas_gemm(e, gm)) != WS_OK) return rc;
  }
  float *x = xa, *other = xb;
  for (const StreamBlock& b : p->blocks) {
    if (p->block_kernel) {
      WS_RUN(e, ws_tcn_block_stream_rows_fwd(x, b.rb, b.w1, b.ldw, b.rb ? nullptr : b.b1, b.a1, b.g1, b.be1, b.wd, b.bd, b.a2, b.g2,
                                             b.be2, b.w3, b.b3, A, Tc, B, H, P, b.dil, kLnEps, p->nslots, d_slot, d_t0, d_tc, b.cap,
                                             b.ring, other, q));
      std::swap(x, other);
      continue;
    }
    TasGemm gm;
    gm.A = x, gm.lda = B, gm.M = M, gm.K = B, gm.W = b.w1, gm.ldw = b.ldw, gm.N = H, gm.bias = b.rb ? nullptr : b.b1, gm.C = c, gm.ldc = H;
    if ((rc = tas_gemm(e, gm)) != WS_OK) return rc;
    WS_RUN(e, ws_tcn_mid_stream_rows_fwd(c, b.rb, b.a1, b.g1, b.be1, b.wd, b.bd, b.a2, A, Tc, H, P, b.dil, kLnEps, p->nslots, d_slot,
                                         d_t0, d_tc, b.cap, b.ring, y2, st2, q));
    TasGemm o;
    o.A = y2, o.lda = H, o.M = M, o.K = H, o.W = b.w3, o.ldw = H, o.N = B, o.bias = b.b3, o.C = other, o.ldc = B, o.R = x;
    o.stats = st2, o.gamma = b.g2, o.beta = b.be2, o.st_div1 = 1;
    if ((rc = tas_gemm(e, o)) != WS_OK) return rc;
    std::swap(x, other);
  }
  {
    TasGemm gm;
    gm.A = x, gm.lda = B, gm.M = M, gm.K = B, gm.W = p->mask_w, gm.ldw = B, gm.N = N, gm.bias = p->mask_b, gm.act = 2, gm.C = m, gm.ldc = N;
    if ((rc = tas_gemm(e, gm)) != WS_OK) return rc;
    WS_RUN(e, ws_maskmul_fwd(cat, 3 * N, m, M, N, sm, q));
    TasGemm d;
    d.A = sm, d.lda = N, d.M = M, d.K = N, d.W = t.dec_wt, d.ldw = N, d.N = L, d.C = fr, d.ldc = L;
    if ((rc = tas_gemm(e, d)) != WS_OK) return rc;
    WS_RUN(e, ws_ola_stream_rows_fwd(fr, p->dec_b, A, Tc, L, s, p->nslots, d_slot, d_t0, d_tc, p->carry, est, q));
  }
  if (dio) {
    WS_RUN(e, ws_rows_copy_fwd(g.scatter.data(), d_rows + A, A, est, (long long)A * Tc * s, state, state_floats, q));
  } else if ((rc = async_copy(e, g.est.data(), est, g.est.size() * 4, hipMemcpyDeviceToHost, "device-to-host copy")) != WS_OK) {
    return rc;
  }
  for (int i = 0; i < A; ++i) {
    PoolSlot& sl = p->slots[g.slot[i]];
    const size_t used = std::min(size_t(g.tc[i]) * s, sl.pend.size());
    sl.pend.erase(sl.pend.begin(), sl.pend.begin() + used);
    sl.k += g.tc[i];
  }
  a.release(mk);
  return WS_OK;
}

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
    if ((rc = run_group(p, p->groups.back())) != WS_OK) return rc;
  }
}

int check_pool(const ws_pool* p, const char* who) {
  if (!p || !p->e) {
    set_err("%s: null pool", who);
    return WS_ERR_INVALID;
  }
  for (int i = 0; i < p->nslots; ++i)
    if (p->slots[i].failed) {
      set_err("%s: an earlier call on this pool failed half way with slot %d in it; detach the slots of that call (or close the pool)",
              who, i);
      return WS_ERR_INVALID;
    }
  return WS_OK;
}

void free_pool(ws_pool* p) {
  if (p->state) {
    if (p->e->dry)
      free(p->state);
    else
      (void)hipFree(p->state);
  }
  delete p;
}

}  // namespace

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
  const TasNet& t = e->tas;
  const int L = t.L, s = L / 2, H = t.H, G = max_chunk_frames;
  if ((long long)slots * G * 3 * t.N > 0x7fffffffLL || (long long)slots * ((long long)(t.P - 1) * (1 << (t.X - 1)) + G) * H > 0x7fffffffLL) {
    set_err("%s: slots=%d with max_chunk_frames=%d reaches 2^31 elements in one buffer", who, slots, G);
    return WS_ERR_INVALID;
  }
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  ws_pool* p = new ws_pool();
  p->e = e, p->nslots = slots, p->G = G, p->block_kernel = (flags & WS_STREAM_BLOCK_KERNEL) != 0;
  p->slots.resize(slots);
  // ---- the state block: rings, carry, its reset image, embedding, row biases; 256-byte aligned parts ----
  const int nblocks = t.R * t.X;
  std::vector<size_t> off;
  size_t total = 0;
  auto part = [&](size_t nfloats) {
    off.push_back(total);
    total += Arena::round_up(nfloats * 4);
  };
  for (int r = 0; r < t.R; ++r)
    for (int k = 0; k < t.X; ++k) part(size_t(slots) * ((size_t)(t.P - 1) * (1 << k) + G) * H);
  part(size_t(slots) * (L - s));
  part(size_t(L - s));
  part(size_t(slots) * e->E);
  for (int r = 0; r < t.R; ++r) part(size_t(slots) * H);
  if (extra_floats) part(extra_floats);
  p->device_io = extra_floats != 0;
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
  auto at = [&](size_t i) { return reinterpret_cast<float*>(p->state + off[i]); };
  size_t si = nblocks;
  p->carry = at(si++), p->carry0 = at(si++), p->emb = at(si++);
  for (int r = 0; r < t.R; ++r) p->rb.push_back(at(si++));
  if (extra_floats && extra) *extra = at(si++);
  resolve_stream_weights(e, p);
  for (int r = 0; r < t.R; ++r)
    for (int k = 0; k < t.X; ++k) {
      StreamBlock& b = p->blocks[size_t(r) * t.X + k];
      b.cap = (t.P - 1) * b.dil + G, b.ring = at(size_t(r) * t.X + k), b.rb = k == 0 ? p->rb[r] : nullptr;
    }
  const std::vector<float> c0(size_t(L - s), e->host("decoder.decoder_1d_1.bias")[0]);   // the carry's reset image: the decoder bias
  if ((rc = to_device(e, p->carry0, c0.data(), c0.size() * 4)) != WS_OK) {
    free_pool(p);
    return rc;
  }
  e->stream_state_bytes = static_cast<long long>(total);
  *out = p;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_pool_attach(ws_pool* p, const void* enroll, int enroll_kind, int enroll_len, int* slot) {
  return pool_attach_impl(p, "ws_engine_pool_attach", enroll, enroll_kind, enroll_len, slot);
}

int wsrt::pool_attach_impl(ws_pool* p, const char* who, const void* enroll, int enroll_kind, int enroll_len, int* slot) {
  int rc = check_pool(p, who);
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  if (!enroll || !slot) {
    set_err("%s: bad arguments (enroll %s, slot %s)", who, enroll ? "given" : "NULL", slot ? "given" : "NULL");
    return WS_ERR_INVALID;
  }
  if ((rc = tasnet_check_enroll(e, enroll_kind, enroll_len)) != WS_OK) return rc;
  int id = 0;
  while (id < p->nslots && p->slots[id].state != PoolSlot::kFree) ++id;
  if (id == p->nslots) {
    set_err("%s: the pool is full: all %d slots are attached (detach one, or open a larger pool)", who, p->nslots);
    return WS_ERR_INVALID;
  }
  const TasNet& t = e->tas;
  const int L = t.L, s = L / 2, H = t.H, B = t.B;
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  // ---- the speaker stage for this one enrollment: embedding, SpeakerTransform, the stacks' row biases W_e e + b ----
  Arena& a = e->work;
  const Arena::Mark mk = a.mark();
  float* d_emb = a.alloc(size_t(e->E));
  const float* embp = nullptr;
  float* emb = p->emb + size_t(id) * e->E;
  rc = d_emb ? WS_OK : WS_ERR_LAUNCH;
  if (rc == WS_OK) rc = speaker_stage(e, enroll, enroll_kind, 1, enroll_len, enroll_len, nullptr, nullptr, d_emb);
  if (rc == WS_OK) rc = spk_transform(e, d_emb, 1, &embp);
  if (rc == WS_OK) rc = async_copy(e, emb, embp, size_t(e->E) * 4, hipMemcpyDeviceToDevice, "device copy");
  for (int r = 0; rc == WS_OK && r < t.R; ++r) {
    const StreamBlock& b = p->blocks[size_t(r) * t.X];
    rc = linear(e, emb, 1, e->E, b.w1 + B, B + e->E, H, b.b1, 0, p->rb[r] + size_t(id) * H);
  }
  // position 0: the carry is the bias image; the rings need no clearing (no term reads a frame before the start)
  if (rc == WS_OK) rc = async_copy(e, p->carry + size_t(id) * (L - s), p->carry0, size_t(L - s) * 4, hipMemcpyDeviceToDevice, "device copy");
  if (rc == WS_OK) rc = sync_pool(e);
  a.release(mk);
  if (rc != WS_OK) return rc;
  PoolSlot& sl = p->slots[id];
  sl = PoolSlot();
  sl.state = PoolSlot::kAttached;
  *slot = id;
  return WS_OK;
}

WS_ENGINE_API int ws_engine_pool_push(ws_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n,
                                      float* const* est, const int* est_cap, int* n_out) {
  int rc = check_pool(p, "ws_engine_pool_push");
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  const int L = e->tas.L, s = L / 2;
  if (n_active < 1 || !slots || !chunks || !n || !est || !est_cap || !n_out) {
    set_err("ws_engine_pool_push: bad arguments (n_active=%d >= 1%s)", n_active,
            slots && chunks && n && est && est_cap && n_out ? "" : ", a NULL array");
    return WS_ERR_INVALID;
  }
  std::vector<char> seen(p->nslots, 0);
  std::vector<long long> owed(n_active);
  for (int i = 0; i < n_active; ++i) {
    const int id = slots[i];
    if (id < 0 || id >= p->nslots || p->slots[id].state == PoolSlot::kFree) {
      set_err("ws_engine_pool_push: slot %d (entry %d) is not attached (the pool has %d slots)", id, i, p->nslots);
      return WS_ERR_INVALID;
    }
    if (p->slots[id].state == PoolSlot::kDone) {
      set_err("ws_engine_pool_push: slot %d (entry %d) was flushed (detach it, then attach the next stream)", id, i);
      return WS_ERR_INVALID;
    }
    if (seen[id]) {
      set_err("ws_engine_pool_push: slot %d is named twice (entry %d): one packet a slot in a push", id, i);
      return WS_ERR_INVALID;
    }
    seen[id] = 1;
    if (n[i] < 1 || !chunks[i]) {
      set_err("ws_engine_pool_push: entry %d (slot %d): n=%d >= 1, chunk %s", i, id, n[i], chunks[i] ? "given" : "NULL");
      return WS_ERR_INVALID;
    }
    const PoolSlot& sl = p->slots[id];
    const long long total = sl.n + n[i];
    const long long target = total >= kLmax ? (total - kLmax) / s + 1 : 0;
    owed[i] = target - sl.k;
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
  if ((rc = sync_pool(e)) != WS_OK) return rc;       // the one host synchronisation of a push
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
  int rc = check_pool(p, "ws_engine_pool_flush");
  if (rc != WS_OK) return rc;
  ws_engine* e = p->e;
  const int L = e->tas.L, s = L / 2;
  if (slot < 0 || slot >= p->nslots || p->slots[slot].state == PoolSlot::kFree) {
    set_err("ws_engine_pool_flush: slot %d is not attached (the pool has %d slots)", slot, p->nslots);
    return WS_ERR_INVALID;
  }
  PoolSlot& sl = p->slots[slot];
  if (sl.state == PoolSlot::kDone) {
    set_err("ws_engine_pool_flush: slot %d was flushed already (detach it, then attach the next stream)", slot);
    return WS_ERR_INVALID;
  }
  if (sl.n < L) {
    set_err("ws_engine_pool_flush: slot %d: %lld samples were pushed, fewer than the encoder window L = %d", slot, sl.n, L);
    return WS_ERR_INVALID;
  }
  const long long target = (sl.n - L) / s + 1;
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
  if ((rc = async_copy(e, est + tail, p->carry + size_t(slot) * (L - s), size_t(L - s) * 4, hipMemcpyDeviceToHost,
                       "device-to-host copy")) != WS_OK)
    return rc;
  if ((rc = sync_pool(e)) != WS_OK) return rc;
  if (!e->dry)
    for (const PoolGroup& g : p->groups) memcpy(est + g.col[0], g.est.data(), size_t(g.tc[0]) * s * 4);
  p->groups.clear();
  sl.pend.clear();
  sl.failed = false;
  sl.state = PoolSlot::kDone;
  *n_out = static_cast<int>(emit);
  return WS_OK;
}

WS_ENGINE_API int ws_engine_pool_detach(ws_pool* p, int slot) {
  if (!p || !p->e) {
    set_err("ws_engine_pool_detach: null pool");
    return WS_ERR_INVALID;
  }
  if (slot < 0 || slot >= p->nslots || p->slots[slot].state == PoolSlot::kFree) {
    set_err("ws_engine_pool_detach: slot %d is not attached (the pool has %d slots)", slot, p->nslots);
    return WS_ERR_INVALID;
  }
  p->slots[slot] = PoolSlot();          // free, and no longer the slot of a half-finished call
  return WS_OK;
}

WS_ENGINE_API void ws_engine_pool_close(ws_pool* p) {
  if (!p) return;
  if (p->e && !p->e->dry) {
    (void)hipSetDevice(p->e->device);
    (void)hipStreamSynchronize(p->e->stream);
  }
  free_pool(p);
}

// ---- for the rate pool (rate_pool.cc) ----
int wsrt::pool_run_group(ws_pool* p, PoolGroup& g) { return run_group(p, g); }
int wsrt::pool_check(const ws_pool* p, const char* who) { return check_pool(p, who); }
void wsrt::pool_free(ws_pool* p) { free_pool(p); }
