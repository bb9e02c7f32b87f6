// =================================================================================================================
// Long recordings (ws_engine_separate_long): one mixture of n samples, K target speakers.  The mixture is cut
// into W overlapping windows of `window` samples (layout: include/wesep_hip.h, longform.hip -- the last window is aligned
// to the end, so every window has full length and every architecture's RECTANGULAR plan applies), the K * W rows go
// through the separator in groups of at most max_rows rows, and the estimates are cross-faded back into [K][n].
// Target-speaker extraction needs no permutation alignment between windows: the enrollment fixes which speaker comes out.
//   * the speaker stage runs once, over the K enrollments, or not at all (fixed embeddings / WS_ENROLL_SPEAKER); a group
//     gets the embedding of each of its rows uploaded;
//   * one ws_window_rows launch gathers the windows, one ws_xfade_ola launch blends the estimates, one copy goes to the host;
//   * the rows and the estimates [K][W][window] live below the arena mark that every group's forward is released to, so
//     the peak is one group's working set plus two copies of the windowed signal;
//   * a row is what ws_engine_separate makes of it: TF-GridNet scales a window by its own standard deviation and its
//     estimate back (the two kernels take the factors as a per-window table).
// =================================================================================================================
#include "engine_internal.h"

namespace wsrt {

// What ws_engine_separate_long demands of (window, overlap, max_rows), with its messages; ws_engine_live_open (live.cc) makes
// the same checks
int long_check_window(ws_engine* e, int window, int overlap, int max_rows) {
  int rc;
  if (max_rows < 1) {
    set_err("ws_engine_separate_long: max_rows = %d (at least one row per forward)", max_rows);
    return WS_ERR_INVALID;
  }
  // the window as a mixture of its own: the architecture's lower bound on T, with its message
  if ((rc = check_rows(e, true, 1, window)) != WS_OK) return rc;
  if (overlap < 0 || overlap > window / 2) {
    set_err("ws_engine_separate_long: overlap = %d outside [0, window / 2 = %d]", overlap, window / 2);
    return WS_ERR_INVALID;
  }
  if (e->arch == 1) {
    // T' = (T - L) / stride + 1 frames cover (T' - 1) stride + L samples; what is left of a row is the plan's zero
    // extension, not model output -- inside a recording that would be cross-faded in
    const int L = e->tas.L, stride = L / 2;
    if ((window - L) % stride != 0) {
      const int lo = L + (window - L) / stride * stride;
      set_err("ws_engine_separate_long: a Conv-TasNet window must be L + k * L / 2 samples (L = %d): window = %d leaves %d samples "
              "without model output; the nearest valid windows are %d and %d", L, window, window - lo, lo, lo + stride);
      return WS_ERR_INVALID;
    }
  }
  return WS_OK;
}

// ... and of a group of G rows of L samples and the K enrollments
int long_check_group(ws_engine* e, int G, int L, int K, int enroll_kind, int enroll_len, const int* enroll_lengths, int* Te,
                     std::vector<int>* te_row) {
  int rc;
  if ((rc = check_rows(e, true, G, L)) != WS_OK) return rc;       // the group's geometry against the plan's 2^31 guards
  if (enroll_lengths && e->arch != 0 && e->arch != 3) {
    set_err("ws_engine_separate_long: per-row enrollment lengths are built for pBSRNN (arch 0) and TF-GridNet (arch 3) only; "
            "this container holds arch %d", e->arch);
    return WS_ERR_INVALID;
  }
  return check_enroll(e, K, enroll_kind, enroll_len, enroll_lengths, Te, te_row);
}

int separate_long(ws_engine* e, const float* mix, int n, int K, const void* enroll, int enroll_kind, int enroll_len,
                  const int* enroll_lengths, int window, int overlap, int max_rows, float* est) {
  int rc = check_engine(e, "ws_engine_separate_long");
  if (rc != WS_OK) return rc;
  if (!mix || !enroll || !est || n < 1 || K < 1) {
    set_err("ws_engine_separate_long: bad arguments (n=%d, K=%d)", n, K);
    return WS_ERR_INVALID;
  }
  if ((rc = long_check_window(e, window, overlap, max_rows)) != WS_OK) return rc;
  const int H = window - overlap;
  const long long W64 = n <= window ? 1 : 1 + ((long long)n - window + H - 1) / H, rows64 = W64 * K;
  if (rows64 > 0x7fffffffLL) {
    set_err("ws_engine_separate_long: %lld windows x %d speakers: more rows than an int holds", W64, K);
    return WS_ERR_INVALID;
  }
  const int W = static_cast<int>(W64), rows = static_cast<int>(rows64), L = n < window ? n : window;
  if (W == 1 && K <= max_rows) {
    // the recording fits one window: ws_engine_separate on [K][n] (the speaker stage included), bit for bit
    std::vector<float> m(size_t(K) * n);
    for (int k = 0; k < K; ++k) memcpy(m.data() + size_t(k) * n, mix, size_t(n) * 4);
    if ((rc = separate_impl(e, m.data(), K, n, nullptr, enroll, enroll_kind, enroll_len, enroll_lengths, est)) != WS_OK) return rc;
    e->long_windows = e->long_forwards = 1;
    return WS_OK;
  }
  const int G = rows < max_rows ? rows : max_rows;
  int Te = enroll_len;
  std::vector<int> te_row;
  if ((rc = long_check_group(e, G, L, K, enroll_kind, enroll_len, enroll_lengths, &Te, &te_row)) != WS_OK) return rc;

  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  Arena& a = e->work;
  a.reset();
  const int E = e->E;
  // the K embeddings on the host: the caller's, or the speaker stage's (one pass over the K enrollments)
  std::vector<float> emb(size_t(K) * E);
  if (enroll_kind == WS_ENROLL_EMBEDDING || enroll_kind == WS_ENROLL_SPEAKER) {
    memcpy(emb.data(), enroll, emb.size() * 4);
  } else {
    float* d_emb = a.alloc(emb.size());
    WS_PTR(d_emb);
    if ((rc = speaker_stage(e, enroll, enroll_kind, K, enroll_len, Te, enroll_lengths, te_row.data(), d_emb)) != WS_OK) return rc;
    if ((rc = to_host(e, emb.data(), d_emb, emb.size() * 4)) != WS_OK) return rc;
    a.reset();
  }
  float* d_x = a.alloc(size_t(n));
  float* d_rows = a.alloc(size_t(rows) * L);
  float* d_y = a.alloc(size_t(rows) * L);
  float* d_out = a.alloc(size_t(K) * n);
  WS_PTR(d_x && d_rows && d_y && d_out);
  if ((rc = to_device(e, d_x, mix, size_t(n) * 4)) != WS_OK) return rc;
  // TF-GridNet: every window is scaled by its own standard deviation and its estimate back (tfgridnet.py:222-226,292)
  float *d_inv = nullptr, *d_std = nullptr;
  if (e->arch == 3) {
    std::vector<float> tab(2 * size_t(W));
    for (int w = 0; w < W; ++w) {
      const long long start = std::min((long long)w * H, (long long)n - L);
      row_std_scale(mix + start, L, &tab[size_t(W) + w], nullptr);
      tab[w] = 1.0f / tab[size_t(W) + w];
    }
    d_inv = upload(e, a, tab.data(), tab.size());
    WS_PTR(d_inv);
    d_std = d_inv + W;
  }
  WS_RUN(e, ws_window_rows(d_x, n, W, window, H, K, d_inv, d_rows, e->stream));
  const Arena::Mark group_mark = a.mark();
  std::vector<float> emb_g(size_t(G) * E);
  for (int g0 = 0; g0 < rows; g0 += G) {
    const int Gn = rows - g0 < G ? rows - g0 : G;
    a.release(group_mark);
    for (int r = 0; r < Gn; ++r) memcpy(emb_g.data() + size_t(r) * E, emb.data() + size_t((g0 + r) / W) * E, size_t(E) * 4);
    float* d_emb_g = upload(e, a, emb_g.data(), size_t(Gn) * E);
    WS_PTR(d_emb_g);
    const float* in = d_rows + size_t(g0) * L;
    float* out = d_y + size_t(g0) * L;
    rc = e->arch == 1   ? tasnet_device(e, in, Gn, L, d_emb_g, nullptr, 0, out)
         : e->arch == 2 ? dpccn_device(e, in, Gn, L, d_emb_g, out)
         : e->arch == 3 ? gridnet_device(e, in, Gn, L, d_emb_g, out)
                        : separate_device(e, in, Gn, L, d_emb_g, out);
    if (rc != WS_OK) return rc;
    ++e->long_forwards;
  }
  a.release(group_mark);
  WS_RUN(e, ws_xfade_ola(d_y, K, W, window, overlap, n, d_std, d_out, e->stream));
  if ((rc = to_host(e, est, d_out, size_t(K) * n * 4)) != WS_OK) return rc;
  if ((rc = note_cluster_status(e)) != WS_OK) return rc;
  e->long_windows = W;
  a.reset();
  a.consolidate();
  return WS_OK;
}

}  // namespace wsrt
