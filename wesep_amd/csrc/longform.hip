// Windowed separation of long recordings (runtime/longform.cc): one mixture of n samples is cut into W
// overlapping windows of S samples, the windows go through a separator as the rows of a rectangle, and the estimates are
// cross-faded back into one signal.  The layout is a pure function of (n, S, O), O the overlap, hop H = S - O:
//   n <= S:  one window [0, n) of L = n samples;
//   else:    W = 1 + ceil((n - S) / H) windows of L = S samples, start_w = min(w * H, n - S) -- the last window is aligned
//            to the end of the recording, so every window has full length (it may overlap its predecessor by up to S - 1
//            samples, and a third window with it).
// ws_xfade_stream_fwd is ws_xfade_ola over a range of absolute positions, its windows read from a ring: the live form
// (runtime/live.cc).  Both cross-fades inline ONE body, lf_blend, so their arithmetic cannot differ.
// ws_window_slots_fwd and ws_xfade_stream_rows_fwd are the table-driven forms of the gather and of the ring cross-fade for the
// live pool (runtime/live_pool.cc): row i names its own source, destination, ring and layout; same bodies, same bits.
// ws_tail_emit_rows_fwd is the emission of the tail pool (runtime/tail_pool.cc), a rule of its own: the newest part of a trailing
// window, its first samples cross-faded with what the window before held back.
// The kernels compute the starts themselves; no table of them exists.  Two HBM-bound passes: ws_window_rows gathers the
// rows (once per target speaker), ws_xfade_ola blends the estimates with linear ramps over the O overlapping samples,
// normalised by the sum of the weights that cover a sample.  Offsets are 64-bit (n up to 2^31 - 1); sums run in ascending
// window order, no atomics; plain C++, no packed FP32.
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

inline int lf_blocks(long long n, int per = 256, int cap = 32768) {   // grid-stride kernels: the cap of ragged_grid.hip
  long long b = (n + per - 1) / per;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

// the window count of (n, S, H); 1 when the recording fits one window
inline long long lf_windows(long long n, long long S, long long H) { return n <= S ? 1 : 1 + (n - S + H - 1) / H; }

// rows[(k * W + w)][j] = x[start_w + j] * (scale ? scale[w] : 1), k < reps.  A thread owns four consecutive samples of one
// window and writes them to all `reps` copies.  start_{W-1} = n - S is any sample, so the source is read with scalar loads
// (consecutive lanes read consecutive floats either way); a destination quad is stored as 16 bytes where its address
// allows it -- every quad when L % 4 == 0 -- and sample by sample otherwise.
__global__ __launch_bounds__(256) void window_rows_kernel(const float* __restrict__ x, long long n, int W, int L, int H,
                                                          int reps, const float* __restrict__ scale,
                                                          float* __restrict__ rows) {
  const int L4 = (L + 3) >> 2;
  const long long total = (long long)W * L4, last = n - L;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int w = (int)(idx / L4), j0 = (int)(idx - (long long)w * L4) * 4;
    const long long start = min((long long)w * H, last);
    const float* src = x + start + j0;
    const int cnt = min(4, L - j0);
    const float sv = scale ? scale[w] : 1.f;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = q < cnt ? src[q] : 0.f;
    if (scale) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] *= sv;
    }
    for (int k = 0; k < reps; ++k) {
      float* dst = rows + ((long long)k * W + w) * L + j0;
      if (cnt == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const f32x4 t = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(dst) = t;
      } else {
        for (int q = 0; q < cnt; ++q) dst[q] = v[q];
      }
    }
  }
}

// weight of window w at its local position j: a ramp up over the first O samples unless it is the first window, a ramp
// down over the last O unless it is the last.  Two regular neighbours: (j' + 1) / (O + 1) + (O - j') / (O + 1) = 1.
__device__ __forceinline__ float lf_weight(long long w, long long W, int j, int L, float o1) {
#pragma clang fp contract(off)
  float g = 1.f;
  if (w > 0) g = fminf(1.f, (float)(j + 1) / o1);
  if (w < W - 1) g *= fminf(1.f, (float)(L - j) / o1);
  return g;
}

// One output sample i of one target, the body of both cross-fade kernels: (sum over the windows that cover i, ascending w,
// of g_w y_w) / (sum of the same g_w); y_w taken times scale[.] where a table is given.  The regular windows that cover i
// are w in [i < L ? 0 : (i - L) / H + 1, min(W - 2, i / H)]; the end-aligned last window covers i >= last = n - L (`last`
// beyond every i: there is none).  Every g is positive, so the sum of the weights is, too.  Window w's estimate is
// yk[slot * pitch ..] and its factor scale[slot], slot = w for a whole recording (kCap = false) and w % cap in a ring.
// The roundings are spelled out -- g = fl(up * down), v = fl(y * scale), num = fma(g, v, num), den = fl(den + g) -- and the
// compiler is kept from contracting others, so what is known about a window at compile time cannot change a bit.
template <bool kCap>
__device__ __forceinline__ float lf_blend(const float* __restrict__ yk, const float* __restrict__ scale, long long i,
                                          long long W, int L, int H, float o1, long long last, long long pitch, int cap) {
#pragma clang fp contract(off)
  float num = 0.f, den = 0.f;
  const long long w_lo = i < L ? 0 : (i - L) / H + 1, w_hi = min(W - 2, i / H);
  for (long long w = w_lo; w <= w_hi; ++w) {
    const int j = (int)(i - w * H);                     // in [0, L): w * H <= i < w * H + L
    const float g = lf_weight(w, W, j, L, o1);
    const long long slot = kCap ? w % cap : w;
    float v = yk[slot * pitch + j];
    if (scale) v *= scale[slot];
    num = __builtin_fmaf(g, v, num);
    den += g;
  }
  if (i >= last) {
    const int j = (int)(i - last);
    const float g = lf_weight(W - 1, W, j, L, o1);
    const long long slot = kCap ? (W - 1) % cap : W - 1;
    float v = yk[slot * pitch + j];
    if (scale) v *= scale[slot];
    num = __builtin_fmaf(g, v, num);
    den += g;
  }
  return num / den;
}

// out[k][i] = lf_blend of the K * n samples of a whole recording, y [K][W][L].  One thread per output sample: consecutive
// lanes read consecutive floats of each window.
__global__ __launch_bounds__(256) void xfade_ola_kernel(const float* __restrict__ y, int K, int W, int L, int H, int O,
                                                        long long n, const float* __restrict__ scale,
                                                        float* __restrict__ out) {
  const long long total = (long long)K * n, last = n - L;
  const float o1 = (float)(O + 1);
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(idx / n);
    const long long i = idx - (long long)k * n;
    out[idx] = lf_blend<false>(y + (long long)k * W * L, scale, i, W, L, H, o1, last, L, 0);
  }
}

// The same over the absolute positions [i0, i0 + count) of a recording whose windows arrive one by one: ring [K][cap][S]
// holds window w's estimate in slot w % cap.  W, last: the final layout at a flush; before it W = windows run + 1 and last
// lies beyond every position, so every covering window is regular with its tail ramp and no end-aligned term exists.
// out[k][i - i0], row pitch ld_out.  A slot is read only for a window that covers the sample.
__global__ __launch_bounds__(256) void xfade_stream_kernel(const float* __restrict__ ring, int K, int cap, int S, int L, int H,
                                                           int O, long long W, long long last, long long i0, long long count,
                                                           const float* __restrict__ scale_ring, float* __restrict__ out,
                                                           long long ld_out) {
  const long long total = (long long)K * count;
  const float o1 = (float)(O + 1);
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(idx / count);
    const long long c = idx - (long long)k * count;
    out[(long long)k * ld_out + c] = lf_blend<true>(ring + (long long)k * cap * S, scale_ring, i0 + c, W, L, H, o1, last, S, cap);
  }
}

// ---- rows forms (the live pool, runtime/live_pool.cc): one launch for A table rows that share nothing but the launch.  Grid
// (blocks of the largest row, A); a workgroup beyond its own row's count leaves at once.

// Row i of the table is one window of one slot: window_rows_kernel with the start, the destination and the factor read from
// the table.  A thread owns four consecutive samples; scalar loads (no start alignment is assumed), a 16-byte store where the
// destination allows it.  scale == 1 is a copy, as window_rows_kernel without a factor table.
__global__ __launch_bounds__(256) void window_slots_kernel(const ws_window_slot_row* __restrict__ rows, const float* __restrict__ src,
                                                           float* __restrict__ dst) {
  const ws_window_slot_row r = rows[blockIdx.y];
  const long long q0 = (long long)blockIdx.x * 256;
  const int L4 = (r.len + 3) >> 2;
  if (q0 >= L4) return;
  const int quad = (int)q0 + (int)threadIdx.x;
  if (quad >= L4) return;
  const int j0 = quad * 4, cnt = min(4, r.len - j0);
  const float* s = src + r.src_off + j0;
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = q < cnt ? s[q] : 0.f;
  if (r.scale != 1.f) {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] *= r.scale;
  }
  float* d = dst + r.dst_off + j0;
  if (cnt == 4 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
    const f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(d) = t;
  } else {
    for (int q = 0; q < cnt; ++q) d[q] = v[q];
  }
}

// Row i of the table is one target of one slot: xfade_stream_kernel with K = 1 on the row's own ring, factor ring, range and
// layout.  The layout (L, Wk, last) is derived exactly as ws_xfade_stream_fwd derives it; one thread per output sample.
__global__ __launch_bounds__(256) void xfade_stream_rows_kernel(const ws_xfade_stream_row* __restrict__ rows, int S, int O, int cap,
                                                                const float* __restrict__ ring, const float* __restrict__ scale_ring,
                                                                float* __restrict__ out) {
  const ws_xfade_stream_row r = rows[blockIdx.y];
  const long long c0 = (long long)blockIdx.x * 256;
  if (c0 >= r.count) return;
  const long long c = c0 + threadIdx.x;
  if (c >= r.count) return;
  int L = S;
  long long Wk = r.windows_run + 1, last = 0x7fffffffffffffffLL;
  if (r.final) {
    if (r.n < S) L = (int)r.n;
    Wk = r.W, last = r.n - L;
  }
  const float o1 = (float)(O + 1);
  out[r.out_off + c] = lf_blend<true>(ring + r.ring_off, r.scale_off >= 0 ? scale_ring + r.scale_off : nullptr, r.i0 + c, Wk, L, S - O,
                                      o1, last, S, cap);
}

// ---- tail pool (runtime/tail_pool.cc): row i is one target of one slot at a tick.  Of the window's estimate y [L] it emits the m
// samples from local index p on -- the first h of them cross-faded with what the last window held back for the same positions --
// and holds the last c_new back in turn.  With v = fl(y * scale) (scale == 1: y itself):
//   out[j]  = j < h ? fma(ramp[j], fl(v - hold_in[j]), hold_in[j]) : v,   j < m
//   hold_out[q] = fl(y[p + m + q] * scale),                               q < c_new
// the roundings spelled out as in lf_blend, contraction off.  A thread owns four consecutive floats of ONE destination, counted
// from the 16-byte boundary at or below the destination's first float (sh = the floats between the two), so every whole quad is
// stored as 16 bytes wherever the destination starts; y and hold_in are read with scalar loads (no alignment is assumed).  The
// out quads come first, then the hold quads; tail_quads is the count the host sizes the grid with.
__host__ __device__ inline int tail_shift(const float* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }
__host__ __device__ inline int tail_quads(int n, int sh) { return n > 0 ? (n + sh + 3) >> 2 : 0; }

__global__ __launch_bounds__(256) void tail_emit_rows_kernel(const ws_tail_emit_row* __restrict__ rows, const float* __restrict__ ramp,
                                                             const float* __restrict__ y, const float* __restrict__ hold_in,
                                                             float* __restrict__ hold_out, float* __restrict__ out) {
#pragma clang fp contract(off)
  const ws_tail_emit_row r = rows[blockIdx.y];
  float* const d_out = out + r.out_off;
  float* const d_hold = hold_out + r.hold_out_off;
  const int sh_o = tail_shift(d_out), sh_h = tail_shift(d_hold);
  const int nq_o = tail_quads(r.m, sh_o), nq_h = tail_quads(r.c_new, sh_h);
  const long long q0 = (long long)blockIdx.x * 256;
  if (q0 >= nq_o + nq_h) return;
  int quad = (int)q0 + (int)threadIdx.x;
  if (quad >= nq_o + nq_h) return;
  const bool held = quad >= nq_o;            // this quad belongs to the new hold
  if (held) quad -= nq_o;
  const int n = held ? r.c_new : r.m, j0 = quad * 4 - (held ? sh_h : sh_o);
  const float* src = y + r.y_off + r.p + (held ? r.m : 0);
  const float* hin = hold_in + r.hold_in_off;
  float* dst = held ? d_hold : d_out;
  const int h = held ? 0 : r.h;
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = j0 + q;
    float t = 0.f;
    if (j >= 0 && j < n) {
      t = src[j];
      if (r.scale != 1.f) t = t * r.scale;
      if (j < h) {
        const float hd = hin[j];
        const float d = t - hd;
        t = __builtin_fmaf(ramp[j], d, hd);
      }
    }
    v[q] = t;
  }
  if (j0 >= 0 && j0 + 4 <= n) {              // a whole quad: 16-byte aligned by the choice of j0
    const f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst + j0) = t;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (j0 + q >= 0 && j0 + q < n) dst[j0 + q] = v[q];
  }
}

// Address ranges of one rows call: a written range may meet no other range of the call, read or written (another workgroup
// of the launch owns it).  Ranges that are only read may share.
struct LfSpan {
  uintptr_t lo, hi;
  int row;
  bool write;
  const char* name;
};

inline LfSpan lf_span(const float* p, long long off, long long n, int row, bool write, const char* name) {
  return LfSpan{reinterpret_cast<uintptr_t>(p + off), reinterpret_cast<uintptr_t>(p + off + n), row, write, name};
}

int lf_spans_disjoint(const char* who, std::vector<LfSpan>& v) {
  std::sort(v.begin(), v.end(), [](const LfSpan& a, const LfSpan& b) { return a.lo < b.lo; });
  const LfSpan *far_r = nullptr, *far_w = nullptr;      // the read / written range that ends last so far
  for (const LfSpan& x : v) {
    const LfSpan* hit = far_w && x.lo < far_w->hi ? far_w : (x.write && far_r && x.lo < far_r->hi ? far_r : nullptr);
    WS_REQUIRE(!hit, "%s: row %d: its %s range overlaps the %s range of row %d", who, x.row, x.name, hit->name, hit->row);
    const LfSpan*& far = x.write ? far_w : far_r;
    if (!far || x.hi > far->hi) far = &x;
  }
  return WS_OK;
}

}  // namespace

extern "C" int ws_window_slots_fwd(const ws_window_slot_row* rows, const ws_window_slot_row* d_rows, int A, const float* src,
                                   long long n_src, float* dst, long long n_dst, void* stream) {
  const char* who = "ws_window_slots_fwd";
  WS_REQUIRE(rows && d_rows && src && dst, "%s: rows, d_rows, src or dst is NULL", who);
  WS_REQUIRE(A > 0 && A <= 65535, "%s: A=%d is outside [1, 65535]", who, A);
  WS_REQUIRE(n_src >= 0 && n_dst >= 0, "%s: an arena length is negative (src %lld, dst %lld)", who, n_src, n_dst);
  std::vector<LfSpan> spans;
  spans.reserve((size_t)A * 2);
  long long nb_max = 0;
  for (int i = 0; i < A; ++i) {
    const ws_window_slot_row& r = rows[i];
    WS_REQUIRE(r.len > 0 && (long long)r.len + 1024 < (1LL << 31), "%s: row %d: bad args (len=%d in [1, 2^31 - 1024))", who, i, r.len);
    WS_REQUIRE(r.src_off >= 0 && r.src_off <= n_src - r.len, "%s: row %d: src [%lld, %lld + %d) leaves the arena of %lld floats", who, i,
               r.src_off, r.src_off, r.len, n_src);
    WS_REQUIRE(r.dst_off >= 0 && r.dst_off <= n_dst - r.len, "%s: row %d: dst [%lld, %lld + %d) leaves the arena of %lld floats", who, i,
               r.dst_off, r.dst_off, r.len, n_dst);
    spans.push_back(lf_span(src, r.src_off, r.len, i, false, "src"));
    spans.push_back(lf_span(dst, r.dst_off, r.len, i, true, "dst"));
    nb_max = std::max(nb_max, (((long long)r.len + 3) / 4 + 255) / 256);
  }
  const int rc = lf_spans_disjoint(who, spans);
  if (rc != WS_OK) return rc;
  hipLaunchKernelGGL(window_slots_kernel, dim3((unsigned)nb_max, (unsigned)A), dim3(256), 0, (hipStream_t)stream, d_rows, src, dst);
  return ws_check_launch(who);
}

extern "C" int ws_xfade_stream_rows_fwd(const ws_xfade_stream_row* rows, const ws_xfade_stream_row* d_rows, int A, int S, int O, int cap,
                                        const float* ring, long long n_ring, const float* scale_ring, long long n_scale, float* out,
                                        long long n_out, void* stream) {
  const char* who = "ws_xfade_stream_rows_fwd";
  WS_REQUIRE(rows && d_rows && ring && out, "%s: rows, d_rows, ring or out is NULL", who);
  WS_REQUIRE(A > 0 && A <= 65535, "%s: A=%d is outside [1, 65535]", who, A);
  WS_REQUIRE(S > 0 && cap > 0, "%s: bad args (S=%d, cap=%d)", who, S, cap);
  WS_REQUIRE(O >= 0 && O <= S / 2, "%s: overlap O=%d outside [0, S / 2] (S=%d)", who, O, S);
  WS_REQUIRE(n_ring >= 0 && n_scale >= 0 && n_out >= 0, "%s: an arena length is negative (ring %lld, scale_ring %lld, out %lld)", who,
             n_ring, n_scale, n_out);
  const long long H = S - O;
  std::vector<LfSpan> spans;
  spans.reserve((size_t)A * 3);
  long long nb_max = 0;
  for (int i = 0; i < A; ++i) {
    const ws_xfade_stream_row& r = rows[i];
    WS_REQUIRE(r.i0 >= 0 && r.count >= 0 && r.windows_run >= 0 && r.count + 256 < (1LL << 31),
               "%s: row %d: bad range (i0=%lld, count=%lld below 2^31 - 256, windows_run=%lld)", who, i, r.i0, r.count, r.windows_run);
    const long long end = r.i0 + r.count;
    long long Wk, last;                                      // what the kernel takes as the row's layout
    int L = S;
    if (r.final) {
      WS_REQUIRE(r.n > 0 && r.W == lf_windows(r.n, S, H) && r.windows_run == r.W,
                 "%s: row %d: a final range needs all W=%lld windows of (n=%lld, S=%d, O=%d) run: %lld windows, %lld run", who, i, r.W, r.n, S,
                 O, r.n > 0 ? lf_windows(r.n, S, H) : 0LL, r.windows_run);
      WS_REQUIRE(end <= r.n, "%s: row %d: the range [%lld, %lld) reaches past the recording's n=%lld samples", who, i, r.i0, end, r.n);
      if (r.n < S) L = (int)r.n;
      Wk = r.W, last = r.n - L;
    } else {
      const long long emitted = r.windows_run > 0 ? (r.windows_run - 1) * H : 0;
      WS_REQUIRE(end <= emitted, "%s: row %d: the range [%lld, %lld) reaches past the %lld samples that the %lld windows run make final "
                 "(pass the final layout at a flush)", who, i, r.i0, end, emitted, r.windows_run);
      Wk = r.windows_run + 1, last = 0x7fffffffffffffffLL;
    }
    WS_REQUIRE(r.ring_off >= 0 && r.ring_off <= n_ring - (long long)cap * S, "%s: row %d: ring [%lld, %lld + %d * %d) leaves the arena of %lld floats",
               who, i, r.ring_off, r.ring_off, cap, S, n_ring);
    WS_REQUIRE(r.scale_off == -1 || (scale_ring && r.scale_off >= 0 && r.scale_off <= n_scale - cap),
               "%s: row %d: scale_ring [%lld, %lld + %d) leaves the arena of %lld floats%s (-1: no factors)", who, i, r.scale_off, r.scale_off,
               cap, n_scale, scale_ring ? "" : ", and scale_ring is NULL");
    if (r.count == 0) continue;                              // skipped by the kernel
    WS_REQUIRE(r.out_off >= 0 && r.out_off <= n_out - r.count, "%s: row %d: out [%lld, %lld + %lld) leaves the arena of %lld floats", who, i,
               r.out_off, r.out_off, r.count, n_out);
    // the windows the range reads, [w_min, w_max], must all be in the ring still: the newest `cap` windows are
    const long long w_min = r.i0 < L ? 0 : (r.i0 - L) / H + 1;
    long long w_max = std::min(Wk - 2, (end - 1) / H);
    if (r.final && end - 1 >= last) w_max = Wk - 1;
    WS_REQUIRE(w_min + cap >= r.windows_run && w_max - w_min < cap,
               "%s: row %d: cap=%d slots do not hold windows %lld..%lld of the range [%lld, %lld) with %lld windows run", who, i, cap, w_min,
               w_max, r.i0, end, r.windows_run);
    spans.push_back(lf_span(ring, r.ring_off, (long long)cap * S, i, false, "ring"));
    if (r.scale_off >= 0) spans.push_back(lf_span(scale_ring, r.scale_off, cap, i, false, "scale_ring"));
    spans.push_back(lf_span(out, r.out_off, r.count, i, true, "out"));
    nb_max = std::max(nb_max, (r.count + 255) / 256);
  }
  const int rc = lf_spans_disjoint(who, spans);
  if (rc != WS_OK) return rc;
  if (nb_max == 0) return WS_OK;                             // every row has count == 0
  hipLaunchKernelGGL(xfade_stream_rows_kernel, dim3((unsigned)nb_max, (unsigned)A), dim3(256), 0, (hipStream_t)stream, d_rows, S, O, cap,
                     ring, scale_ring, out);
  return ws_check_launch(who);
}

extern "C" int ws_tail_emit_rows_fwd(const ws_tail_emit_row* rows, const ws_tail_emit_row* d_rows, int A, int C, const float* ramp,
                                     const float* y, long long n_y, float* hold, long long n_hold, float* out, long long n_out,
                                     void* stream) {
  const char* who = "ws_tail_emit_rows_fwd";
  WS_REQUIRE(rows && d_rows && y && hold && out, "%s: rows, d_rows, y, hold or out is NULL", who);
  WS_REQUIRE(A > 0 && A <= 65535, "%s: A=%d is outside [1, 65535]", who, A);
  WS_REQUIRE(C >= 0, "%s: fade C=%d is negative", who, C);
  WS_REQUIRE(ramp || C == 0, "%s: ramp is NULL with fade C=%d (it may be NULL when C == 0 only)", who, C);
  WS_REQUIRE(n_y >= 0 && n_hold >= 0 && n_out >= 0, "%s: an arena length is negative (y %lld, hold %lld, out %lld)", who, n_y, n_hold,
             n_out);
  std::vector<LfSpan> spans;
  spans.reserve((size_t)A * 4);
  long long nb_max = 0;
  for (int i = 0; i < A; ++i) {
    const ws_tail_emit_row& r = rows[i];
    WS_REQUIRE(r.h == 0 || r.h == C, "%s: row %d: h=%d held samples, the fade takes 0 or C=%d", who, i, r.h, C);
    WS_REQUIRE(r.c_new == 0 || r.c_new == C, "%s: row %d: c_new=%d samples for the new hold, 0 or C=%d", who, i, r.c_new, C);
    WS_REQUIRE(r.m >= 0 && r.h <= r.m, "%s: row %d: h=%d held samples do not fit the m=%d emitted ones", who, i, r.h, r.m);
    WS_REQUIRE(r.p >= 0, "%s: row %d: p=%d is negative", who, i, r.p);
    WS_REQUIRE((long long)r.m + r.c_new >= 1, "%s: row %d: nothing to do (m=%d, c_new=%d)", who, i, r.m, r.c_new);
    WS_REQUIRE((long long)r.p + r.m + r.c_new == r.L, "%s: row %d: p + m + c_new = %d + %d + %d is not the window's L=%d", who, i, r.p,
               r.m, r.c_new, r.L);
    WS_REQUIRE((long long)r.L + 4096 < (1LL << 31), "%s: row %d: L=%d is not below 2^31 - 4096", who, i, r.L);
    WS_REQUIRE(r.y_off >= 0 && r.y_off <= n_y - r.L, "%s: row %d: y [%lld, %lld + %d) leaves the arena of %lld floats", who, i, r.y_off,
               r.y_off, r.L, n_y);
    WS_REQUIRE(r.h == 0 || (r.hold_in_off >= 0 && r.hold_in_off <= n_hold - r.h),
               "%s: row %d: hold_in [%lld, %lld + %d) leaves the arena of %lld floats", who, i, r.hold_in_off, r.hold_in_off, r.h, n_hold);
    WS_REQUIRE(r.c_new == 0 || (r.hold_out_off >= 0 && r.hold_out_off <= n_hold - r.c_new),
               "%s: row %d: hold_out [%lld, %lld + %d) leaves the arena of %lld floats", who, i, r.hold_out_off, r.hold_out_off, r.c_new,
               n_hold);
    WS_REQUIRE(r.m == 0 || (r.out_off >= 0 && r.out_off <= n_out - r.m), "%s: row %d: out [%lld, %lld + %d) leaves the arena of %lld floats",
               who, i, r.out_off, r.out_off, r.m, n_out);
    spans.push_back(lf_span(y, r.y_off, r.L, i, false, "y"));
    if (r.h > 0) spans.push_back(lf_span(hold, r.hold_in_off, r.h, i, false, "hold_in"));
    if (r.c_new > 0) spans.push_back(lf_span(hold, r.hold_out_off, r.c_new, i, true, "hold_out"));
    if (r.m > 0) spans.push_back(lf_span(out, r.out_off, r.m, i, true, "out"));
    // the quads of the row, counted as the kernel counts them (an empty destination is never addressed)
    const long long nq = (long long)tail_quads(r.m, r.m > 0 ? tail_shift(out + r.out_off) : 0) +
                         tail_quads(r.c_new, r.c_new > 0 ? tail_shift(hold + r.hold_out_off) : 0);
    nb_max = std::max(nb_max, (nq + 255) / 256);
  }
  const int rc = lf_spans_disjoint(who, spans);
  if (rc != WS_OK) return rc;
  hipLaunchKernelGGL(tail_emit_rows_kernel, dim3((unsigned)nb_max, (unsigned)A), dim3(256), 0, (hipStream_t)stream, d_rows, ramp, y, hold,
                     hold, out);
  return ws_check_launch(who);
}

extern "C" int ws_window_rows(const float* x, int n, int W, int S, int H, int reps, const float* scale, float* rows,
                              void* stream) {
  WS_REQUIRE(x && rows, "ws_window_rows: x or rows is NULL");
  WS_REQUIRE(n > 0 && S > 0 && reps > 0, "ws_window_rows: bad args (n=%d, S=%d, reps=%d)", n, S, reps);
  WS_REQUIRE(H > 0 && H <= S && S - H <= S / 2, "ws_window_rows: hop H=%d needs an overlap S - H in [0, S / 2] (S=%d)", H, S);
  WS_REQUIRE(W == lf_windows(n, S, H), "ws_window_rows: W=%d does not match (n=%d, S=%d, H=%d): %lld windows", W, n, S, H,
             lf_windows(n, S, H));
  const int L = n < S ? n : S;
  hipLaunchKernelGGL(window_rows_kernel, dim3(lf_blocks((long long)W * ((L + 3) / 4))), dim3(256), 0, (hipStream_t)stream,
                     x, (long long)n, W, L, H, reps, scale, rows);
  return ws_check_launch("ws_window_rows");
}

extern "C" int ws_xfade_ola(const float* y, int K, int W, int S, int O, int n, const float* scale, float* out,
                            void* stream) {
  WS_REQUIRE(y && out, "ws_xfade_ola: y or out is NULL");
  WS_REQUIRE(n > 0 && S > 0 && K > 0, "ws_xfade_ola: bad args (n=%d, S=%d, K=%d)", n, S, K);
  WS_REQUIRE(O >= 0 && O <= S / 2, "ws_xfade_ola: overlap O=%d outside [0, S / 2] (S=%d)", O, S);
  WS_REQUIRE(W == lf_windows(n, S, S - O), "ws_xfade_ola: W=%d does not match (n=%d, S=%d, O=%d): %lld windows", W, n, S, O,
             lf_windows(n, S, S - O));
  const int L = n < S ? n : S;
  hipLaunchKernelGGL(xfade_ola_kernel, dim3(lf_blocks((long long)K * n)), dim3(256), 0, (hipStream_t)stream, y, K, W, L,
                     S - O, O, (long long)n, scale, out);
  return ws_check_launch("ws_xfade_ola");
}

extern "C" int ws_xfade_stream_fwd(const float* ring, int K, int cap, int S, int O, const float* scale_ring, long long i0,
                                   long long count, long long windows_run, int final, long long W, long long n, float* out,
                                   long long ld_out, void* stream) {
  WS_REQUIRE(ring && out, "ws_xfade_stream_fwd: ring or out is NULL");
  WS_REQUIRE(S > 0 && K > 0 && cap > 0, "ws_xfade_stream_fwd: bad args (S=%d, K=%d, cap=%d)", S, K, cap);
  WS_REQUIRE(O >= 0 && O <= S / 2, "ws_xfade_stream_fwd: overlap O=%d outside [0, S / 2] (S=%d)", O, S);
  WS_REQUIRE(i0 >= 0 && count >= 0 && windows_run >= 0 && ld_out >= count,
             "ws_xfade_stream_fwd: bad range (i0=%lld, count=%lld, windows_run=%lld, ld_out=%lld)", i0, count, windows_run, ld_out);
  const long long H = S - O, end = i0 + count;
  long long Wk, last;                                      // what the kernel takes as the layout
  int L = S;
  if (final) {
    WS_REQUIRE(n > 0 && W == lf_windows(n, S, H) && windows_run == W,
               "ws_xfade_stream_fwd: a final range needs all W=%lld windows of (n=%lld, S=%d, O=%d) run: %lld windows, %lld run", W, n,
               S, O, n > 0 ? lf_windows(n, S, H) : 0LL, windows_run);
    WS_REQUIRE(end <= n, "ws_xfade_stream_fwd: the range [%lld, %lld) reaches past the recording's n=%lld samples", i0, end, n);
    if (n < S) L = (int)n;
    Wk = W, last = n - L;
  } else {
    const long long emitted = windows_run > 0 ? (windows_run - 1) * H : 0;
    WS_REQUIRE(end <= emitted, "ws_xfade_stream_fwd: the range [%lld, %lld) reaches past the %lld samples that the %lld windows "
               "run make final (pass the final layout at a flush)", i0, end, emitted, windows_run);
    Wk = windows_run + 1, last = 0x7fffffffffffffffLL;
  }
  if (count == 0) return WS_OK;
  // the windows the range reads, [w_min, w_max], must all be in the ring still: the newest `cap` windows are
  const long long w_min = i0 < L ? 0 : (i0 - L) / H + 1;
  long long w_max = std::min(Wk - 2, (end - 1) / H);
  if (final && end - 1 >= last) w_max = Wk - 1;
  WS_REQUIRE(w_min + cap >= windows_run && w_max - w_min < cap,
             "ws_xfade_stream_fwd: cap=%d slots do not hold windows %lld..%lld of the range [%lld, %lld) with %lld windows run", cap,
             w_min, w_max, i0, end, windows_run);
  hipLaunchKernelGGL(xfade_stream_kernel, dim3(lf_blocks((long long)K * count)), dim3(256), 0, (hipStream_t)stream, ring, K, cap,
                     S, L, (int)H, O, Wk, last, i0, count, scale_ring, out, ld_out);
  return ws_check_launch("ws_xfade_stream_fwd");
}
