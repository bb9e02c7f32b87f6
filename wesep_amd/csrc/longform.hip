// Windowed separation of long recordings (runtime/longform.cc): one mixture of n samples is cut into W
// overlapping windows of S samples, the windows go through a separator as the rows of a rectangle, and the estimates are
// cross-faded back into one signal.  The layout is a pure function of (n, S, O), O the overlap, hop H = S - O:
//   n <= S:  one window [0, n) of L = n samples;
//   else:    W = 1 + ceil((n - S) / H) windows of L = S samples, start_w = min(w * H, n - S) -- the last window is aligned
//            to the end of the recording, so every window has full length (it may overlap its predecessor by up to S - 1
//            samples, and a third window with it).
// ws_xfade_stream_fwd is ws_xfade_ola over a range of absolute positions, its windows read from a ring: the live form
// (runtime/live.cc).  Both cross-fades inline ONE body, lf_blend, so their arithmetic cannot differ.
// The kernels compute the starts themselves; no table of them exists.  Two HBM-bound passes: ws_window_rows gathers the
// rows (once per target speaker), ws_xfade_ola blends the estimates with linear ramps over the O overlapping samples,
// normalised by the sum of the weights that cover a sample.  Offsets are 64-bit (n up to 2^31 - 1); sums run in ascending
// window order, no atomics; plain C++, no packed FP32.
#include <algorithm>

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

}  // namespace

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
