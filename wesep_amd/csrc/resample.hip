// Sample-rate conversion (include/wesep_hip.h "sample rates"): a polyphase windowed-sinc filter, the
// published sinc_interp_hann design with lowpass_filter_width 6 and rolloff 0.99.  For rate_in -> rate_out, g = gcd,
// D = rate_in / g, U = rate_out / g, base = min(D, U) * 0.99, w = ceil(6 D / base), K = 2 w + D, and
//   y[q] = sum_{k < K} taps[q % U][k] * x[(q / U) * D + k - w],   x = 0 outside [0, n_in).
// The table is made in double and rounded to float once, on the host, by ws_resample_taps: the one place it is made.
//
// One device function, resample_one, computes one output sample: one accumulator started at 0, advanced by fmaf over the
// taps that fall on valid samples, in ascending k.  A tap before the first or behind the last valid sample is not part of
// the loop (no multiplication by a zero, nothing is read there).  Both entry points -- the whole signal, and a buffer of
// `history | new samples` of a stream -- run it, with buffer-relative int offsets only, so an output sample has the same
// bits in either form, under any chunking, alone or beside other rows, and from run to run.  No atomics; one thread owns one
// output sample of one row; rows have any pitch (scalar loads; consecutive lanes read addresses D floats apart).
//
// Taps: a table of at most RS_LDS_TAPS floats (8k <-> 16k, 48k <-> 16k: under 200) is staged in LDS once per workgroup --
// a wave's lanes then read at most U distinct addresses per k, served as LDS broadcasts.  A larger one (44.1k and
// 22.05k against 16k: 300 - 575 KB) does not fit and stays in global memory: lane q walks row q % U of the table
// front to back, so every 64-byte line it fetches serves its next 16 taps from the vector cache, and the table is shared by
// all workgroups through L2.  The two paths read the same floats in the same order.  Plain C++, no packed FP32.
//
// Rows forms (below the solo launch): ws_resample_stream_rows_fwd runs A rows, each with its own geometry, table, buffer,
// position and destinations, through the same resample_one in one launch; ws_rows_copy_fwd is table-driven data movement.
// ws_window_resample_rows_fwd is the gather of a rate tail pool: row i is L consecutive outputs of the whole-signal filter that
// start at ANY phase of a group (a trailing window does not start on a group boundary), computed from the input span that
// their taps cover and written to a destination of its own, `fill` zeros behind them.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "common.h"

namespace {

constexpr int RS_LDS_TAPS = 2048;   // floats of LDS a staged table may take (8 KB)
constexpr int RS_MAX_UD = WS_RESAMPLE_MAX_UD;
constexpr int RS_MAX_K = WS_RESAMPLE_MAX_K;

struct RsGeom {
  int U, D, w, K;
};

long long rs_gcd(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b, b = t;
  }
  return a;
}

// WS_OK or WS_ERR_INVALID with the text set
int rs_geom(const char* who, int rate_in, int rate_out, RsGeom* g) {
  WS_REQUIRE(rate_in > 0 && rate_out > 0, "%s: rate_in=%d and rate_out=%d must be positive", who, rate_in, rate_out);
  const long long c = rs_gcd(rate_in, rate_out);
  const long long D = rate_in / c, U = rate_out / c;
  WS_REQUIRE(U <= RS_MAX_UD && D <= RS_MAX_UD, "%s: %d -> %d reduces to U=%lld, D=%lld; U and D may not exceed %d", who, rate_in,
             rate_out, U, D, RS_MAX_UD);
  const double base = (double)(D < U ? D : U) * 0.99;
  const long long w = (long long)ceil(6.0 * (double)D / base);
  const long long K = 2 * w + D;
  WS_REQUIRE(K <= RS_MAX_K, "%s: %d -> %d needs K=%lld taps per output sample; K may not exceed %d", who, rate_in, rate_out, K,
             RS_MAX_K);
  g->U = (int)U, g->D = (int)D, g->w = (int)w, g->K = (int)K;
  return WS_OK;
}

// output q of the buffer's numbering: group q / U, phase q % U; the group's first tap sits at buffer index
// (q / U) * D - lead.  Valid samples are buf[0, n_valid).
__device__ __forceinline__ float resample_one(const float* __restrict__ buf, const float* __restrict__ tp, int D, int K, int lead,
                                              int n_valid, int grp) {
  const int j0 = grp * D - lead;
  const int k_lo = j0 < 0 ? -j0 : 0;
  const int k_hi = min(K, n_valid - j0);
  float acc = 0.f;
  for (int k = k_lo; k < k_hi; ++k) acc = fmaf(tp[k], buf[j0 + k], acc);
  return acc;
}

// grid (nb_out + nb_hist, R): the first nb_out workgroups of a row own 256 output samples each; the others copy the
// samples [hist_from, hist_from + hist_len) of the buffer to `hist` (another buffer: the stream's next history).
template <bool LDS>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ buf, long long ldb, const float* __restrict__ taps,
                                                       int U, int D, int K, int lead, int n_valid, int q_first, int n_out,
                                                       float* __restrict__ y, long long ldy, int nb_out, int hist_from,
                                                       int hist_len, float* __restrict__ hist, long long ldh) {
  extern __shared__ float s_taps[];
  const int r = blockIdx.y;
  const float* row = buf + (long long)r * ldb;
  if ((int)blockIdx.x >= nb_out) {
    const int i = ((int)blockIdx.x - nb_out) * 256 + (int)threadIdx.x;
    if (i < hist_len) hist[(long long)r * ldh + i] = row[hist_from + i];
    return;
  }
  if (LDS) {
    for (int i = threadIdx.x; i < U * K; i += 256) s_taps[i] = taps[i];
    __syncthreads();
  }
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n_out) return;
  const int q = q_first + i;
  const int grp = q / U, p = q - grp * U;
  const float* tp = (LDS ? s_taps : taps) + p * K;
  y[(long long)r * ldy + i] = resample_one(row, tp, D, K, lead, n_valid, grp);
}

int rs_launch(const char* who, const float* buf, long long ldb, int R, const RsGeom& g, const float* taps, int lead, int n_valid,
              int q_first, int n_out, float* y, long long ldy, int hist_from, int hist_len, float* hist, long long ldh,
              void* stream) {
  const int nb_out = (n_out + 255) / 256, nb_hist = (hist_len + 255) / 256;
  const dim3 grid((unsigned)(nb_out + nb_hist), (unsigned)R);
  if (g.U * g.K <= RS_LDS_TAPS)
    hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(256), (size_t)g.U * g.K * sizeof(float), (hipStream_t)stream, buf, ldb, taps,
                       g.U, g.D, g.K, lead, n_valid, q_first, n_out, y, ldy, nb_out, hist_from, hist_len, hist, ldh);
  else
    hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, buf, ldb, taps, g.U, g.D, g.K, lead,
                       n_valid, q_first, n_out, y, ldy, nb_out, hist_from, hist_len, hist, ldh);
  return ws_check_launch(who);
}

// ---- rows forms: one launch for A rows, each with its own geometry, table, buffer, position and destinations -----------
// grid (max_i(nb_out_i + nb_hist_i), A): workgroup (b, i) reads row i's descriptor (the same address in every lane) and
// leaves before any barrier when b is beyond the row's own count -- blockIdx and the descriptor only, so the exit, the
// history / output split and the choice of tap staging are workgroup-uniform.  Outputs run resample_one as above.
__global__ __launch_bounds__(256) void resample_rows_kernel(const ws_resample_row* __restrict__ rows, const float* __restrict__ buf,
                                                            const float* __restrict__ taps, float* __restrict__ y,
                                                            float* __restrict__ hist) {
  extern __shared__ float s_taps[];
  const ws_resample_row r = rows[blockIdx.y];
  const int nb_out = (r.n_out + 255) / 256, nb_hist = (r.hist_len + 255) / 256;
  const int b = (int)blockIdx.x;
  if (b >= nb_out + nb_hist) return;
  const float* row = buf + r.in_off;
  if (b >= nb_out) {
    const int i = (b - nb_out) * 256 + (int)threadIdx.x;
    if (i < r.hist_len) hist[r.hist_off + i] = row[r.hist_from + i];
    return;
  }
  const float* tg = taps + r.taps_off;
  const bool lds = r.U * r.K <= RS_LDS_TAPS;
  if (lds) {
    for (int i = threadIdx.x; i < r.U * r.K; i += 256) s_taps[i] = tg[i];
    __syncthreads();
  }
  const int i = b * 256 + (int)threadIdx.x;
  if (i >= r.n_out) return;
  const int q = r.g_first * r.U + i;
  const int grp = q / r.U, p = q - grp * r.U;
  if (lds)
    y[r.out_off + i] = resample_one(row, s_taps + p * r.K, r.D, r.K, r.lead, r.n_valid, grp);
  else
    y[r.out_off + i] = resample_one(row, tg + p * r.K, r.D, r.K, r.lead, r.n_valid, grp);
}

// grid (max_i blocks of L_i + fill_i, A): workgroup (b, i) owns 256 consecutive floats of row i's destination -- outputs first,
// zeros behind them -- and leaves before any barrier when b is beyond the row's count.  A workgroup that lies wholly in the
// zeros stages no table.  Everything that decides these is blockIdx and the descriptor: workgroup-uniform.
__global__ __launch_bounds__(256) void window_resample_rows_kernel(const ws_window_resample_row* __restrict__ rows,
                                                                   const float* __restrict__ buf, const float* __restrict__ taps,
                                                                   float* __restrict__ y) {
  extern __shared__ float s_taps[];
  const ws_window_resample_row r = rows[blockIdx.y];
  const int n = r.L + r.fill;
  const int i0 = (int)blockIdx.x * 256;
  if (i0 >= n) return;
  const float* tg = taps + r.taps_off;
  const bool lds = r.U * r.K <= RS_LDS_TAPS;
  if (lds && i0 < r.L) {
    for (int i = threadIdx.x; i < r.U * r.K; i += 256) s_taps[i] = tg[i];
    __syncthreads();
  }
  const int i = i0 + (int)threadIdx.x;
  if (i >= n) return;
  if (i >= r.L) {
    y[r.out_off + i] = 0.f;
    return;
  }
  const int q = r.g_first * r.U + r.p_first + i;
  const int grp = q / r.U, p = q - grp * r.U;
  const float* row = buf + r.in_off;
  if (lds)
    y[r.out_off + i] = resample_one(row, s_taps + p * r.K, r.D, r.K, r.lead, r.n_valid, grp);
  else
    y[r.out_off + i] = resample_one(row, tg + p * r.K, r.D, r.K, r.lead, r.n_valid, grp);
}

// grid (max_i nb_i, A): row i copies len floats and writes fill zeros behind them
__global__ __launch_bounds__(256) void rows_copy_kernel(const ws_rows_copy_row* __restrict__ rows, const float* __restrict__ src,
                                                        float* __restrict__ dst) {
  const ws_rows_copy_row r = rows[blockIdx.y];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < r.len)
    dst[r.dst_off + i] = src[r.src_off + i];
  else if (i < (long long)r.len + r.fill)
    dst[r.dst_off + i] = 0.f;
}

// Address ranges of one rows call: a written range may meet no other range of the call, read or written (another
// workgroup of the launch owns it).  Ranges that are only read may share.
struct RsSpan {
  uintptr_t lo, hi;
  int row;
  bool write;
  const char* name;
};

int rs_spans_disjoint(const char* who, std::vector<RsSpan>& v) {
  std::sort(v.begin(), v.end(), [](const RsSpan& a, const RsSpan& b) { return a.lo < b.lo; });
  const RsSpan *far_r = nullptr, *far_w = nullptr;      // the read / written range that ends last so far
  for (const RsSpan& x : v) {
    const RsSpan* hit = far_w && x.lo < far_w->hi ? far_w : (x.write && far_r && x.lo < far_r->hi ? far_r : nullptr);
    WS_REQUIRE(!hit, "%s: row %d: its %s range overlaps the %s range of row %d", who, x.row, x.name, hit->name, hit->row);
    const RsSpan*& far = x.write ? far_w : far_r;
    if (!far || x.hi > far->hi) far = &x;
  }
  return WS_OK;
}

}  // namespace

extern "C" int ws_resample_stream_rows_fwd(const ws_resample_row* rows, const ws_resample_row* d_rows, int A, const float* buf,
                                           long long n_buf, const float* taps, long long n_taps, float* y, long long n_y,
                                           float* hist, long long n_hist, void* stream) {
  const char* who = "ws_resample_stream_rows_fwd";
  WS_REQUIRE(rows && d_rows && buf && taps, "%s: rows, d_rows, buf or taps is NULL", who);
  WS_REQUIRE(A > 0 && A <= 65535, "%s: A=%d is outside [1, 65535]", who, A);
  WS_REQUIRE(n_buf >= 0 && n_taps >= 0 && n_y >= 0 && n_hist >= 0, "%s: an arena length is negative (buf %lld, taps %lld, y %lld, hist %lld)",
             who, n_buf, n_taps, n_y, n_hist);
  std::vector<RsSpan> spans;
  spans.reserve((size_t)A * 4);
  int nb_max = 0;
  bool any_lds = false;
  for (int i = 0; i < A; ++i) {
    const ws_resample_row& r = rows[i];
    WS_REQUIRE(r.U >= 1 && r.D >= 1 && r.U <= RS_MAX_UD && r.D <= RS_MAX_UD, "%s: row %d: U=%d, D=%d; U and D lie in [1, %d]", who, i, r.U, r.D,
               RS_MAX_UD);
    WS_REQUIRE(r.K >= 1 && r.K <= RS_MAX_K, "%s: row %d: K=%d taps per output sample; K lies in [1, %d]", who, i, r.K, RS_MAX_K);
    WS_REQUIRE(r.K >= r.D, "%s: row %d: K=%d is below D=%d", who, i, r.K, r.D);
    WS_REQUIRE((r.K - r.D) % 2 == 0, "%s: row %d: K - D = %d is odd (K = 2 w + D)", who, i, r.K - r.D);
    const int w = (r.K - r.D) / 2;
    WS_REQUIRE(y || r.n_out == 0, "%s: row %d: y is NULL with n_out=%d", who, i, r.n_out);
    WS_REQUIRE(hist || r.hist_len == 0, "%s: row %d: hist is NULL with hist_len=%d", who, i, r.hist_len);
    WS_REQUIRE(r.n_valid > 0 && r.n_out >= 0 && r.hist_len >= 0 && r.n_out + (long long)r.hist_len > 0,
               "%s: row %d: bad sizes (n_valid=%d >= 1, n_out=%d, hist_len=%d, one of them positive)", who, i, r.n_valid, r.n_out, r.hist_len);
    WS_REQUIRE(r.lead >= 0 && r.lead <= w && r.g_first >= 0, "%s: row %d: lead=%d outside [0, w=%d] or g_first=%d negative", who, i, r.lead, w,
               r.g_first);
    WS_REQUIRE(r.in_off >= 0 && r.in_off <= n_buf - r.n_valid, "%s: row %d: buf [%lld, %lld + %d) leaves the arena of %lld floats", who, i,
               r.in_off, r.in_off, r.n_valid, n_buf);
    WS_REQUIRE(r.taps_off >= 0 && r.taps_off <= n_taps - (long long)r.U * r.K, "%s: row %d: taps [%lld, %lld + %d * %d) leaves the arena of %lld floats",
               who, i, r.taps_off, r.taps_off, r.U, r.K, n_taps);
    WS_REQUIRE(r.n_out == 0 || (r.out_off >= 0 && r.out_off <= n_y - r.n_out), "%s: row %d: y [%lld, %lld + %d) leaves the arena of %lld floats", who,
               i, r.out_off, r.out_off, r.n_out, n_y);
    WS_REQUIRE(r.hist_len == 0 || (r.hist_off >= 0 && r.hist_off <= n_hist - r.hist_len),
               "%s: row %d: hist [%lld, %lld + %d) leaves the arena of %lld floats", who, i, r.hist_off, r.hist_off, r.hist_len, n_hist);
    WS_REQUIRE(r.hist_from >= 0 && (long long)r.hist_from + r.hist_len <= r.n_valid, "%s: row %d: history [%d, %d + %d) leaves the %d valid samples",
               who, i, r.hist_from, r.hist_from, r.hist_len, r.n_valid);
    const long long q_end = (long long)r.g_first * r.U + r.n_out;
    WS_REQUIRE(q_end + r.U + 256 < (1LL << 31) && (q_end / r.U + 2) * r.D + r.K < (1LL << 31) && (long long)r.n_valid + r.K + 256 < (1LL << 31),
               "%s: row %d: offsets reach 2^31 (g_first=%d, n_out=%d, n_valid=%d)", who, i, r.g_first, r.n_out, r.n_valid);
    if (r.n_out > 0) {
      if (r.final) {
        const long long span = (long long)r.n_valid + r.lead - w;
        const long long allowed = span > 0 ? ((long long)r.U * span + r.D - 1) / r.D : 0;
        WS_REQUIRE(q_end <= allowed, "%s: row %d: outputs up to %lld asked, the %d valid samples end the signal at output %lld", who, i, q_end,
                   r.n_valid, allowed);
      } else {
        const long long last_grp = (q_end - 1) / r.U;
        WS_REQUIRE(last_grp * r.D - r.lead + r.K <= r.n_valid,
                   "%s: row %d: outputs up to %lld need %lld valid samples, %d are given and the end is not final", who, i, q_end,
                   last_grp * r.D - r.lead + r.K, r.n_valid);
      }
    }
    const auto span = [i](const float* p, long long off, long long n, bool wr, const char* name) {
      return RsSpan{reinterpret_cast<uintptr_t>(p + off), reinterpret_cast<uintptr_t>(p + off + n), i, wr, name};
    };
    spans.push_back(span(buf, r.in_off, r.n_valid, false, "buf"));
    spans.push_back(span(taps, r.taps_off, (long long)r.U * r.K, false, "taps"));
    if (r.n_out > 0) spans.push_back(span(y, r.out_off, r.n_out, true, "y"));
    if (r.hist_len > 0) spans.push_back(span(hist, r.hist_off, r.hist_len, true, "hist"));
    nb_max = std::max(nb_max, (r.n_out + 255) / 256 + (r.hist_len + 255) / 256);
    any_lds = any_lds || r.U * r.K <= RS_LDS_TAPS;
  }
  const int rc = rs_spans_disjoint(who, spans);
  if (rc != WS_OK) return rc;
  hipLaunchKernelGGL(resample_rows_kernel, dim3((unsigned)nb_max, (unsigned)A), dim3(256), any_lds ? RS_LDS_TAPS * sizeof(float) : 0,
                     (hipStream_t)stream, d_rows, buf, taps, y, hist);
  return ws_check_launch(who);
}

extern "C" int ws_window_resample_rows_fwd(const ws_window_resample_row* rows, const ws_window_resample_row* d_rows, int A,
                                           const float* buf, long long n_buf, const float* taps, long long n_taps, float* y,
                                           long long n_y, void* stream) {
  const char* who = "ws_window_resample_rows_fwd";
  WS_REQUIRE(rows && d_rows && buf && taps && y, "%s: rows, d_rows, buf, taps or y is NULL", who);
  WS_REQUIRE(A > 0 && A <= 65535, "%s: A=%d is outside [1, 65535]", who, A);
  WS_REQUIRE(n_buf >= 0 && n_taps >= 0 && n_y >= 0, "%s: an arena length is negative (buf %lld, taps %lld, y %lld)", who, n_buf, n_taps, n_y);
  std::vector<RsSpan> spans;
  spans.reserve((size_t)A * 3);
  long long nb_max = 0;
  bool any_lds = false;
  for (int i = 0; i < A; ++i) {
    const ws_window_resample_row& r = rows[i];
    WS_REQUIRE(r.U >= 1 && r.D >= 1 && r.U <= RS_MAX_UD && r.D <= RS_MAX_UD, "%s: row %d: U=%d, D=%d; U and D lie in [1, %d]", who, i, r.U, r.D,
               RS_MAX_UD);
    WS_REQUIRE(r.K >= 1 && r.K <= RS_MAX_K, "%s: row %d: K=%d taps per output sample; K lies in [1, %d]", who, i, r.K, RS_MAX_K);
    WS_REQUIRE(r.K >= r.D, "%s: row %d: K=%d is below D=%d", who, i, r.K, r.D);
    WS_REQUIRE((r.K - r.D) % 2 == 0, "%s: row %d: K - D = %d is odd (K = 2 w + D)", who, i, r.K - r.D);
    const int w = (r.K - r.D) / 2;
    WS_REQUIRE(r.n_valid > 0 && r.L >= 0 && r.fill >= 0 && r.L + (long long)r.fill > 0,
               "%s: row %d: bad sizes (n_valid=%d >= 1, L=%d, fill=%d, one of them positive)", who, i, r.n_valid, r.L, r.fill);
    WS_REQUIRE(r.lead >= 0 && r.lead <= w && r.g_first >= 0, "%s: row %d: lead=%d outside [0, w=%d] or g_first=%d negative", who, i, r.lead, w,
               r.g_first);
    WS_REQUIRE(r.p_first >= 0 && r.p_first < r.U, "%s: row %d: p_first=%d is outside [0, U=%d)", who, i, r.p_first, r.U);
    WS_REQUIRE(r.in_off >= 0 && r.in_off <= n_buf - r.n_valid, "%s: row %d: buf [%lld, %lld + %d) leaves the arena of %lld floats", who, i,
               r.in_off, r.in_off, r.n_valid, n_buf);
    WS_REQUIRE(r.taps_off >= 0 && r.taps_off <= n_taps - (long long)r.U * r.K, "%s: row %d: taps [%lld, %lld + %d * %d) leaves the arena of %lld floats",
               who, i, r.taps_off, r.taps_off, r.U, r.K, n_taps);
    const long long n_dst = (long long)r.L + r.fill;
    WS_REQUIRE(r.out_off >= 0 && r.out_off <= n_y - n_dst, "%s: row %d: y [%lld, %lld + %d + %d) leaves the arena of %lld floats", who, i, r.out_off,
               r.out_off, r.L, r.fill, n_y);
    const long long q_end = (long long)r.g_first * r.U + r.p_first + r.L;
    WS_REQUIRE(q_end + r.U + 256 < (1LL << 31) && (q_end / r.U + 2) * r.D + r.K < (1LL << 31) && (long long)r.n_valid + r.K + 256 < (1LL << 31) &&
                   n_dst + 256 < (1LL << 31),
               "%s: row %d: offsets reach 2^31 (g_first=%d, p_first=%d, L=%d, fill=%d, n_valid=%d)", who, i, r.g_first, r.p_first, r.L, r.fill,
               r.n_valid);
    if (r.L > 0) {
      if (r.final) {
        const long long span = (long long)r.n_valid + r.lead - w;
        const long long allowed = span > 0 ? ((long long)r.U * span + r.D - 1) / r.D : 0;
        WS_REQUIRE(q_end <= allowed, "%s: row %d: outputs up to %lld asked, the %d valid samples end the signal at output %lld", who, i, q_end,
                   r.n_valid, allowed);
      } else {
        const long long last_grp = (q_end - 1) / r.U;
        WS_REQUIRE(last_grp * r.D - r.lead + r.K <= r.n_valid,
                   "%s: row %d: outputs up to %lld need %lld valid samples, %d are given and the end is not final", who, i, q_end,
                   last_grp * r.D - r.lead + r.K, r.n_valid);
      }
    }
    const auto span = [i](const float* p, long long off, long long n, bool wr, const char* name) {
      return RsSpan{reinterpret_cast<uintptr_t>(p + off), reinterpret_cast<uintptr_t>(p + off + n), i, wr, name};
    };
    spans.push_back(span(buf, r.in_off, r.n_valid, false, "buf"));
    spans.push_back(span(taps, r.taps_off, (long long)r.U * r.K, false, "taps"));
    spans.push_back(span(y, r.out_off, n_dst, true, "y"));
    nb_max = std::max(nb_max, (n_dst + 255) / 256);
    any_lds = any_lds || r.U * r.K <= RS_LDS_TAPS;
  }
  const int rc = rs_spans_disjoint(who, spans);
  if (rc != WS_OK) return rc;
  hipLaunchKernelGGL(window_resample_rows_kernel, dim3((unsigned)nb_max, (unsigned)A), dim3(256), any_lds ? RS_LDS_TAPS * sizeof(float) : 0,
                     (hipStream_t)stream, d_rows, buf, taps, y);
  return ws_check_launch(who);
}

extern "C" int ws_rows_copy_fwd(const ws_rows_copy_row* rows, const ws_rows_copy_row* d_rows, int A, const float* src, long long n_src,
                                float* dst, long long n_dst, void* stream) {
  const char* who = "ws_rows_copy_fwd";
  WS_REQUIRE(rows && d_rows && src && dst, "%s: rows, d_rows, src or dst is NULL", who);
  WS_REQUIRE(A > 0 && A <= 65535, "%s: A=%d is outside [1, 65535]", who, A);
  WS_REQUIRE(n_src >= 0 && n_dst >= 0, "%s: an arena length is negative (src %lld, dst %lld)", who, n_src, n_dst);
  std::vector<RsSpan> spans;
  spans.reserve((size_t)A * 2);
  long long nb_max = 0;
  for (int i = 0; i < A; ++i) {
    const ws_rows_copy_row& r = rows[i];
    WS_REQUIRE(r.len >= 0 && r.fill >= 0 && (long long)r.len + r.fill > 0 && (long long)r.len + r.fill + 256 < (1LL << 31),
               "%s: row %d: bad sizes (len=%d >= 0, fill=%d >= 0, one of them positive, their sum below 2^31)", who, i, r.len, r.fill);
    WS_REQUIRE(r.len == 0 || (r.src_off >= 0 && r.src_off <= n_src - r.len), "%s: row %d: src [%lld, %lld + %d) leaves the arena of %lld floats", who,
               i, r.src_off, r.src_off, r.len, n_src);
    WS_REQUIRE(r.dst_off >= 0 && r.dst_off <= n_dst - ((long long)r.len + r.fill),
               "%s: row %d: dst [%lld, %lld + %d + %d) leaves the arena of %lld floats", who, i, r.dst_off, r.dst_off, r.len, r.fill, n_dst);
    if (r.len > 0)
      spans.push_back(RsSpan{reinterpret_cast<uintptr_t>(src + r.src_off), reinterpret_cast<uintptr_t>(src + r.src_off + r.len), i, false, "src"});
    spans.push_back(RsSpan{reinterpret_cast<uintptr_t>(dst + r.dst_off), reinterpret_cast<uintptr_t>(dst + r.dst_off + r.len + r.fill), i, true, "dst"});
    nb_max = std::max(nb_max, ((long long)r.len + r.fill + 255) / 256);
  }
  const int rc = rs_spans_disjoint(who, spans);
  if (rc != WS_OK) return rc;
  hipLaunchKernelGGL(rows_copy_kernel, dim3((unsigned)nb_max, (unsigned)A), dim3(256), 0, (hipStream_t)stream, d_rows, src, dst);
  return ws_check_launch(who);
}

extern "C" int ws_resample_geom(int rate_in, int rate_out, int* U, int* D, int* w, int* K) {
  WS_REQUIRE(U && D && w && K, "ws_resample_geom: U, D, w or K is NULL");
  RsGeom g;
  const int rc = rs_geom("ws_resample_geom", rate_in, rate_out, &g);
  if (rc != WS_OK) return rc;
  *U = g.U, *D = g.D, *w = g.w, *K = g.K;
  return WS_OK;
}

extern "C" int ws_resample_taps(int rate_in, int rate_out, float* taps) {
  WS_REQUIRE(taps, "ws_resample_taps: taps is NULL");
  RsGeom g;
  const int rc = rs_geom("ws_resample_taps", rate_in, rate_out, &g);
  if (rc != WS_OK) return rc;
  const double pi = 3.14159265358979323846;
  const double base = (double)(g.D < g.U ? g.D : g.U) * 0.99;
  for (int p = 0; p < g.U; ++p)
    for (int k = 0; k < g.K; ++k) {
      double t = (-(double)p / (double)g.U + (double)(k - g.w) / (double)g.D) * base;
      t = t < -6.0 ? -6.0 : (t > 6.0 ? 6.0 : t);
      const double sinc = t == 0.0 ? 1.0 : sin(pi * t) / (pi * t);
      const double c = cos(pi * t / 12.0);
      taps[(size_t)p * g.K + k] = (float)(sinc * (c * c) * base / (double)g.D);
    }
  return WS_OK;
}

extern "C" int ws_resample_fwd(const float* x, long long ldx, int R, int n_in, int rate_in, int rate_out, const float* taps,
                               float* y, long long ldy, void* stream) {
  WS_REQUIRE(x && taps && y, "ws_resample_fwd: x, taps or y is NULL");
  RsGeom g;
  const int rc = rs_geom("ws_resample_fwd", rate_in, rate_out, &g);
  if (rc != WS_OK) return rc;
  WS_REQUIRE(R > 0 && R <= 65535 && n_in > 0, "ws_resample_fwd: bad sizes (R=%d in [1, 65535], n_in=%d >= 1)", R, n_in);
  const long long n_out = ((long long)g.U * n_in + g.D - 1) / g.D;
  // (+ 256: the last workgroup's thread index, an int, stays below 2^31)
  WS_REQUIRE(n_out + g.U + 256 < (1LL << 31) && (long long)n_in + g.K + g.D < (1LL << 31),
             "ws_resample_fwd: n_in=%d or its %lld output samples reach 2^31", n_in, n_out);
  WS_REQUIRE(ldx >= n_in && ldy >= n_out, "ws_resample_fwd: row pitch ldx=%lld below n_in=%d or ldy=%lld below n_out=%lld", ldx, n_in,
             ldy, n_out);
  return rs_launch("ws_resample_fwd", x, ldx, R, g, taps, g.w, n_in, 0, (int)n_out, y, ldy, 0, 0, nullptr, 0, stream);
}

extern "C" int ws_resample_stream_fwd(const float* buf, long long ldb, int R, int rate_in, int rate_out, const float* taps,
                                      int lead, int n_valid, int final, int g_first, int n_out, float* y, long long ldy,
                                      int hist_from, int hist_len, float* hist, long long ldh, void* stream) {
  WS_REQUIRE(buf && taps, "ws_resample_stream_fwd: buf or taps is NULL");
  WS_REQUIRE(y || n_out == 0, "ws_resample_stream_fwd: y is NULL with n_out=%d", n_out);
  WS_REQUIRE(hist || hist_len == 0, "ws_resample_stream_fwd: hist is NULL with hist_len=%d", hist_len);
  RsGeom g;
  const int rc = rs_geom("ws_resample_stream_fwd", rate_in, rate_out, &g);
  if (rc != WS_OK) return rc;
  WS_REQUIRE(R > 0 && R <= 65535 && n_valid > 0 && n_out >= 0 && hist_len >= 0 && n_out + (long long)hist_len > 0,
             "ws_resample_stream_fwd: bad sizes (R=%d in [1, 65535], n_valid=%d >= 1, n_out=%d, hist_len=%d, one of them positive)", R,
             n_valid, n_out, hist_len);
  WS_REQUIRE(lead >= 0 && lead <= g.w && g_first >= 0, "ws_resample_stream_fwd: lead=%d outside [0, w=%d] or g_first=%d negative", lead,
             g.w, g_first);
  WS_REQUIRE(ldb >= n_valid && (n_out == 0 || ldy >= n_out) && (hist_len == 0 || ldh >= hist_len),
             "ws_resample_stream_fwd: a row pitch is below its row (ldb=%lld, n_valid=%d; ldy=%lld, n_out=%d; ldh=%lld, hist_len=%d)",
             ldb, n_valid, ldy, n_out, ldh, hist_len);
  WS_REQUIRE(hist_from >= 0 && (long long)hist_from + hist_len <= n_valid,
             "ws_resample_stream_fwd: history [%d, %d + %d) leaves the %d valid samples", hist_from, hist_from, hist_len, n_valid);
  WS_REQUIRE(hist_len == 0 || hist + (size_t)(R - 1) * ldh + hist_len <= buf || buf + (size_t)(R - 1) * ldb + n_valid <= hist,
             "ws_resample_stream_fwd: hist overlaps buf");
  const long long q_end = (long long)g_first * g.U + n_out;
  WS_REQUIRE(q_end + g.U + 256 < (1LL << 31) && (q_end / g.U + 2) * g.D + g.K < (1LL << 31) && (long long)n_valid + g.K + 256 < (1LL << 31),
             "ws_resample_stream_fwd: offsets reach 2^31 (g_first=%d, n_out=%d, n_valid=%d)", g_first, n_out, n_valid);
  if (n_out > 0) {
    if (final) {
      const long long span = (long long)n_valid + lead - g.w;      // samples from the first group's centre to the end
      const long long allowed = span > 0 ? ((long long)g.U * span + g.D - 1) / g.D : 0;
      WS_REQUIRE(q_end <= allowed, "ws_resample_stream_fwd: outputs up to %lld asked, the %d valid samples end the signal at output %lld",
                 q_end, n_valid, allowed);
    } else {
      const long long last_grp = (q_end - 1) / g.U;
      WS_REQUIRE(last_grp * g.D - lead + g.K <= n_valid,
                 "ws_resample_stream_fwd: outputs up to %lld need %lld valid samples, %d are given and the end is not final", q_end,
                 last_grp * g.D - lead + g.K, n_valid);
    }
  }
  return rs_launch("ws_resample_stream_fwd", buf, ldb, R, g, taps, lead, n_valid, g_first * g.U, n_out, y, ldy, hist_from, hist_len, hist,
                   ldh, stream);
}
