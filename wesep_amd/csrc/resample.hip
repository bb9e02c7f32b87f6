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

}  // namespace

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
