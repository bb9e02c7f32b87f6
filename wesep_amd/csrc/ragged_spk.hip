// Length-aware kernels of the ragged speaker stage: enrollments of different lengths share ONE encoder pass
// over the rectangle [R][...][Wmax][C].  The invariant every layer's input keeps: row r is exactly zero at time positions
// w >= W_r (its own valid width at that layer), so a convolution at w < W_r' reads what it would read on the row alone --
// the row's zero padding and the rectangle's zero tail are the same numbers.  BatchNorm shift, bias and residual make the
// tail non-zero again; the masked epilogue re-selects it to zero.  Only reductions over time take the length as an
// operand (TSTP, ASTP, the SE mean, CMN).
//
// Length tables are device int[R].  Every kernel clamps the entries it reads, so no entry moves an access out of its
// row.  "Zero" is always selected, never multiplied: NaN / Inf behind a row's end do not reach a valid output.
#include "common.h"

namespace {

inline int rg_blocks(long long n, int per = 256, int cap = 32768) {   // grid-stride kernels: the cap of tasnet.hip's ew_blocks
  long long b = (n + per - 1) / per;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

__device__ __forceinline__ int rg_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- masked BatchNorm epilogue --------------------------------------------------------------------------------------
// ws_bn_prelu_fwd (tasnet.hip) with a width table: row m belongs to r = m / rows_per_r and sits at w = m % W; rows with
// w >= wlen[r] are written as zeros (u and y), without reading x or res there.  The arithmetic of the other rows is
// the expression of bn_prelu_fwd_kernel, term for term, so they come out bit for bit.
__global__ void bn_prelu_fwd_len_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                        const float* __restrict__ res, const float* __restrict__ a, long long M, int C,
                                        int rows_per_r, int W, const int* __restrict__ wlen, float* __restrict__ u,
                                        float* __restrict__ y) {
  const float slope = a[0];
  const int c4n = C >> 2;
  const long long total = M * c4n;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long m = i / c4n;
    const int c = (int)(i - m * c4n) * 4;
    const int w = (int)(m % W);
    if (w >= rg_clamp(wlen[m / rows_per_r], 0, W)) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(u + i * 4) = z;
      *reinterpret_cast<f32x4*>(y + i * 4) = z;
      continue;
    }
    f32x4 v = (*reinterpret_cast<const f32x4*>(x + i * 4) - *reinterpret_cast<const f32x4*>(stats + c)) *
                  *reinterpret_cast<const f32x4*>(stats + C + c) * *reinterpret_cast<const f32x4*>(gamma + c) +
              *reinterpret_cast<const f32x4*>(beta + c);
    if (res) v += *reinterpret_cast<const f32x4*>(res + i * 4);
    *reinterpret_cast<f32x4*>(u + i * 4) = v;
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = v[j] > 0.f ? v[j] : slope * v[j];
    *reinterpret_cast<f32x4*>(y + i * 4) = o;
  }
}

// ---- TSTP over t < tlen[r]: the loops of tstp_fwd_kernel (conv2d.hip) with the row's own frame count -------------------
__global__ void tstp_fwd_len_kernel(const float* __restrict__ x, int R, int F, int T, int C, const int* __restrict__ tlen,
                                    float eps, float* __restrict__ stats) {
  const long long total = (long long)R * F * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long long q = i / C;
    const int f = (int)(q % F), r = (int)(q / F);
    const int tl = rg_clamp(tlen[r], 1, T);
    const float* b = x + (((long long)r * F + f) * T) * C + c;
    float s = 0.f;
    for (int t = 0; t < tl; ++t) s += b[(long long)t * C];
    const float mean = s / (float)tl;
    float m2 = 0.f;
    for (int t = 0; t < tl; ++t) {
      const float dv = b[(long long)t * C] - mean;
      m2 += dv * dv;
    }
    const float var = tl > 1 ? m2 / (float)(tl - 1) : 0.f;
    float* o = stats + (long long)r * 2 * C * F;
    o[c * F + f] = mean;
    o[C * F + c * F + f] = sqrtf(var + eps);
  }
}

// ---- ASTP with the softmax, mean and second moment over t < tlen[r] (astp_fwd_kernel, conv2d.hip) ---------------------
__global__ void astp_fwd_len_kernel(const float* __restrict__ x, const float* __restrict__ lg, int R, int T, int C,
                                    const int* __restrict__ tlen, float floor_, float* __restrict__ out,
                                    float* __restrict__ aux) {
  const long long total = (long long)R * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C), r = (int)(i / C);
    const int tl = rg_clamp(tlen[r], 1, T);
    const float* xb = x + (long long)r * T * C + c;
    const float* lb = lg + (long long)r * T * C + c;
    float m = -INFINITY;
    for (int t = 0; t < tl; ++t) m = fmaxf(m, lb[(long long)t * C]);
    float z = 0.f, s1 = 0.f, s2 = 0.f;
    for (int t = 0; t < tl; ++t) {
      const float e = expf(lb[(long long)t * C] - m), v = xb[(long long)t * C];
      z += e;
      s1 += e * v;
      s2 += e * v * v;
    }
    const float mean = s1 / z, ex2 = s2 / z;
    out[(long long)r * 2 * C + c] = mean;
    out[(long long)r * 2 * C + C + c] = sqrtf(fmaxf(ex2 - mean * mean, floor_));
    float* a = aux + (long long)r * 4 * C + c;
    a[0] = m;
    a[C] = z;
    a[2 * C] = mean;
    a[3 * C] = ex2;
  }
}

// ---- per-row mean over the valid frames of [R][T][C]; CMN: subtract it and zero the tail -----------------------------
// One workgroup per (row, 64 channels): lane = channel, the four waves take the frames t = wave, wave + 4, ...; their
// partial sums are added in wave order (deterministic).  CMN = true: y[r][t][:] = t < tl ? x - mean : 0 (in place is
// fine: a frame is read and written by the same thread); CMN = false: mean [R][C] only.
template <bool CMN>
__global__ __launch_bounds__(256) void row_mean_len_kernel(const float* x, int T, int C, const int* __restrict__ tlen,
                                                           float* y) {
  __shared__ float part[4][64];
  const int r = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + lane;
  const int tl = rg_clamp(tlen[r], 1, T);
  const bool live = c < C;
  const float* xr = x + (long long)r * T * C + c;
  float s = 0.f;
  if (live)
    for (int t = wv; t < tl; t += 4) s += xr[(long long)t * C];
  part[wv][lane] = s;
  __syncthreads();
  const float mean = (part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane]) / (float)tl;
  if (!live) return;
  if (!CMN) {
    if (wv == 0) y[(long long)r * C + c] = mean;
    return;
  }
  float* yr = y + (long long)r * T * C + c;
  for (int t = wv; t < T; t += 4) yr[(long long)t * C] = t < tl ? xr[(long long)t * C] - mean : 0.f;
}

// ---- y[r][t][:] = t < tlen[r] ? x[r][t][:] : 0 on [R][T][C] (in place allowed) ----------------------------------------
__global__ void tail_select_len_kernel(const float* x, int R, int T, int C, const int* __restrict__ tlen, float* y) {
  const int c4n = C >> 2;
  const long long total = (long long)R * T * c4n;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long row = i / c4n;
    const int t = (int)(row % T), r = (int)(row / T);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t < rg_clamp(tlen[r], 0, T)) v = *reinterpret_cast<const f32x4*>(x + i * 4);
    *reinterpret_cast<f32x4*>(y + i * 4) = v;
  }
}

// ---- ws_preemph_pad whose reflect padding turns at the row's own end; nothing behind lengths[r] is read ---------------
// out[r][j] = y[reflect(j - pad)] for j < L + 2 pad, 0 behind, L = lengths[r] clamped to [max(pad + 1, 2), T]
__global__ void preemph_pad_len_kernel(const float* __restrict__ x, int R, int T, int pad, int ldo, float coef,
                                       const int* __restrict__ lengths, float* __restrict__ out) {
  const int Tp = T + 2 * pad;
  const long long total = (long long)R * Tp;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / Tp), j = (int)(i - (long long)r * Tp);
    const int L = rg_clamp(lengths[r], max(pad + 1, 2), T);      // two samples at least: y[0] reads x[1]
    float v = 0.f;
    if (j < L + 2 * pad) {
      int k = j - pad;
      if (k < 0) k = -k;
      if (k >= L) k = 2 * (L - 1) - k;
      const float* xr = x + (long long)r * T;
      v = xr[k] - coef * (k > 0 ? xr[k - 1] : xr[1]);
    }
    out[(long long)r * ldo + j] = v;
  }
}

}  // namespace

extern "C" int ws_bn_prelu_fwd_len(const float* x, const float* stats, const float* gamma, const float* beta,
                                   const float* res, const float* a, long long M, int C, int rows_per_r, int W,
                                   const int* wlen, float* u, float* y, void* stream) {
  WS_REQUIRE(wlen, "ws_bn_prelu_fwd_len: wlen table is NULL");
  WS_REQUIRE(x && stats && gamma && beta && a && u && y && M > 0 && C > 0 && C % 4 == 0, "ws_bn_prelu_fwd_len: bad args");
  WS_REQUIRE(W > 0 && rows_per_r > 0 && rows_per_r % W == 0 && M % rows_per_r == 0,
             "ws_bn_prelu_fwd_len: width W=%d must be positive and divide rows_per_r=%d, which must divide M=%lld", W,
             rows_per_r, M);
  hipLaunchKernelGGL(bn_prelu_fwd_len_kernel, dim3(rg_blocks(M * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, stats,
                     gamma, beta, res, a, M, C, rows_per_r, W, wlen, u, y);
  return ws_check_launch("ws_bn_prelu_fwd_len");
}

extern "C" int ws_tstp_fwd_len(const float* x, int R, int F, int T, int C, const int* tlen, float eps, float* stats,
                               void* stream) {
  WS_REQUIRE(tlen, "ws_tstp_fwd_len: tlen table is NULL");
  WS_REQUIRE(x && stats && R > 0 && F > 0 && T > 0 && C > 0, "ws_tstp_fwd_len: bad args");
  hipLaunchKernelGGL(tstp_fwd_len_kernel, dim3(rg_blocks((long long)R * F * C)), dim3(256), 0, (hipStream_t)stream, x, R,
                     F, T, C, tlen, eps, stats);
  return ws_check_launch("ws_tstp_fwd_len");
}

extern "C" int ws_astp_fwd_len(const float* x, const float* logits, int R, int T, int C, const int* tlen, float floor_,
                               float* out, float* aux, void* stream) {
  WS_REQUIRE(tlen, "ws_astp_fwd_len: tlen table is NULL");
  WS_REQUIRE(x && logits && out && aux && R > 0 && T > 0 && C > 0, "ws_astp_fwd_len: bad args");
  hipLaunchKernelGGL(astp_fwd_len_kernel, dim3(rg_blocks((long long)R * C)), dim3(256), 0, (hipStream_t)stream, x,
                     logits, R, T, C, tlen, floor_, out, aux);
  return ws_check_launch("ws_astp_fwd_len");
}

extern "C" int ws_time_mean_len(const float* x, int R, int T, int C, const int* tlen, float* mean, void* stream) {
  WS_REQUIRE(tlen, "ws_time_mean_len: tlen table is NULL");
  WS_REQUIRE(x && mean && R > 0 && R <= 65535 * 4 && T > 0 && C > 0, "ws_time_mean_len: bad args");
  hipLaunchKernelGGL(row_mean_len_kernel<false>, dim3(R, (C + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, T, C,
                     tlen, mean);
  return ws_check_launch("ws_time_mean_len");
}

extern "C" int ws_cmn_len(const float* x, int R, int T, int C, const int* tlen, float* y, void* stream) {
  WS_REQUIRE(tlen, "ws_cmn_len: tlen table is NULL");
  WS_REQUIRE(x && y && R > 0 && R <= 65535 * 4 && T > 0 && C > 0, "ws_cmn_len: bad args");
  hipLaunchKernelGGL(row_mean_len_kernel<true>, dim3(R, (C + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, T, C, tlen,
                     y);
  return ws_check_launch("ws_cmn_len");
}

extern "C" int ws_tail_select_len(const float* x, int R, int T, int C, const int* tlen, float* y, void* stream) {
  WS_REQUIRE(tlen, "ws_tail_select_len: tlen table is NULL");
  WS_REQUIRE(x && y && R > 0 && T > 0 && C > 0 && C % 4 == 0, "ws_tail_select_len: bad args (C %% 4)");
  hipLaunchKernelGGL(tail_select_len_kernel, dim3(rg_blocks((long long)R * T * (C / 4))), dim3(256), 0,
                     (hipStream_t)stream, x, R, T, C, tlen, y);
  return ws_check_launch("ws_tail_select_len");
}

extern "C" int ws_preemph_pad_len(const float* x, int R, int T, int pad, int ldo, float coef, const int* lengths,
                                  float* out, void* stream) {
  WS_REQUIRE(lengths, "ws_preemph_pad_len: lengths table is NULL");
  WS_REQUIRE(x && out && R > 0 && T > 1 && T > pad && pad >= 0 && ldo >= T + 2 * pad,
             "ws_preemph_pad_len: bad args (T > pad)");
  hipLaunchKernelGGL(preemph_pad_len_kernel, dim3(rg_blocks((long long)R * (T + 2 * pad))), dim3(256), 0,
                     (hipStream_t)stream, x, R, T, pad, ldo, coef, lengths, out);
  return ws_check_launch("ws_preemph_pad_len");
}
