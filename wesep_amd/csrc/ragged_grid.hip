// Length-aware kernels of the ragged TF-GridNet plan (runtime/gridnet_plan.cc): utterances of different
// lengths share ONE forward over the rectangle [R][Tf][Q][C].  Everything per frame runs over the rectangle unchanged --
// the frames behind a row's end hold finite values that nothing valid reads -- and only what reduces over time takes the
// row's frame count Tf_r = 1 + lengths[r] / hop: the GroupNorm(1, C) statistics after the input convolution
// (ws_flat_stats_len) and the overlap-add with its window envelope (ws_ola_norm_len).  ws_transpose_batched and
// ws_heads_merge_fwd replace the per-(head, row) launch loops of the attention by one launch each (pure copies).
//
// Length tables are device int[R].  Every kernel clamps the entries it reads, so no entry moves an access out of its
// row.  "Zero" is always selected, never multiplied: NaN / Inf behind a row's end do not reach a valid output.
// All four are HBM-bound passes: 16-byte accesses along the contiguous axis, grid-stride loops, block reductions in a
// fixed order, no atomics.
#include "common.h"

namespace {

inline int gg_blocks(long long n, int per = 256, int cap = 32768) {   // grid-stride kernels: the cap of tasnet.hip's ew_blocks
  long long b = (n + per - 1) / per;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

__device__ __forceinline__ int gg_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- chunked mean / variance of the first glen[g] * per_step floats of every group -------------------------------------
// flat_stats_chunk_kernel / flat_stats_final_kernel of tasnet.hip with the group's own count: the same two-pass
// (count, mean, M2) triple per chunk and the same fixed merge order, but a group's chunks divide ITS count, and nothing
// behind the count is read.
__global__ __launch_bounds__(256) void flat_stats_len_chunk_kernel(const float* __restrict__ x, long long n_per_group,
                                                                   const int* __restrict__ glen, int per_step, int nchunk,
                                                                   float* __restrict__ scratch) {
  __shared__ float red[16];
  const int g = blockIdx.y, ch = blockIdx.x;
  const int steps = gg_clamp(glen[g], 1, (int)(n_per_group / per_step));
  const long long n4 = ((long long)steps * per_step) >> 2;
  const long long per = (n4 + nchunk - 1) / nchunk;
  const long long lo = ch * per, hi = min(n4, lo + per);
  const f32x4* xb = reinterpret_cast<const f32x4*>(x + (long long)g * n_per_group);
  float s = 0.f;
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const f32x4 t = xb[i];
    s += (t[0] + t[1]) + (t[2] + t[3]);
  }
  const float cnt = (float)(max(hi - lo, 0LL) * 4);
  const float mean = cnt > 0.f ? ws_block_sum(s, red) / cnt : 0.f;
  float q = 0.f;
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const f32x4 t = xb[i] - mean;
    q += (t[0] * t[0] + t[1] * t[1]) + (t[2] * t[2] + t[3] * t[3]);
  }
  q = ws_block_sum(q, red);
  if (threadIdx.x == 0) {
    float* o = scratch + ((long long)g * nchunk + ch) * 4;
    o[0] = cnt;
    o[1] = mean;
    o[2] = q;
  }
}

__device__ __forceinline__ void gg_chan_merge(double& n, double& mean, double& m2, double nb, double mb, double qb) {
  if (nb <= 0.0) return;
  const double nt = n + nb, d = mb - mean;
  mean += d * nb / nt;
  m2 += qb + d * d * n * nb / nt;
  n = nt;
}

// one wave per group: lane l merges chunks l, l + 64, ... serially, then a shuffle butterfly merges the 64 partial
// triples, (lower lane's, upper lane's) in that order -- the order of flat_stats_final_kernel
__global__ __launch_bounds__(64) void flat_stats_len_final_kernel(const float* __restrict__ scratch, int nchunk, float eps,
                                                                  float* __restrict__ stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int c = lane; c < nchunk; c += 64) {
    const float* s = scratch + ((long long)g * nchunk + c) * 4;
    gg_chan_merge(n, mean, m2, s[0], s[1], s[2]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double nb = __shfl_xor(n, o, 64), mb = __shfl_xor(mean, o, 64), qb = __shfl_xor(m2, o, 64);
    double an = n, am = mean, aq = m2, bn = nb, bm = mb, bq = qb;
    if (lane & o) {
      an = nb; am = mb; aq = qb; bn = n; bm = mean; bq = m2;
    }
    gg_chan_merge(an, am, aq, bn, bm, bq);
    n = an; mean = am; m2 = aq;
  }
  if (lane == 0) {
    stats[2 * g] = (float)mean;
    stats[2 * g + 1] = 1.f / sqrtf((float)(m2 / n) + eps);
  }
}

// ---- overlap-add of the frames t < Tf_r, 1 / window envelope over those frames, centre trim, zeros from lengths[r] -------
// hop = n / 2: sample j = i + n / 2 of the untrimmed signal lies in the frames t1 = j / hop (first half of the window) and
// t1 - 1 (second half).  The sum adds the earlier frame first, as ola_fwd does; the envelope is the double sum of the
// squared float window values, inverted in double and rounded once, as the host-built table of the rectangular plan.
// One thread per 4 consecutive samples (hop % 4 == 0: they share t1): 16-byte loads of both frames and of the window.
__global__ void ola_norm_len_kernel(const float* __restrict__ frames, const float* __restrict__ win, int R, int Tf, int n,
                                    int T, const int* __restrict__ lengths, float* __restrict__ est) {
  const int hop = n >> 1, T4 = (T + 3) >> 2;
  const long long total = (long long)R * T4;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(idx / T4), i0 = (int)(idx - (long long)r * T4) * 4;
    const int len = gg_clamp(lengths[r], 0, T);
    const int tfr = 1 + len / hop;                      // <= Tf = 1 + T / hop (checked by the launcher)
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i0 < len) {
      const int j = i0 + hop, t1 = j / hop, k = j - t1 * hop;   // t1 >= 1: the earlier frame t1 - 1 always exists
      const float* fr = frames + ((long long)r * Tf + (t1 - 1)) * n;
      const f32x4 a = *reinterpret_cast<const f32x4*>(fr + hop + k);
      const f32x4 wa = *reinterpret_cast<const f32x4*>(win + hop + k);
      f32x4 b = {0.f, 0.f, 0.f, 0.f}, wb = {0.f, 0.f, 0.f, 0.f};
      const bool two = t1 < tfr;
      if (two) {
        b = *reinterpret_cast<const f32x4*>(fr + n + k);
        wb = *reinterpret_cast<const f32x4*>(win + k);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        double env = (double)wa[u] * (double)wa[u];
        float sum = a[u];
        if (two) {
          env += (double)wb[u] * (double)wb[u];
          sum += b[u];
        }
        v[u] = i0 + u < len ? sum * (float)(1.0 / env) : 0.f;
      }
    }
    float* o = est + (long long)r * T + i0;
    if (i0 + 3 < T && (T & 3) == 0) {
      *reinterpret_cast<f32x4*>(o) = v;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i0 + u < T) o[u] = v[u];
    }
  }
}

// ---- [G][rows][cols] -> [G][cols][rows] through a 64 x 64 LDS tile ------------------------------------------------------
// 256 threads: 16-byte loads along cols, 16-byte stores along rows (rows % 4 == 0, cols % 4 == 0, so a quad is inside or
// outside as a whole).  tile[c][r] with a row pitch of 65 floats: the transposed scalar writes of a load hit 64 distinct
// banks modulo the pitch, the reads of a store walk a row.
__global__ __launch_bounds__(256) void transpose_batched_kernel(const float* __restrict__ src, int G, int rows, int cols,
                                                                float* __restrict__ dst) {
  __shared__ float tile[64][65];
  const int tr = (rows + 63) >> 6, tc = (cols + 63) >> 6;
  const long long ntile = (long long)G * tr * tc;
  const int q = threadIdx.x & 15, line = threadIdx.x >> 4;     // quad within a 64-float line, line 0..15 (+16 per pass)
  for (long long t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int g = (int)(t / (tr * tc)), rem = (int)(t - (long long)g * tr * tc);
    const int r0 = (rem / tc) << 6, c0 = (rem % tc) << 6;
    const float* s = src + (long long)g * rows * cols;
    float* d = dst + (long long)g * rows * cols;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int r = r0 + line + 16 * p, c = c0 + 4 * q;
      if (r < rows && c < cols) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(s + (long long)r * cols + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) tile[4 * q + u][line + 16 * p] = v[u];
      }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int c = c0 + line + 16 * p, r = r0 + 4 * q;
      if (c < cols && r < rows) {
        f32x4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = tile[line + 16 * p][4 * q + u];
        *reinterpret_cast<f32x4*>(d + (long long)c * rows + r) = v;
      }
    }
    __syncthreads();
  }
}

// ---- head merge: ov [nh][R][P][cp] -> o [R][P][nh * cp], P = frames * bins of a row ---------------------------------------
__global__ void heads_merge_fwd_kernel(const float* __restrict__ ov, int nh, int R, long long P, int cp, float* __restrict__ o) {
  const int c4n = (nh * cp) >> 2, cp4 = cp >> 2;
  const long long total = (long long)R * P * c4n;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long row = i / c4n;                      // r * P + p
    const int c4 = (int)(i - row * c4n), h = c4 / cp4, e4 = c4 - h * cp4;
    *reinterpret_cast<f32x4*>(o + i * 4) =
        *reinterpret_cast<const f32x4*>(ov + (((long long)h * R * P + row) * cp4 + e4) * 4);
  }
}

}  // namespace

extern "C" int ws_flat_stats_len(const float* x, int ngroups, long long n_per_group, const int* glen, int per_step,
                                 float eps, int nchunk, float* scratch, float* stats, void* stream) {
  WS_REQUIRE(glen, "ws_flat_stats_len: glen table is NULL");
  WS_REQUIRE(x && scratch && stats && ngroups > 0 && ngroups <= 65535 && n_per_group > 0 && nchunk > 0 && nchunk <= 65535,
             "ws_flat_stats_len: bad args");
  WS_REQUIRE(per_step > 0 && per_step % 4 == 0 && n_per_group % per_step == 0 && n_per_group / per_step <= 0x7fffffffLL,
             "ws_flat_stats_len: per_step=%d must be a positive multiple of 4 that divides n_per_group=%lld", per_step,
             n_per_group);
  hipLaunchKernelGGL(flat_stats_len_chunk_kernel, dim3(nchunk, ngroups), dim3(256), 0, (hipStream_t)stream, x,
                     n_per_group, glen, per_step, nchunk, scratch);
  hipLaunchKernelGGL(flat_stats_len_final_kernel, dim3(ngroups), dim3(64), 0, (hipStream_t)stream, scratch, nchunk, eps,
                     stats);
  return ws_check_launch("ws_flat_stats_len");
}

extern "C" int ws_ola_norm_len(const float* frames, const float* win, int R, int Tf, int n, int T, const int* lengths,
                               float* est, void* stream) {
  WS_REQUIRE(lengths, "ws_ola_norm_len: lengths table is NULL");
  WS_REQUIRE(frames && win && est && R > 0 && Tf > 0 && T > 0, "ws_ola_norm_len: bad args");
  WS_REQUIRE(n >= 8 && n % 8 == 0, "ws_ola_norm_len: n=%d must be a multiple of 8 (hop = n / 2, 16-byte accesses)", n);
  WS_REQUIRE(Tf == 1 + T / (n / 2), "ws_ola_norm_len: Tf=%d does not match T=%d (Tf = 1 + T / hop, hop = %d)", Tf, T, n / 2);
  hipLaunchKernelGGL(ola_norm_len_kernel, dim3(gg_blocks((long long)R * ((T + 3) / 4))), dim3(256), 0,
                     (hipStream_t)stream, frames, win, R, Tf, n, T, lengths, est);
  return ws_check_launch("ws_ola_norm_len");
}

extern "C" int ws_transpose_batched(const float* src, int G, int rows, int cols, float* dst, void* stream) {
  WS_REQUIRE(src && dst && src != dst && G > 0 && rows > 0 && cols > 0, "ws_transpose_batched: bad args");
  WS_REQUIRE(rows % 4 == 0 && cols % 4 == 0, "ws_transpose_batched: rows=%d and cols=%d must be multiples of 4", rows, cols);
  const long long ntile = (long long)G * ((rows + 63) / 64) * ((cols + 63) / 64);
  hipLaunchKernelGGL(transpose_batched_kernel, dim3(gg_blocks(ntile, 1)), dim3(256), 0, (hipStream_t)stream, src, G, rows,
                     cols, dst);
  return ws_check_launch("ws_transpose_batched");
}

extern "C" int ws_heads_merge_fwd(const float* ov, int nh, int R, long long P, int cp, float* o, void* stream) {
  WS_REQUIRE(ov && o && ov != o && nh > 0 && R > 0 && P > 0 && cp > 0 && cp % 4 == 0,
             "ws_heads_merge_fwd: bad args (cp %% 4)");
  hipLaunchKernelGGL(heads_merge_fwd_kernel, dim3(gg_blocks((long long)R * P * (nh * cp / 4))), dim3(256), 0,
                     (hipStream_t)stream, ov, nh, R, P, cp, o);
  return ws_check_launch("ws_heads_merge_fwd");
}
