// Chunked (streaming) forms of the two Conv-TasNet kernels that look across time, for causal models fed audio as it
// arrives (wesep_amd/streaming.py): the causal depthwise dilated convolution with a ring of past normalised frames, and
// the overlap-add with a carry of the samples that later frames still add to.  Everything else in the causal model is
// per frame.  All carried state is device memory owned by the caller; both kernels update it in the launch that uses it.
// Both are built to give, over any chunking, bit for bit what dwconv_fwd_kernel(causal) / ola_fwd_kernel (tasnet.hip)
// give over the whole sequence: same operand expression (tasnet_dw.h), same order of additions.  Plain C++, no atomics.
#include "common.h"
#include "tasnet_dw.h"

namespace {

// y[r][t][c] = b[c] + sum_p w[c][p] * xn(r, t0 + t - (P-1-p)*dil), ascending p.  xn(a): the chunk's own normalised frame
// for a >= t0, ring slot a % cap for 0 <= a < t0, and NO term for a < 0 (the whole-sequence kernel skips the tap, too; the
// ring is not read there, so whatever it holds -- NaN included -- cannot reach an output).  Every chunk frame's normalised
// value goes to its slot in the same launch: with cap >= (P-1)*dil + Tc the slot written for frame a last held frame
// a - cap < t0 - (P-1)*dil, which no output of this chunk reads, and the Tc written slots are distinct -- no second buffer.
// threadIdx.y picks the frame (grid-stride over the R*Tc frames), threadIdx.x the channel quad (16-byte accesses): the
// slots of a frame's taps are computed once per frame from wave-uniform values, without a division (base = t0 % cap comes
// from the host; base + t - off lies in (-cap, 2 cap)).
__global__ __launch_bounds__(256) void dwconv_stream_kernel(const float* __restrict__ x,
                                                            const float* __restrict__ stats,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            DwGeom g, long long t0, int base, int cap, float* ring,
                                                            float* __restrict__ y) {
  const int c4n = g.C >> 2;
  const long long frames = (long long)g.R * g.Tp;
  for (long long f = (long long)blockIdx.x * blockDim.y + threadIdx.y; f < frames;
       f += (long long)gridDim.x * blockDim.y) {
    const int r = (int)(f / g.Tp), t = (int)(f - (long long)r * g.Tp);
    float* rr = ring + (long long)r * cap * g.C;
    long long src[TN_MAXP];     // >= 0: offset of the tap's frame in the ring row; -1: chunk frame; -2: before the start
    int dt[TN_MAXP];            // chunk frame of the tap relative to t
#pragma unroll
    for (int p = 0; p < TN_MAXP; ++p) {
      if (p >= g.P) break;
      const int off = (g.P - 1 - p) * g.dil;
      dt[p] = -off;
      if (t0 + t - off < 0) {
        src[p] = -2;
      } else if (off <= t) {
        src[p] = -1;
      } else {
        int s = base + t - off;
        s = s < 0 ? s + cap : (s >= cap ? s - cap : s);
        src[p] = (long long)s * g.C;
      }
    }
    int own = base + t;
    own = own >= cap ? own - cap : own;
    for (int q = threadIdx.x; q < c4n; q += blockDim.x) {
      const int c = q * 4;
      const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c), bt = *reinterpret_cast<const f32x4*>(beta + c);
      f32x4 acc = *reinterpret_cast<const f32x4*>(b + c);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int p = 0; p < TN_MAXP; ++p) {
        if (p >= g.P) break;
        if (src[p] == -2) continue;
        v = src[p] == -1 ? dw_xn(x, stats, gm, bt, g, f + dt[p], c) : *reinterpret_cast<const f32x4*>(rr + src[p] + c);
        dw_tap(acc, w, c, g.P, p, v);
      }
      // the last tap (p = P - 1, offset 0) is the frame itself and is never skipped: v holds its normalised value
      *reinterpret_cast<f32x4*>(rr + (long long)own * g.C + c) = v;
      *reinterpret_cast<f32x4*>(y + f * g.C + c) = acc;
    }
  }
}

// One workgroup per row.  The row's carry (bias + what earlier frames added to the L - hop samples that are not final yet)
// is copied to LDS first, so the in-place update cannot read a slot another thread has already replaced.  Then one thread
// per sample i of [0, Tc*hop + L - hop), relative to the chunk's first sample: acc = carry[i] (i < L - hop) or the bias,
// plus the chunk's frames that cover i in ascending t -- the additions of ola_fwd_kernel in its order.  i < Tc*hop is
// final and goes to est; the rest is the new carry.
__global__ __launch_bounds__(256) void ola_stream_kernel(const float* __restrict__ frames, const float* __restrict__ bias,
                                                         int Tc, int L, int hop, float* carry, float* __restrict__ est) {
  extern __shared__ float old_carry[];
  const int r = blockIdx.x, nc = L - hop, nfin = Tc * hop;
  float* cr = carry + (long long)r * nc;
  for (int i = threadIdx.x; i < nc; i += blockDim.x) old_carry[i] = cr[i];
  __syncthreads();
  const float bv = bias ? bias[0] : 0.f;
  const float* fr = frames + (long long)r * Tc * L;
  for (int i = threadIdx.x; i < nfin + nc; i += blockDim.x) {
    int t_hi = i / hop;
    if (t_hi > Tc - 1) t_hi = Tc - 1;
    int t_lo = (i - L + hop) / hop;  // ceil((i - L + 1) / hop)
    if (i - L + 1 <= 0) t_lo = 0;
    float acc = i < nc ? old_carry[i] : bv;
    for (int t = t_lo; t <= t_hi; ++t) acc += fr[(long long)t * L + (i - hop * t)];
    if (i < nfin)
      est[(long long)r * nfin + i] = acc;
    else
      cr[i - nfin] = acc;
  }
}

}  // namespace

extern "C" int ws_dwconv_stream_fwd(const float* x, const float* stats, const float* gamma, const float* beta,
                                    const float* w, const float* b, int R, int Tc, int C, int P, int dil, int st_div,
                                    long long t0, int cap, float* ring, float* y, void* stream) {
  WS_REQUIRE(x && stats && gamma && beta && w && b && ring && y, "ws_dwconv_stream_fwd: null pointer");
  WS_REQUIRE(R > 0 && Tc > 0 && C > 0 && dil >= 1 && st_div > 0, "ws_dwconv_stream_fwd: bad geometry (R=%d, Tc=%d, C=%d, dil=%d, st_div=%d)",
             R, Tc, C, dil, st_div);
  WS_REQUIRE(C % 4 == 0, "ws_dwconv_stream_fwd: C=%d is not a multiple of 4", C);
  WS_REQUIRE(P >= 1 && P <= TN_MAXP && (P & 1), "ws_dwconv_stream_fwd: P=%d (odd P <= %d)", P, TN_MAXP);
  WS_REQUIRE(t0 >= 0, "ws_dwconv_stream_fwd: t0=%lld is negative", t0);
  const long long need = (long long)(P - 1) * dil + Tc;
  WS_REQUIRE(cap >= need, "ws_dwconv_stream_fwd: cap=%d is below (P - 1) * dil + Tc = %lld", cap, need);
  const long long n = (long long)R * Tc * C;
  WS_REQUIRE(y + n <= x || x + n <= y, "ws_dwconv_stream_fwd: y overlaps x");
  const DwGeom g{R, Tc, C, P, dil, st_div, P - 1};
  const int tx = C / 4 >= 256 ? 256 : ((C / 4 + 63) / 64) * 64, ty = 256 / tx;
  long long blocks = ((long long)R * Tc + ty - 1) / ty;
  if (blocks > 32768) blocks = 32768;
  hipLaunchKernelGGL(dwconv_stream_kernel, dim3((unsigned)blocks), dim3(tx, ty), 0, (hipStream_t)stream, x, stats, gamma,
                     beta, w, b, g, t0, (int)(t0 % cap), cap, ring, y);
  return ws_check_launch("ws_dwconv_stream_fwd");
}

extern "C" int ws_ola_stream_fwd(const float* frames, const float* bias, int R, int Tc, int L, int hop, float* carry,
                                 float* est, void* stream) {
  WS_REQUIRE(frames && est, "ws_ola_stream_fwd: frames or est is NULL");
  WS_REQUIRE(R > 0 && Tc > 0 && L > 0 && hop > 0, "ws_ola_stream_fwd: bad args (R=%d, Tc=%d, L=%d, hop=%d)", R, Tc, L, hop);
  WS_REQUIRE(L >= hop && L % hop == 0, "ws_ola_stream_fwd: L=%d is not a multiple of hop=%d", L, hop);
  WS_REQUIRE(carry || L == hop, "ws_ola_stream_fwd: carry is NULL (L > hop)");
  WS_REQUIRE(L - hop <= 16384, "ws_ola_stream_fwd: L - hop = %d above 16384 (the carry row is staged in LDS)", L - hop);
  WS_REQUIRE((long long)Tc * hop + L < (1LL << 31), "ws_ola_stream_fwd: Tc * hop + L reaches 2^31");
  hipLaunchKernelGGL(ola_stream_kernel, dim3(R), dim3(256), (size_t)(L - hop) * sizeof(float), (hipStream_t)stream,
                     frames, bias, Tc, L, hop, carry, est);
  return ws_check_launch("ws_ola_stream_fwd");
}
