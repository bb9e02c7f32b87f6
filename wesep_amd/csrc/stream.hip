// Chunked (streaming) forms of the two Conv-TasNet kernels that look across time, for causal models fed audio as it
// arrives (wesep_amd/streaming.py): the causal depthwise dilated convolution with a ring of past normalised frames, and
// the overlap-add with a carry of the samples that later frames still add to.  Everything else in the causal model is
// per frame.  All carried state is device memory owned by the caller; both kernels update it in the launch that uses it.
// Both are built to give, over any chunking, bit for bit what dwconv_fwd_kernel(causal) / ola_fwd_kernel (tasnet.hip)
// give over the whole sequence: same operand expression (tasnet_dw.h), same order of additions.  Plain C++, no atomics.
// tcn_mid_stream_kernel is the whole middle of a causal cLN block (PReLU, statistics, the ring convolution, PReLU,
// statistics) in one launch, for small chunks where the five launches it replaces cost more than their work.
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

// One workgroup per row (ola_stream_row: the solo kernel and the pool's share it).  The row's carry (bias + what earlier
// frames added to the L - hop samples that are not final yet) is copied to LDS first, so the in-place update cannot read a slot another thread has already replaced.  Then one thread
// per sample i of [0, Tc*hop + L - hop), relative to the chunk's first sample: acc = carry[i] (i < L - hop) or the bias,
// plus the chunk's frames that cover i in ascending t -- the additions of ola_fwd_kernel in its order.  i < Tc*hop is
// final and goes to est; the rest is the new carry.
__device__ __forceinline__ void ola_stream_row(const float* __restrict__ fr, float bv, int Tc, int L, int hop, float* cr,
                                               float* __restrict__ er, float* old_carry) {
  const int nc = L - hop, nfin = Tc * hop;
  for (int i = threadIdx.x; i < nc; i += blockDim.x) old_carry[i] = cr[i];
  __syncthreads();
  for (int i = threadIdx.x; i < nfin + nc; i += blockDim.x) {
    int t_hi = i / hop;
    if (t_hi > Tc - 1) t_hi = Tc - 1;
    int t_lo = (i - L + hop) / hop;  // ceil((i - L + 1) / hop)
    if (i - L + 1 <= 0) t_lo = 0;
    float acc = i < nc ? old_carry[i] : bv;
    for (int t = t_lo; t <= t_hi; ++t) acc += fr[(long long)t * L + (i - hop * t)];
    if (i < nfin)
      er[i] = acc;
    else
      cr[i - nfin] = acc;
  }
}

__global__ __launch_bounds__(256) void ola_stream_kernel(const float* __restrict__ frames, const float* __restrict__ bias,
                                                         int Tc, int L, int hop, float* carry, float* __restrict__ est) {
  extern __shared__ float old_carry[];
  const int r = blockIdx.x;
  ola_stream_row(frames + (long long)r * Tc * L, bias ? bias[0] : 0.f, Tc, L, hop, carry + (long long)r * (L - hop),
                 est + (long long)r * Tc * hop, old_carry);
}

// The same for the rows of a stream pool: row i of the [A][Tc] rectangle carries tc[i] <= Tc frames of the stream whose
// carry is row slot[i] of carry [nslots][L - hop].  ola_stream_row runs with the row's own frame count -- the additions of
// the solo kernel with (R = 1, Tc = tc[i]) in its order -- and the rest of the est row, up to its pitch Tc * hop, is zero.
// A row with tc[i] = 0 (or a table entry that names no slot: out of range, or t0 < 0) leaves before the barrier, which a
// workgroup does as one: the carry row is neither read nor written.
__global__ __launch_bounds__(256) void ola_stream_rows_kernel(const float* __restrict__ frames, const float* __restrict__ bias,
                                                              int Tc, int L, int hop, int nslots, const int* __restrict__ slot,
                                                              const long long* __restrict__ t0, const int* __restrict__ tc,
                                                              float* carry, float* __restrict__ est) {
  extern __shared__ float old_carry[];
  const int i = blockIdx.x, sl = slot[i];
  int n = tc[i];
  n = n > Tc ? Tc : n;
  if (n < 0 || sl < 0 || sl >= nslots || t0[i] < 0) n = 0;
  float* er = est + (long long)i * Tc * hop;
  for (int j = n * hop + threadIdx.x; j < Tc * hop; j += blockDim.x) er[j] = 0.f;
  if (n == 0) return;
  ola_stream_row(frames + (long long)i * Tc * L, bias ? bias[0] : 0.f, n, L, hop, carry + (long long)sl * (L - hop), er, old_carry);
}

// The middle of a causal cLN block on one chunk, between its two GEMMs: PReLU, cLN statistics, the depthwise convolution
// with its ring, PReLU, cLN statistics.  One workgroup per (row, chunk frame); thread i owns the channel quads i, i + NT, ...
// of every frame it touches.  A tap inside the chunk is NOT read from the ring (another workgroup of this launch writes
// it): the workgroup recomputes that frame's y1, statistics and xn from c -- a few KB of L2 hits per tap.  Every workgroup
// has the same NT (a function of H alone) and walks a frame in the same order, so a frame's xn is the same bits whether its
// own workgroup computes it (and writes it to the ring) or a later frame's does; a later chunk reads those bits back.
// Statistics: the two-pass mean / variance of group_stats_kernel (norm.hip) with its per-thread and cross-wave order.
// LDS (dynamic): y1 of the tap in hand [H], the accumulator / y2 [H], 16 floats for the cross-wave sums; a thread reads
// back only the quads it wrote, so the barriers are those of ws_block_sum alone.  Nothing here waits on another workgroup.
//
// One frame of the fused middle, by one workgroup: cf = the frame's row of c (its chunk predecessors lie before it), rbr
// the row's bias or NULL, rr the row's ring [cap][H], t the frame's index in its chunk, t0 / base the chunk's first frame
// and t0 % cap, y2f / st2f the frame's outputs.  The solo kernel and the pool's share it: one expression, one order.
__device__ __forceinline__ void tcn_mid_stream_frame(const float* __restrict__ cf, const float* __restrict__ rbr,
                                                     const float* __restrict__ a1, const float* __restrict__ gamma1,
                                                     const float* __restrict__ beta1, const float* __restrict__ wd,
                                                     const float* __restrict__ bd, const float* __restrict__ a2, int t, int H,
                                                     int P, int dil, float eps, long long t0, int base, int cap, float* rr,
                                                     float* __restrict__ y2f, float* __restrict__ st2f) {
  extern __shared__ __attribute__((aligned(16))) float tm_lds[];
  f32x4* stage = reinterpret_cast<f32x4*>(tm_lds);
  f32x4* accs = reinterpret_cast<f32x4*>(tm_lds + H);
  float* red = tm_lds + 2 * H;
  const int c4n = H >> 2, nt = blockDim.x;
  const float sl1 = a1[0], sl2 = a2[0];
  for (int q = threadIdx.x; q < c4n; q += nt) accs[q] = *reinterpret_cast<const f32x4*>(bd + 4 * q);
#pragma unroll 1
  for (int p = 0; p < P; ++p) {
    const int off = (P - 1 - p) * dil;
    if (t0 + t - off < 0) continue;                       // before the start: no term, the ring is not read
    if (off <= t) {                                       // a frame of this chunk: from c
      const float* cr = cf - (long long)off * H;
      float s = 0.f;
      for (int q = threadIdx.x; q < c4n; q += nt) {
        f32x4 v = *reinterpret_cast<const f32x4*>(cr + 4 * q);
        if (rbr) v += *reinterpret_cast<const f32x4*>(rbr + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : sl1 * v[j];
        stage[q] = v;
        s += (v[0] + v[1]) + (v[2] + v[3]);
      }
      const float mean = ws_block_sum(s, red) / (float)H;
      float qs = 0.f;
      for (int q = threadIdx.x; q < c4n; q += nt) {
        const f32x4 d = stage[q] - mean;
        qs += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
      }
      const float rstd = 1.f / sqrtf(ws_block_sum(qs, red) / (float)H + eps);
      int own = base + t;
      own = own >= cap ? own - cap : own;
      for (int q = threadIdx.x; q < c4n; q += nt) {
        const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma1 + 4 * q), bt = *reinterpret_cast<const f32x4*>(beta1 + 4 * q);
        const f32x4 xn = (stage[q] - mean) * rstd * gm + bt;
        if (off == 0) *reinterpret_cast<f32x4*>(rr + (long long)own * H + 4 * q) = xn;
        f32x4 acc = accs[q];
        dw_tap(acc, wd, 4 * q, P, p, xn);
        accs[q] = acc;
      }
    } else {                                              // an earlier chunk's frame: its slot (base + t - off in (-cap, cap))
      int sl = base + t - off;
      sl = sl < 0 ? sl + cap : (sl >= cap ? sl - cap : sl);
      const float* rs = rr + (long long)sl * H;
      for (int q = threadIdx.x; q < c4n; q += nt) {
        const f32x4 xn = *reinterpret_cast<const f32x4*>(rs + 4 * q);
        f32x4 acc = accs[q];
        dw_tap(acc, wd, 4 * q, P, p, xn);
        accs[q] = acc;
      }
    }
  }
  float s = 0.f;
  for (int q = threadIdx.x; q < c4n; q += nt) {
    f32x4 v = accs[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : sl2 * v[j];
    accs[q] = v;
    *reinterpret_cast<f32x4*>(y2f + 4 * q) = v;
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = ws_block_sum(s, red) / (float)H;
  float qs = 0.f;
  for (int q = threadIdx.x; q < c4n; q += nt) {
    const f32x4 d = accs[q] - mean;
    qs += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
  }
  const float var = ws_block_sum(qs, red) / (float)H;
  if (threadIdx.x == 0) {
    st2f[0] = mean;
    st2f[1] = 1.f / sqrtf(var + eps);
  }
}

__global__ __launch_bounds__(256) void tcn_mid_stream_kernel(const float* __restrict__ c, const float* __restrict__ rb,
                                                             const float* __restrict__ a1,
                                                             const float* __restrict__ gamma1,
                                                             const float* __restrict__ beta1,
                                                             const float* __restrict__ wd, const float* __restrict__ bd,
                                                             const float* __restrict__ a2, int Tc, int H, int P, int dil,
                                                             float eps, long long t0, int base, int cap, float* ring,
                                                             float* __restrict__ y2, float* __restrict__ st2) {
  const long long f = blockIdx.x;
  const int r = (int)(f / Tc), t = (int)(f - (long long)r * Tc);
  tcn_mid_stream_frame(c + f * H, rb ? rb + (long long)r * H : nullptr, a1, gamma1, beta1, wd, bd, a2, t, H, P, dil, eps, t0, base,
                       cap, ring + (long long)r * cap * H, y2 + f * H, st2 + 2 * f);
}

// The fused middle for the rows of a stream pool: row i of the [A][Tc] rectangle is the stream in state slot slot[i], at
// its own first frame t0[i], with tc[i] <= Tc valid frames.  One workgroup per (i, t), the NT of the solo launch, and
// tcn_mid_stream_frame on the row's own (t0, t0 % cap, ring row, rb row): a valid frame is what the solo kernel gives with
// (R = 1, Tc = tc[i], t0 = t0[i]) -- a tap inside the chunk has a frame index <= t < tc[i], so only valid frames are
// recomputed from c.  A workgroup with t >= tc[i] (or whose table entry names no slot: out of range, or t0 < 0) writes
// zeros to its y2 row and (0, 1) to its st2 pair, so the next GEMM's norm-on-load stays finite, and leaves before the first
// barrier; the condition depends on blockIdx alone, so the workgroup leaves as one.  It touches no ring.
__global__ __launch_bounds__(256) void tcn_mid_stream_rows_kernel(
    const float* __restrict__ c, const float* __restrict__ rb, const float* __restrict__ a1, const float* __restrict__ gamma1,
    const float* __restrict__ beta1, const float* __restrict__ wd, const float* __restrict__ bd, const float* __restrict__ a2,
    int Tc, int H, int P, int dil, float eps, int nslots, const int* __restrict__ slot, const long long* __restrict__ t0,
    const int* __restrict__ tc, int cap, float* ring, float* __restrict__ y2, float* __restrict__ st2) {
  const long long f = blockIdx.x;
  const int i = (int)(f / Tc), t = (int)(f - (long long)i * Tc);
  const int sl = slot[i];
  const long long first = t0[i];
  int n = tc[i];
  n = n > Tc ? Tc : n;
  if (sl < 0 || sl >= nslots || first < 0) n = 0;
  if (t >= n) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int q = threadIdx.x; q < (H >> 2); q += blockDim.x) *reinterpret_cast<f32x4*>(y2 + f * H + 4 * q) = z;
    if (threadIdx.x == 0) {
      st2[2 * f] = 0.f;
      st2[2 * f + 1] = 1.f;
    }
    return;
  }
  tcn_mid_stream_frame(c + f * H, rb ? rb + (long long)sl * H : nullptr, a1, gamma1, beta1, wd, bd, a2, t, H, P, dil, eps, first,
                       (int)(first % cap), cap, ring + (long long)sl * cap * H, y2 + f * H, st2 + 2 * f);
}

}  // namespace

extern "C" int ws_tcn_mid_stream_fwd(const float* c, const float* rb, const float* a1, const float* gamma1,
                                     const float* beta1, const float* wd, const float* bd, const float* a2, int R, int Tc,
                                     int H, int P, int dil, float eps, long long t0, int cap, float* ring, float* y2,
                                     float* st2, void* stream) {
  WS_REQUIRE(c && a1 && gamma1 && beta1 && wd && bd && a2 && ring && y2 && st2, "ws_tcn_mid_stream_fwd: null pointer");
  WS_REQUIRE(R > 0 && Tc > 0 && H > 0 && dil >= 1, "ws_tcn_mid_stream_fwd: bad geometry (R=%d, Tc=%d, H=%d, dil=%d)", R, Tc,
             H, dil);
  WS_REQUIRE(H % 4 == 0, "ws_tcn_mid_stream_fwd: H=%d is not a multiple of 4", H);
  WS_REQUIRE(H <= WS_TCN_MID_MAXH, "ws_tcn_mid_stream_fwd: H=%d above %d (two rows of H floats are staged in LDS)", H,
             WS_TCN_MID_MAXH);
  WS_REQUIRE(P >= 1 && P <= TN_MAXP && (P & 1), "ws_tcn_mid_stream_fwd: P=%d (odd P <= %d)", P, TN_MAXP);
  WS_REQUIRE(t0 >= 0, "ws_tcn_mid_stream_fwd: t0=%lld is negative", t0);
  const long long need = (long long)(P - 1) * dil + Tc;
  WS_REQUIRE(cap >= need, "ws_tcn_mid_stream_fwd: cap=%d is below (P - 1) * dil + Tc = %lld", cap, need);
  WS_REQUIRE((long long)R * Tc < (1LL << 31), "ws_tcn_mid_stream_fwd: R * Tc reaches 2^31");
  const long long n = (long long)R * Tc * H;
  WS_REQUIRE(y2 + n <= c || c + n <= y2, "ws_tcn_mid_stream_fwd: y2 overlaps c");
  const int nt = H / 4 >= 256 ? 256 : ((H / 4 + 63) / 64) * 64;
  hipLaunchKernelGGL(tcn_mid_stream_kernel, dim3((unsigned)((long long)R * Tc)), dim3(nt),
                     (size_t)(2 * H + 16) * sizeof(float), (hipStream_t)stream, c, rb, a1, gamma1, beta1, wd, bd, a2, Tc, H,
                     P, dil, eps, t0, (int)(t0 % cap), cap, ring, y2, st2);
  return ws_check_launch("ws_tcn_mid_stream_fwd");
}

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

extern "C" int ws_tcn_mid_stream_rows_fwd(const float* c, const float* rb, const float* a1, const float* gamma1,
                                          const float* beta1, const float* wd, const float* bd, const float* a2, int A, int Tc,
                                          int H, int P, int dil, float eps, int nslots, const int* slot, const long long* t0,
                                          const int* tc, int cap, float* ring, float* y2, float* st2, void* stream) {
  WS_REQUIRE(c && a1 && gamma1 && beta1 && wd && bd && a2 && ring && y2 && st2, "ws_tcn_mid_stream_rows_fwd: null pointer");
  WS_REQUIRE(slot && t0 && tc, "ws_tcn_mid_stream_rows_fwd: a NULL table (slot, t0 and tc are device arrays of A entries)");
  WS_REQUIRE(A > 0 && nslots > 0, "ws_tcn_mid_stream_rows_fwd: bad tables (A=%d rows, nslots=%d)", A, nslots);
  WS_REQUIRE(Tc > 0 && H > 0 && dil >= 1, "ws_tcn_mid_stream_rows_fwd: bad geometry (Tc=%d, H=%d, dil=%d)", Tc, H, dil);
  WS_REQUIRE(H % 4 == 0, "ws_tcn_mid_stream_rows_fwd: H=%d is not a multiple of 4", H);
  WS_REQUIRE(H <= WS_TCN_MID_MAXH, "ws_tcn_mid_stream_rows_fwd: H=%d above %d (two rows of H floats are staged in LDS)", H,
             WS_TCN_MID_MAXH);
  WS_REQUIRE(P >= 1 && P <= TN_MAXP && (P & 1), "ws_tcn_mid_stream_rows_fwd: P=%d (odd P <= %d)", P, TN_MAXP);
  const long long need = (long long)(P - 1) * dil + Tc;
  WS_REQUIRE(cap >= need, "ws_tcn_mid_stream_rows_fwd: cap=%d is below (P - 1) * dil + Tc = %lld", cap, need);
  WS_REQUIRE((long long)A * Tc < (1LL << 31), "ws_tcn_mid_stream_rows_fwd: A * Tc reaches 2^31");
  const long long n = (long long)A * Tc * H;
  WS_REQUIRE(y2 + n <= c || c + n <= y2, "ws_tcn_mid_stream_rows_fwd: y2 overlaps c");
  const int nt = H / 4 >= 256 ? 256 : ((H / 4 + 63) / 64) * 64;   // the solo launch's, a function of H alone
  hipLaunchKernelGGL(tcn_mid_stream_rows_kernel, dim3((unsigned)((long long)A * Tc)), dim3(nt),
                     (size_t)(2 * H + 16) * sizeof(float), (hipStream_t)stream, c, rb, a1, gamma1, beta1, wd, bd, a2, Tc, H, P,
                     dil, eps, nslots, slot, t0, tc, cap, ring, y2, st2);
  return ws_check_launch("ws_tcn_mid_stream_rows_fwd");
}

extern "C" int ws_ola_stream_rows_fwd(const float* frames, const float* bias, int A, int Tc, int L, int hop, int nslots,
                                      const int* slot, const long long* t0, const int* tc, float* carry, float* est,
                                      void* stream) {
  WS_REQUIRE(frames && est, "ws_ola_stream_rows_fwd: frames or est is NULL");
  WS_REQUIRE(slot && t0 && tc, "ws_ola_stream_rows_fwd: a NULL table (slot, t0 and tc are device arrays of A entries)");
  WS_REQUIRE(A > 0 && nslots > 0, "ws_ola_stream_rows_fwd: bad tables (A=%d rows, nslots=%d)", A, nslots);
  WS_REQUIRE(Tc > 0 && L > 0 && hop > 0, "ws_ola_stream_rows_fwd: bad args (Tc=%d, L=%d, hop=%d)", Tc, L, hop);
  WS_REQUIRE(L >= hop && L % hop == 0, "ws_ola_stream_rows_fwd: L=%d is not a multiple of hop=%d", L, hop);
  WS_REQUIRE(carry || L == hop, "ws_ola_stream_rows_fwd: carry is NULL (L > hop)");
  WS_REQUIRE(L - hop <= 16384, "ws_ola_stream_rows_fwd: L - hop = %d above 16384 (the carry row is staged in LDS)", L - hop);
  WS_REQUIRE((long long)Tc * hop + L < (1LL << 31), "ws_ola_stream_rows_fwd: Tc * hop + L reaches 2^31");
  hipLaunchKernelGGL(ola_stream_rows_kernel, dim3(A), dim3(256), (size_t)(L - hop) * sizeof(float), (hipStream_t)stream,
                     frames, bias, Tc, L, hop, nslots, slot, t0, tc, carry, est);
  return ws_check_launch("ws_ola_stream_rows_fwd");
}
