// MHASTP / MQMHASTP pooling of the wespeaker ResNet speaker encoder (wespeaker pooling_layers.py, restated in
// tests/pooling_ref.py) on the channels-last activation x [R][F][T][C] of the last residual block.
//
// Q queries (MQMHASTP; MHASTP is Q = 1) each split the [C*F] feature axis into H heads: head h is the channel range
// [h*Ch, (h+1)*Ch) times all F rows, d_model dm = Ch*F, upstream feature index c*F + f ("native").  Per (query, head):
//   a = W2 tanh(W1 x_t + b1) + b2   (layers 2: W1 [64][dm], W2 [ds][64])   or   a = W1 x_t + b1   (layers 1: W1 [ds][dm])
//   alpha = softmax_T(a) (ds = 1: one logit row broadcast over the head; ds = dm: one per feature)
//   mean = sum_t alpha x,  var = sum_t alpha x^2 - mean^2,  std = sqrt(max(var, 1e-7))
// out [R][Q][H][2][dm] (mean || std per head, native order -- wespeaker's cat order).
//
// Arithmetic: fp32 VALU FMA throughout.  The pooling is a few GFLOP per training step, so the MFMA split-bf16 GEMMs of the
// trunk buy little here, and fp32 keeps the attention logits (which go through exp) at fp32 rounding.
//
// Forward: one workgroup per (r, h) serves all Q queries; it streams T in tiles of up to MH_TT frames staged in LDS in
// (f, c_local) order (the "kernel" feature order k = f*Ch + c) and keeps an online softmax per feature (running max,
// sum exp, sum e x, sum e x^2) in aux, so any T works.  W1's columns are permuted to the kernel order once per weight
// version (ws_mhastp_pack).  Backward: the same workgroup recomputes the attention MLP per tile, writes dx once (all
// queries accumulate in LDS), and -- for the weight gradients -- d(pre-tanh), tanh output and d(logit) per frame into a
// workspace; mhastp_wgrad_kernel turns those into per-split partial weight gradients (64 x 64 output tiles) and
// ws_reduce_slabs sums the splits in a fixed order: no atomics, the same bits every run.
#include <math.h>

#include "common.h"

namespace {

constexpr int MH_THREADS = 256;
constexpr int MH_TT = 16;             // frames per tile at most (register accumulators per thread)
constexpr int MH_LDS_FLOATS = 16384;  // 64 KiB of dynamic LDS per workgroup at most
constexpr float MH_FLOOR = 1e-7f;     // var.clamp(min=1e-7)

struct MhGeom {
  int R, F, T, C, Q, H, layers, ds;
  int Ch, dm, n1, P1, off2, TT;
  int tchunk;                         // frames per T split (T: one split, the per-(row, head) grid)
};

__host__ __device__ inline int mh_n1(int layers, int ds) { return layers == 2 ? 64 : ds; }

// floats of one (query, head) block of the weight pack: W1p [n1][dm], b1 [n1], then (layers 2) W2 [ds][64], b2 [ds]
__host__ __device__ inline long long mh_block_floats(int layers, int ds, int dm) {
  const long long n1 = mh_n1(layers, ds);
  return n1 * dm + n1 + (layers == 2 ? 64LL * ds + ds : 0);
}

__device__ __forceinline__ int mh_native(const MhGeom& g, int k) { return (k % g.Ch) * g.F + k / g.Ch; }

__device__ __forceinline__ long long mh_xoff(const MhGeom& g, int r, int t, int h, int k) {
  return (((long long)r * g.F + k / g.Ch) * g.T + t) * g.C + (long long)h * g.Ch + k % g.Ch;
}

// hs[tt][u] = act(b1[u] + sum_k W1p[u][k] xs[tt][k]), tt < nt; act = tanh (layers 2) or identity (layers 1).
// ks lanes (a power of two <= 64, adjacent in the wave) share one output row u and split its K range.
__device__ void mh_stage1(const MhGeom& g, const float* __restrict__ blk, const float* xs, float* hs, int nt) {
  const int n1 = g.n1, dm = g.dm;
  int ks = 1;
  while (ks * 2 <= 64 && ks * 2 * n1 <= MH_THREADS) ks *= 2;
  const int j = threadIdx.x, grp = j / ks, sl = j % ks, ngrp = MH_THREADS / ks;
  const float* b1 = blk + (long long)n1 * dm;
  for (int u0 = 0; u0 < n1; u0 += ngrp) {      // uniform trip count: every lane reaches the shuffles
    const int u = u0 + grp;
    float acc[MH_TT];
#pragma unroll
    for (int tt = 0; tt < MH_TT; ++tt) acc[tt] = 0.f;
    if (u < n1) {
      const float* w = blk + (long long)u * dm;
      for (int k = sl; k < dm; k += ks) {
        const float wv = w[k];
#pragma unroll
        for (int tt = 0; tt < MH_TT; ++tt)
          if (tt < nt) acc[tt] = fmaf(wv, xs[tt * dm + k], acc[tt]);
      }
    }
    for (int o = ks >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int tt = 0; tt < MH_TT; ++tt) acc[tt] += __shfl_xor(acc[tt], o, 64);
    }
    if (u < n1 && sl == 0) {
#pragma unroll
      for (int tt = 0; tt < MH_TT; ++tt)
        if (tt < nt) {
          const float z = acc[tt] + b1[u];
          hs[tt * n1 + u] = g.layers == 2 ? tanhf(z) : z;
        }
    }
  }
}

// ls[tt][i] = b2[i] + sum_u W2[i][u] hs[tt][u], i < ds (layers 2)
__device__ void mh_stage2(const MhGeom& g, const float* __restrict__ blk, const float* hs, float* ls, int nt) {
  const float* W2 = blk + g.off2;
  const float* b2 = W2 + 64LL * g.ds;
  for (int i = threadIdx.x; i < g.ds; i += MH_THREADS) {
    float acc[MH_TT];
#pragma unroll
    for (int tt = 0; tt < MH_TT; ++tt) acc[tt] = 0.f;
    const float* w = W2 + 64LL * i;
    for (int u = 0; u < 64; ++u) {
      const float wv = w[u];
#pragma unroll
      for (int tt = 0; tt < MH_TT; ++tt)
        if (tt < nt) acc[tt] = fmaf(wv, hs[tt * 64 + u], acc[tt]);
    }
#pragma unroll
    for (int tt = 0; tt < MH_TT; ++tt)
      if (tt < nt) ls[tt * g.ds + i] = acc[tt] + b2[i];
  }
}

__device__ void mh_stage_x(const MhGeom& g, const float* __restrict__ x, int r, int h, int t0, int nt, float* xs) {
  for (int i = threadIdx.x; i < nt * g.dm; i += MH_THREADS) {
    const int tt = i / g.dm, k = i % g.dm;
    xs[i] = x[mh_xoff(g, r, t0 + tt, h, k)];
  }
}

// Online-softmax statistics of frames [t_lo, t_hi) of row r, head h, for every query, into acc (layout of aux:
// [R][Q][H][4][dm] = running max, sum exp, sum e x, sum e x^2).  An empty range leaves (-inf, 0, 0, 0).
__device__ void mh_fwd_range(const MhGeom& g, const float* __restrict__ x, const float* __restrict__ pack, int r, int h,
                             int t_lo, int t_hi, float* __restrict__ acc, float* lds) {
  const int dm = g.dm, TT = g.TT;
  float* xs = lds;
  float* hs = xs + TT * dm;
  float* ls = hs + TT * g.n1;
  const float* lg = g.layers == 2 ? ls : hs;
  if (t_lo >= t_hi)
    for (int q = 0; q < g.Q; ++q) {
      float* a = acc + (((long long)r * g.Q + q) * g.H + h) * 4 * dm;
      for (int k = threadIdx.x; k < dm; k += MH_THREADS) a[k] = -INFINITY, a[dm + k] = 0.f, a[2 * dm + k] = 0.f, a[3 * dm + k] = 0.f;
    }
  for (int t0 = t_lo; t0 < t_hi; t0 += TT) {
    const int nt = min(TT, t_hi - t0);
    __syncthreads();
    mh_stage_x(g, x, r, h, t0, nt, xs);
    __syncthreads();
    for (int q = 0; q < g.Q; ++q) {
      const float* blk = pack + (long long)(q * g.H + h) * g.P1;
      mh_stage1(g, blk, xs, hs, nt);
      __syncthreads();
      if (g.layers == 2) {
        mh_stage2(g, blk, hs, ls, nt);
        __syncthreads();
      }
      float* a = acc + (((long long)r * g.Q + q) * g.H + h) * 4 * dm;
      for (int k = threadIdx.x; k < dm; k += MH_THREADS) {       // this thread owns feature k in every tile
        const int row = g.ds == 1 ? 0 : mh_native(g, k);
        float m = t0 == t_lo ? -INFINITY : a[k];
        float s = t0 == t_lo ? 0.f : a[dm + k], sx = t0 == t_lo ? 0.f : a[2 * dm + k], sxx = t0 == t_lo ? 0.f : a[3 * dm + k];
        float mt = m;
        for (int tt = 0; tt < nt; ++tt) mt = fmaxf(mt, lg[tt * g.ds + row]);
        const float sc = expf(m - mt);
        s *= sc, sx *= sc, sxx *= sc;
        for (int tt = 0; tt < nt; ++tt) {
          const float e = expf(lg[tt * g.ds + row] - mt), xv = xs[tt * dm + k];
          s += e;
          sx = fmaf(e, xv, sx);
          sxx = fmaf(e * xv, xv, sxx);
        }
        a[k] = mt, a[dm + k] = s, a[2 * dm + k] = sx, a[3 * dm + k] = sxx;
      }
      __syncthreads();
    }
  }
}

// (max logit, sum exp, sum e x, sum e x^2) of one (r, q, h) -> aux (max logit, sum exp, mean, raw var) and out
// (mean || sqrt(max(var, floor)), native order)
__device__ __forceinline__ void mh_finish(const MhGeom& g, int r, int q, int h, int k, float m, float s, float sx,
                                          float sxx, float* __restrict__ out, float* __restrict__ aux) {
  const int dm = g.dm;
  float* a = aux + (((long long)r * g.Q + q) * g.H + h) * 4 * dm;
  float* o = out + (long long)r * g.Q * g.H * 2 * dm + (long long)(q * g.H + h) * 2 * dm;
  const float mean = sx / s, var = sxx / s - mean * mean;
  a[k] = m, a[dm + k] = s, a[2 * dm + k] = mean, a[3 * dm + k] = var;
  const int nk = mh_native(g, k);
  o[nk] = mean;
  o[dm + nk] = sqrtf(fmaxf(var, MH_FLOOR));
}

__global__ __launch_bounds__(MH_THREADS) void mhastp_fwd_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ pack, MhGeom g,
                                                                float* __restrict__ out, float* __restrict__ aux) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int r = blockIdx.x / g.H, h = blockIdx.x % g.H, dm = g.dm;
  mh_fwd_range(g, x, pack, r, h, 0, g.T, aux, lds);
  // aux becomes (max logit, sum exp, mean, raw var); std = sqrt(max(var, floor)) goes to out
  for (int q = 0; q < g.Q; ++q) {
    const float* a = aux + (((long long)r * g.Q + q) * g.H + h) * 4 * dm;
    for (int k = threadIdx.x; k < dm; k += MH_THREADS)
      mh_finish(g, r, q, h, k, a[k], a[dm + k], a[2 * dm + k], a[3 * dm + k], out, aux);
  }
}

// Split over T: workgroup (r*H + h, s) takes frames [s*tchunk, min(T, (s+1)*tchunk)) and leaves its partial state in
// part[s] (each [R][Q][H][4][dm], the layout of aux).
__global__ __launch_bounds__(MH_THREADS) void mhastp_fwd_part_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ pack, MhGeom g,
                                                                     float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int r = blockIdx.x / g.H, h = blockIdx.x % g.H, s = blockIdx.y;
  const int t_lo = min(g.T, s * g.tchunk), t_hi = min(g.T, t_lo + g.tchunk);
  mh_fwd_range(g, x, pack, r, h, t_lo, t_hi, part + (long long)s * g.R * g.Q * g.H * 4 * g.dm, lds);
}

// Merge of the nsplit partial states of one (r, q, h) per workgroup, splits in ascending order (the same bits every run)
__global__ __launch_bounds__(MH_THREADS) void mhastp_merge_kernel(const float* __restrict__ part, MhGeom g, int nsplit,
                                                                  float* __restrict__ out, float* __restrict__ aux) {
  const int h = blockIdx.x % g.H, q = (blockIdx.x / g.H) % g.Q, r = blockIdx.x / (g.H * g.Q), dm = g.dm;
  const long long stride = (long long)g.R * g.Q * g.H * 4 * dm;
  const float* p0 = part + (((long long)r * g.Q + q) * g.H + h) * 4 * dm;
  for (int k = threadIdx.x; k < dm; k += MH_THREADS) {
    float m = -INFINITY;
    for (int s = 0; s < nsplit; ++s) m = fmaxf(m, p0[s * stride + k]);
    float se = 0.f, sx = 0.f, sxx = 0.f;
    for (int s = 0; s < nsplit; ++s) {
      const float* p = p0 + s * stride;
      if (p[dm + k] == 0.f) continue;                 // an empty split (max -inf)
      const float sc = expf(p[k] - m);
      se = fmaf(p[dm + k], sc, se);
      sx = fmaf(p[2 * dm + k], sc, sx);
      sxx = fmaf(p[3 * dm + k], sc, sxx);
    }
    mh_finish(g, r, q, h, k, m, se, sx, sxx, out, aux);
  }
}

// Backward of one (r, h) for all queries, frames [y*tchunk, min(T, (y+1)*tchunk)) of split y = blockIdx.y.  Every
// tile is independent given aux: with g_t = dmean x_t + dvar (x_t^2 - 2 mean x_t), the softmax's cross-frame term is
// sum_t alpha_t g_t = dmean mean + dvar (E[x^2] - 2 mean^2) = dmean mean + dvar (var - mean^2), so a T split needs no
// pass over the other frames.  work (NULL: no weight gradients) = dz [M][Q*H][n1], then (layers 2)
// h [M][Q*H][64] and d(logit) [M][Q*H][ds], M = R*T, row m = r*T + t.
__global__ __launch_bounds__(MH_THREADS) void mhastp_bwd_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ pack,
                                                                const float* __restrict__ aux,
                                                                const float* __restrict__ dout, MhGeom g,
                                                                float* __restrict__ dx, float* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int r = blockIdx.x / g.H, h = blockIdx.x % g.H, dm = g.dm, TT = g.TT, QH = g.Q * g.H;
  float* xs = lds;
  float* dxs = xs + TT * dm;
  float* hs = dxs + TT * dm;
  float* ls = hs + TT * g.n1;
  float* red = ls + (g.layers == 2 ? TT * g.ds : 0);            // [4 waves][MH_TT]
  float* lg = g.layers == 2 ? ls : hs;
  const long long M = (long long)g.R * g.T;
  float* wz = work;
  float* wh = work ? work + M * QH * g.n1 : nullptr;
  float* wl = work ? wh + M * QH * 64 : nullptr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t_lo = min(g.T, (int)blockIdx.y * g.tchunk), t_hi = min(g.T, t_lo + g.tchunk);
  for (int t0 = t_lo; t0 < t_hi; t0 += TT) {
    const int nt = min(TT, t_hi - t0);
    __syncthreads();
    mh_stage_x(g, x, r, h, t0, nt, xs);
    for (int i = threadIdx.x; i < nt * dm; i += MH_THREADS) dxs[i] = 0.f;
    __syncthreads();
    for (int q = 0; q < g.Q; ++q) {
      const int qh = q * g.H + h;
      const float* blk = pack + (long long)qh * g.P1;
      mh_stage1(g, blk, xs, hs, nt);
      __syncthreads();
      if (g.layers == 2) {
        mh_stage2(g, blk, hs, ls, nt);
        __syncthreads();
      }
      const float* a = aux + (((long long)r * g.Q + q) * g.H + h) * 4 * dm;
      const float* go = dout + (long long)r * QH * 2 * dm + (long long)qh * 2 * dm;
      // per feature: alpha, the direct part of dx, and d(logit) = alpha (g_t - sum_t' alpha g_t') with
      // g_t = dmean x_t + dvar (x_t^2 - 2 mean x_t); dvar = 0 where the clamp holds
      float part[MH_TT];
#pragma unroll
      for (int tt = 0; tt < MH_TT; ++tt) part[tt] = 0.f;
      for (int k = threadIdx.x; k < dm; k += MH_THREADS) {
        const int nk = mh_native(g, k), row = g.ds == 1 ? 0 : nk;
        const float m = a[k], s = a[dm + k], mean = a[2 * dm + k], var = a[3 * dm + k];
        const float dmean = go[nk], dstd = go[dm + nk];
        const float dvar = var >= MH_FLOOR ? 0.5f * dstd / sqrtf(var) : 0.f;
        const float c = dmean * mean + dvar * (var - mean * mean);
        const float inv_s = 1.f / s;
#pragma unroll
        for (int tt = 0; tt < MH_TT; ++tt)
          if (tt < nt) {
            const float xv = xs[tt * dm + k];
            const float al = expf(lg[tt * g.ds + row] - m) * inv_s;
            const float gt = xv * (dmean + dvar * (xv - 2.f * mean));
            dxs[tt * dm + k] += al * (dmean + 2.f * dvar * (xv - mean));
            if (g.ds == 1) {
              part[tt] += gt - c;
            } else {
              lg[tt * g.ds + row] = al * (gt - c);                  // this thread alone reads and writes row nk
            }
          }
      }
      if (g.ds == 1) {       // one logit per frame: d(logit_t) = alpha_t sum_k (g_tk - c_k)
#pragma unroll
        for (int tt = 0; tt < MH_TT; ++tt) {
          const float v = ws_wave_sum(part[tt]);
          if (lane == 0) red[wave * MH_TT + tt] = v;
        }
        __syncthreads();
        if (threadIdx.x < nt) {
          const int tt = threadIdx.x;
          const float tot = (red[tt] + red[MH_TT + tt]) + (red[2 * MH_TT + tt] + red[3 * MH_TT + tt]);
          lg[tt] = expf(lg[tt] - a[0]) / a[dm] * tot;
        }
      }
      __syncthreads();
      // lg holds d(logit) [tt][ds] (row order native)
      if (g.layers == 2) {
        for (int p = threadIdx.x; p < nt * 64; p += MH_THREADS) {     // dz = (W2^T dl) (1 - h^2), in place of h
          const int tt = p >> 6, u = p & 63;
          const float* W2 = blk + g.off2;
          float acc = 0.f;
          for (int i = 0; i < g.ds; ++i) acc = fmaf(W2[64LL * i + u], lg[tt * g.ds + i], acc);
          const float hv = hs[tt * 64 + u];
          if (work) wh[((long long)(r * g.T + t0 + tt) * QH + qh) * 64 + u] = hv;
          hs[tt * 64 + u] = acc * (1.f - hv * hv);
        }
        if (work)
          for (int i = threadIdx.x; i < nt * g.ds; i += MH_THREADS) {
            const int tt = i / g.ds, row = i % g.ds;
            wl[((long long)(r * g.T + t0 + tt) * QH + qh) * g.ds + row] = lg[i];
          }
        __syncthreads();
      }
      // hs = d(first layer output) [tt][n1]
      if (work)
        for (int i = threadIdx.x; i < nt * g.n1; i += MH_THREADS) {
          const int tt = i / g.n1, u = i % g.n1;
          wz[((long long)(r * g.T + t0 + tt) * QH + qh) * g.n1 + u] = hs[i];
        }
      for (int k = threadIdx.x; k < dm; k += MH_THREADS) {            // dx += W1^T dz
        float acc[MH_TT];
#pragma unroll
        for (int tt = 0; tt < MH_TT; ++tt) acc[tt] = 0.f;
        for (int u = 0; u < g.n1; ++u) {
          const float wv = blk[(long long)u * dm + k];
#pragma unroll
          for (int tt = 0; tt < MH_TT; ++tt)
            if (tt < nt) acc[tt] = fmaf(wv, hs[tt * g.n1 + u], acc[tt]);
        }
#pragma unroll
        for (int tt = 0; tt < MH_TT; ++tt)
          if (tt < nt) dxs[tt * dm + k] += acc[tt];
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < nt * dm; i += MH_THREADS) {
      const int tt = i / dm, k = i % dm;
      dx[mh_xoff(g, r, t0 + tt, h, k)] = dxs[i];
    }
  }
}

// Partial weight gradients of split blockIdx.y (rows [y * rps, min(M, (y + 1) * rps))), one 64 x 64 output tile per
// workgroup: out[a][b] = sum_m G[m][a] A[m][b], column b == nb the bias (A = 1).
//   part A: G = dz (or d(logit) for layers 1) [n1], A = x in kernel order [dm]  -> W1 (upstream column order), b1
//   part B: G = d(logit) [ds],                 A = tanh output [64]            -> W2, b2
__global__ __launch_bounds__(MH_THREADS) void mhastp_wgrad_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ work, MhGeom g,
                                                                  int rps, int tiles_ab, int tiles_bb, int tiles_qh,
                                                                  float* __restrict__ slab) {
  __shared__ float Gs[16][64];
  __shared__ float As[16][64];
  const int QH = g.Q * g.H, qh = blockIdx.x / tiles_qh, h = qh % g.H;
  int t = blockIdx.x % tiles_qh;
  const int tiles_a = ((g.n1 + 63) / 64) * tiles_ab;
  const bool partA = t < tiles_a;
  int na, nb, a0, b0;
  if (partA) {
    na = g.n1, nb = g.dm, a0 = (t / tiles_ab) * 64, b0 = (t % tiles_ab) * 64;
  } else {
    t -= tiles_a;
    na = g.ds, nb = 64, a0 = (t / tiles_bb) * 64, b0 = (t % tiles_bb) * 64;
  }
  const long long M = (long long)g.R * g.T;
  const float* wz = work;
  const float* wh = work + M * QH * g.n1;
  const float* wl = wh + M * QH * 64;
  const long long m0 = (long long)blockIdx.y * rps, m1 = min(M, m0 + rps);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;
  for (long long mm = m0; mm < m1; mm += 16) {
    for (int i = threadIdx.x; i < 16 * 64; i += MH_THREADS) {
      const int mi = i >> 6, c = i & 63;
      const long long m = mm + mi;
      const int a = a0 + c, b = b0 + c;
      float gv = 0.f, av = 0.f;
      if (m < m1) {
        if (a < na) gv = partA ? wz[(m * QH + qh) * g.n1 + a] : wl[(m * QH + qh) * g.ds + a];
        if (b < nb)
          av = partA ? x[mh_xoff(g, (int)(m / g.T), (int)(m % g.T), h, b)] : wh[(m * QH + qh) * 64 + b];
        else if (b == nb)
          av = 1.f;
      }
      Gs[mi][c] = gv;
      As[mi][c] = av;
    }
    __syncthreads();
#pragma unroll
    for (int mi = 0; mi < 16; ++mi) {
      float gv[4], av[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) gv[i] = Gs[mi][ty + 16 * i], av[i] = As[mi][tx + 16 * i];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[i][k] = fmaf(gv[i], av[k], acc[i][k]);
    }
    __syncthreads();
  }
  float* o = slab + (long long)blockIdx.y * QH * g.P1 + (long long)qh * g.P1;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int a = a0 + ty + 16 * i, b = b0 + tx + 16 * k;
      if (a >= na || b > nb) continue;
      long long idx;
      if (partA) idx = b < nb ? (long long)a * g.dm + mh_native(g, b) : (long long)g.n1 * g.dm + a;
      else idx = g.off2 + (b < nb ? 64LL * a + b : 64LL * g.ds + a);
      o[idx] = acc[i][k];
    }
}

// one (query, head) block of the pack; W1's columns to the kernel order k = f*Ch + c
__global__ void mhastp_pack_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                   const float* __restrict__ w2, const float* __restrict__ b2, MhGeom g,
                                   float* __restrict__ blk) {
  const long long nw1 = (long long)g.n1 * g.dm;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < g.P1; i += (long long)gridDim.x * blockDim.x) {
    float v;
    if (i < nw1) {
      const int u = (int)(i / g.dm), k = (int)(i % g.dm);
      v = w1[(long long)u * g.dm + (k % g.Ch) * g.F + k / g.Ch];
    } else if (i < nw1 + g.n1) {
      v = b1[i - nw1];
    } else if (i < g.off2 + 64LL * g.ds) {
      v = w2[i - g.off2];
    } else {
      v = b2[i - g.off2 - 64LL * g.ds];
    }
    blk[i] = v;
  }
}

// geometry + argument checks shared by the entry points; TT from the LDS budget (bwd: x and dx tiles)
bool mh_geom(int R, int F, int T, int C, int Q, int H, int layers, int ds, bool bwd, MhGeom* g) {
  if (R <= 0 || F <= 0 || T <= 0 || C <= 0 || Q <= 0 || H <= 0 || C % H != 0) return false;
  if (layers != 1 && layers != 2) return false;
  g->R = R, g->F = F, g->T = T, g->C = C, g->Q = Q, g->H = H, g->layers = layers, g->ds = ds;
  g->Ch = C / H;
  g->dm = g->Ch * F;
  if (ds != 1 && ds != g->dm) return false;
  g->n1 = mh_n1(layers, ds);
  g->P1 = (int)mh_block_floats(layers, ds, g->dm);
  g->off2 = g->n1 * g->dm + g->n1;
  const int per_tt = (bwd ? 2 : 1) * g->dm + g->n1 + (layers == 2 ? ds : 0);
  const int fixed = bwd ? 4 * MH_TT : 0;
  g->TT = min(MH_TT, (MH_LDS_FLOATS - fixed) / per_tt);
  g->tchunk = T;
  return g->TT >= 1;
}

size_t mh_lds_bytes(const MhGeom& g, bool bwd) {
  const int per_tt = (bwd ? 2 : 1) * g.dm + g.n1 + (g.layers == 2 ? g.ds : 0);
  return sizeof(float) * ((size_t)g.TT * per_tt + (bwd ? 4 * MH_TT : 0));
}

}  // namespace

extern "C" int ws_mhastp_sizes(int R, int T, int Q, int H, int layers, int ds, int d_model, long long* block_floats,
                               long long* work_floats) {
  WS_REQUIRE(R >= 0 && T >= 0 && Q >= 0 && H >= 0 && d_model > 0 && (layers == 1 || layers == 2) &&
                 (ds == 1 || ds == d_model),
             "ws_mhastp_sizes: bad args (layers %d, ds %d, d_model %d)", layers, ds, d_model);
  if (block_floats) *block_floats = mh_block_floats(layers, ds, d_model);
  if (work_floats) *work_floats = (long long)R * T * Q * H * (mh_n1(layers, ds) + (layers == 2 ? 64 + ds : 0));
  return WS_OK;
}

extern "C" int ws_mhastp_pack(const float* w1, const float* b1, const float* w2, const float* b2, int F, int Ch,
                              int layers, int ds, float* blk, void* stream) {
  MhGeom g{};
  WS_REQUIRE(w1 && b1 && blk && F > 0 && Ch > 0 && (layers == 1 || layers == 2) &&
                 (layers == 1 || (w2 && b2)) && (ds == 1 || ds == Ch * F),
             "ws_mhastp_pack: bad args (layers %d, ds %d, F %d, Ch %d)", layers, ds, F, Ch);
  g.F = F, g.Ch = Ch, g.dm = Ch * F, g.layers = layers, g.ds = ds, g.n1 = mh_n1(layers, ds);
  g.P1 = (int)mh_block_floats(layers, ds, g.dm);
  g.off2 = g.n1 * g.dm + g.n1;
  const int blocks = min(1024, (g.P1 + 255) / 256);
  hipLaunchKernelGGL(mhastp_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, b2, g, blk);
  return ws_check_launch("ws_mhastp_pack");
}

extern "C" int ws_mhastp_fwd(const float* x, const float* pack, int R, int F, int T, int C, int Q, int H, int layers,
                             int ds, float* out, float* aux, void* stream) {
  MhGeom g{};
  WS_REQUIRE(x && pack && out && aux, "ws_mhastp_fwd: null pointer");
  WS_REQUIRE(mh_geom(R, F, T, C, Q, H, layers, ds, false, &g),
             "ws_mhastp_fwd: unsupported geometry (R %d F %d T %d C %d Q %d H %d layers %d ds %d): H must divide C, "
             "layers 1 or 2, ds 1 or C/H*F, one frame of the head within the LDS budget",
             R, F, T, C, Q, H, layers, ds);
  WS_REQUIRE((long long)R * H < (1LL << 31), "ws_mhastp_fwd: grid too large");
  hipLaunchKernelGGL(mhastp_fwd_kernel, dim3(R * H), dim3(MH_THREADS), mh_lds_bytes(g, false), (hipStream_t)stream, x,
                     pack, g, out, aux);
  return ws_check_launch("ws_mhastp_fwd");
}

namespace {

// the backward behind ws_mhastp_bwd (tsplit 1) and ws_mhastp_bwd_split: dx over a (R*H, tsplit) grid, then the weight
// gradients from the workspace as before
int mh_bwd(const char* who, const float* x, const float* pack, const float* aux, const float* dout, int R, int F, int T,
           int C, int Q, int H, int layers, int ds, int tsplit, float* dx, float* work, float* slab, int nsplit,
           float* dpack, void* stream) {
  MhGeom g{};
  WS_REQUIRE(x && pack && aux && dout && dx, "%s: null pointer", who);
  WS_REQUIRE(mh_geom(R, F, T, C, Q, H, layers, ds, true, &g),
             "%s: unsupported geometry (R %d F %d T %d C %d Q %d H %d layers %d ds %d)", who, R, F, T, C, Q, H, layers,
             ds);
  WS_REQUIRE(tsplit >= 1 && tsplit <= T && tsplit <= 65535, "%s: %d T splits for %d frames", who, tsplit, T);
  WS_REQUIRE((long long)R * H < (1LL << 31), "%s: grid too large", who);
  const bool wgrad = dpack != nullptr;
  WS_REQUIRE(!wgrad || (work && nsplit > 0 && (nsplit == 1 || slab)),
             "%s: weight gradients need work, nsplit > 0 and (nsplit > 1) a slab", who);
  g.tchunk = (T + tsplit - 1) / tsplit;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mhastp_bwd_kernel, dim3(R * H, tsplit), dim3(MH_THREADS), mh_lds_bytes(g, true), s, x, pack, aux,
                     dout, g, dx, wgrad ? work : nullptr);
  int rc = ws_check_launch(who);
  if (rc != WS_OK || !wgrad) return rc;
  const long long M = (long long)R * T;
  const int rps = (int)((M + nsplit - 1) / nsplit);
  const int tiles_ab = (g.dm + 1 + 63) / 64, tiles_bb = layers == 2 ? (64 + 1 + 63) / 64 : 0;
  const int tiles_qh = ((g.n1 + 63) / 64) * tiles_ab + (layers == 2 ? ((ds + 63) / 64) * tiles_bb : 0);
  float* dst = nsplit == 1 ? dpack : slab;
  hipLaunchKernelGGL(mhastp_wgrad_kernel, dim3(Q * H * tiles_qh, nsplit), dim3(MH_THREADS), 0, s, x, work, g, rps,
                     tiles_ab, tiles_bb, tiles_qh, dst);
  if ((rc = ws_check_launch("ws_mhastp_bwd(wgrad)")) != WS_OK || nsplit == 1) return rc;
  const long long P = (long long)Q * H * g.P1;
  return ws_reduce_slabs(slab, nsplit, P, P, dpack, 0, 0, stream);
}

// T splits of the split grid: about two workgroups per CU over the R*H (row, head) pairs, at least MH_TT frames each
int mh_tsplit(int R, int T, int H, int cus) {
  const long long rh = (long long)R * H, want = 2LL * (cus > 0 ? cus : 1);
  const int tiles = (T + MH_TT - 1) / MH_TT;
  long long n = (want + rh - 1) / rh;
  if (n > tiles) n = tiles;
  if (n < 1) n = 1;
  const int per = (int)((tiles + n - 1) / n);           // tiles per split; no split is left empty
  return (tiles + per - 1) / per;
}

}  // namespace

extern "C" int ws_mhastp_bwd(const float* x, const float* pack, const float* aux, const float* dout, int R, int F,
                             int T, int C, int Q, int H, int layers, int ds, float* dx, float* work, float* slab,
                             int nsplit, float* dpack, void* stream) {
  return mh_bwd("ws_mhastp_bwd", x, pack, aux, dout, R, F, T, C, Q, H, layers, ds, 1, dx, work, slab, nsplit, dpack,
                stream);
}

extern "C" int ws_mhastp_split_sizes(int R, int F, int T, int C, int Q, int H, int cus, int* tsplit,
                                     long long* part_floats) {
  WS_REQUIRE(R > 0 && F > 0 && T > 0 && C > 0 && Q > 0 && H > 0 && C % H == 0 && cus > 0 && tsplit,
             "ws_mhastp_split_sizes: bad args (R %d F %d T %d C %d Q %d H %d cus %d)", R, F, T, C, Q, H, cus);
  *tsplit = mh_tsplit(R, T, H, cus);
  if (part_floats) *part_floats = (long long)*tsplit * R * Q * H * 4 * (C / H) * F;
  return WS_OK;
}

extern "C" int ws_mhastp_fwd_split(const float* x, const float* pack, int R, int F, int T, int C, int Q, int H,
                                   int layers, int ds, int tsplit, float* part, float* out, float* aux, void* stream) {
  MhGeom g{};
  WS_REQUIRE(x && pack && part && out && aux, "ws_mhastp_fwd_split: null pointer");
  WS_REQUIRE(mh_geom(R, F, T, C, Q, H, layers, ds, false, &g),
             "ws_mhastp_fwd_split: unsupported geometry (R %d F %d T %d C %d Q %d H %d layers %d ds %d): H must divide "
             "C, layers 1 or 2, ds 1 or C/H*F, one frame of the head within the LDS budget",
             R, F, T, C, Q, H, layers, ds);
  WS_REQUIRE(tsplit >= 1 && tsplit <= T && tsplit <= 65535, "ws_mhastp_fwd_split: %d T splits for %d frames", tsplit, T);
  WS_REQUIRE((long long)R * Q * H < (1LL << 31), "ws_mhastp_fwd_split: grid too large");
  g.tchunk = (T + tsplit - 1) / tsplit;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mhastp_fwd_part_kernel, dim3(R * H, tsplit), dim3(MH_THREADS), mh_lds_bytes(g, false), s, x, pack,
                     g, part);
  int rc = ws_check_launch("ws_mhastp_fwd_split");
  if (rc != WS_OK) return rc;
  hipLaunchKernelGGL(mhastp_merge_kernel, dim3(R * Q * H), dim3(MH_THREADS), 0, s, part, g, tsplit, out, aux);
  return ws_check_launch("ws_mhastp_fwd_split(merge)");
}

extern "C" int ws_mhastp_bwd_split(const float* x, const float* pack, const float* aux, const float* dout, int R,
                                   int F, int T, int C, int Q, int H, int layers, int ds, int tsplit, float* dx,
                                   float* work, float* slab, int nsplit, float* dpack, void* stream) {
  return mh_bwd("ws_mhastp_bwd_split", x, pack, aux, dout, R, F, T, C, Q, H, layers, ds, tsplit, dx, work, slab, nsplit,
                dpack, stream);
}
