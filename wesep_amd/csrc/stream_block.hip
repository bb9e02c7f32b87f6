// A whole causal cLN block of a streamed Conv-TasNet on one chunk, in ONE launch: the first 1x1 product, PReLU, cLN, the
// depthwise convolution on its ring, PReLU, cLN, the second 1x1 product and the residual (wesep_hip.h:
// ws_tcn_block_stream_fwd / ws_tcn_block_stream_rows_fwd; DESIGN section 7, "The whole block").
//
// One workgroup of TB_NT threads per ROW.  It walks the row's frames in tiles of TB_TF, in order:
//   x tile -> LDS;  c = W1 x: thread i owns the channels i, i + NT, ... of all TF frames (TF accumulators in registers), the
//   weights pass through LDS in [256 rows][KC columns] pieces, stored transposed, so one pass over W1 serves the tile's
//   frames;  PReLU, statistics (per frame: per-thread partial over its channels in ascending order, wave sum, the four wave
//   sums in ascending order), xn -> LDS and the ring;  the taps: a frame of this tile from LDS, anything earlier -- an
//   earlier chunk's frame or an earlier tile's of this launch, which THIS workgroup wrote before a barrier -- from the
//   ring;  PReLU, statistics, normalise in LDS;  out = x + (W2 yn + b2) the same way.
// Every dot product of a frame is ONE accumulator, started at 0 and advanced by fmaf in ascending k: what a frame gives
// depends on nothing but its own operands -- not on its place in the tile, the chunk, or the launch's rectangle.  Every
// multiply-add that reaches an output is an explicit fmaf, so the solo and the rows instantiation cannot contract
// differently.  No atomics, no workgroup waits on another, no packed FP32, no scratch.
#include "common.h"
#include "tasnet_dw.h"

namespace {

constexpr int TB_NT = 256;          // threads of a workgroup (a constant: the statistics' order depends on it)
constexpr int TB_TF = 8;            // frames of a tile
constexpr int TB_KC = 16;           // weight columns staged per step
constexpr int TB_WP = TB_NT + 4;    // pitch of a staged weight column: the transposing stores of a wave hit 64 banks

struct TbArgs {
  const float *W1, *b1, *a1, *g1, *be1, *wd, *bd, *a2, *g2, *be2, *W2, *b2;
  int B, H, ldw1, P, dil, cap;
  float eps;
};

__host__ __device__ constexpr size_t tb_lds_floats(int B, int H) {
  return (size_t)TB_TF * B + (size_t)TB_TF * H + (size_t)TB_KC * TB_WP + 4 * TB_TF;
}

// acc[t] = sum_k W[g0 + tid][k] * in[t][k], ascending k, for the TF frames of the LDS tile in [TF][K].  Rows past nrows
// and columns past K are staged as zeros (the threads that own no row run on them, so every barrier is met by all).
__device__ __forceinline__ void tb_gemm_group(const float* __restrict__ W, int ldw, int nrows, int K, int g0,
                                              const float* in, float* ws, float (&acc)[TB_TF]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int t = 0; t < TB_TF; ++t) acc[t] = 0.f;
  for (int k0 = 0; k0 < K; k0 += TB_KC) {
#pragma unroll
    for (int u = tid; u < TB_NT * (TB_KC / 4); u += TB_NT) {
      const int row = u >> 2, q = u & 3, r = g0 + row, kq = k0 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < nrows && kq < K) v = *reinterpret_cast<const f32x4*>(W + (long long)r * ldw + kq);
#pragma unroll
      for (int j = 0; j < 4; ++j) ws[(4 * q + j) * TB_WP + row] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TB_KC; kk += 4) {
      if (k0 + kk < K) {
        const float w0 = ws[kk * TB_WP + tid], w1 = ws[(kk + 1) * TB_WP + tid], w2 = ws[(kk + 2) * TB_WP + tid],
                    w3 = ws[(kk + 3) * TB_WP + tid];
#pragma unroll
        for (int t = 0; t < TB_TF; ++t) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(in + (size_t)t * K + k0 + kk);
          float a = acc[t];
          a = __builtin_fmaf(w0, xv[0], a);
          a = __builtin_fmaf(w1, xv[1], a);
          a = __builtin_fmaf(w2, xv[2], a);
          a = __builtin_fmaf(w3, xv[3], a);
          acc[t] = a;
        }
      }
    }
    __syncthreads();
  }
}

// s[t] <- the workgroup's sum of s[t], every thread gets it: wave sum, then the four wave sums in ascending order
__device__ __forceinline__ void tb_sum_frames(float (&s)[TB_TF], float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < TB_TF; ++t) s[t] = ws_wave_sum(s[t]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < TB_TF; ++t) red[w * TB_TF + t] = s[t];
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < TB_TF; ++t) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < TB_NT / 64; ++i) a += red[i * TB_TF + t];
    s[t] = a;
  }
}

// PReLU, two-pass statistics and the affine normalisation of the tile ys [TF][H] in place; thread i touches the channels
// i, i + NT, ... only.  With rr given, the nv valid frames' results also go to their ring slots (own0 + t) mod cap.
__device__ __forceinline__ void tb_prelu_norm(float* ys, int H, float slope, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float eps, float* red, float* rr, int own0,
                                              int cap, int nv) {
  const int tid = threadIdx.x;
  float s[TB_TF], q[TB_TF];
#pragma unroll
  for (int t = 0; t < TB_TF; ++t) s[t] = 0.f;
  for (int h = tid; h < H; h += TB_NT) {
#pragma unroll
    for (int t = 0; t < TB_TF; ++t) {
      float v = ys[(size_t)t * H + h];
      v = v > 0.f ? v : slope * v;
      ys[(size_t)t * H + h] = v;
      s[t] += v;
    }
  }
  tb_sum_frames(s, red);
#pragma unroll
  for (int t = 0; t < TB_TF; ++t) s[t] = s[t] / (float)H, q[t] = 0.f;
  for (int h = tid; h < H; h += TB_NT) {
#pragma unroll
    for (int t = 0; t < TB_TF; ++t) {
      const float d = ys[(size_t)t * H + h] - s[t];
      q[t] = __builtin_fmaf(d, d, q[t]);
    }
  }
  tb_sum_frames(q, red);
#pragma unroll
  for (int t = 0; t < TB_TF; ++t) q[t] = 1.f / sqrtf(q[t] / (float)H + eps);
  for (int h = tid; h < H; h += TB_NT) {
    const float gm = gamma[h], bt = beta[h];
#pragma unroll
    for (int t = 0; t < TB_TF; ++t) {
      const float v = __builtin_fmaf((ys[(size_t)t * H + h] - s[t]) * q[t], gm, bt);
      ys[(size_t)t * H + h] = v;
      if (rr && t < nv) {
        int sl = own0 + t;
        sl = sl >= cap ? sl - cap : sl;
        sl = sl >= cap ? sl - cap : sl;
        rr[(long long)sl * H + h] = v;
      }
    }
  }
}

// The n frames of one row, by one workgroup.  xr / outr: the row's [n..][B] input and output, rbr: its bias row or NULL,
// rr: its ring [cap][H], t0 / base: the absolute index of its first frame and t0 % cap.  Shared by the two kernels.
__device__ __forceinline__ void tb_row(const TbArgs& k, const float* __restrict__ xr, const float* __restrict__ rbr, int n,
                                       long long t0, int base, float* rr, float* __restrict__ outr) {
  extern __shared__ __attribute__((aligned(16))) float tb_lds[];
  const int B = k.B, H = k.H, P = k.P, cap = k.cap, tid = threadIdx.x;
  float* xs = tb_lds;
  float* ys = xs + (size_t)TB_TF * B;
  float* ws = ys + (size_t)TB_TF * H;
  float* red = ws + TB_KC * TB_WP;
  const float sl1 = k.a1[0], sl2 = k.a2[0];
  float acc[TB_TF];
  for (int tile0 = 0; tile0 < n; tile0 += TB_TF) {
    const int nv = n - tile0 < TB_TF ? n - tile0 : TB_TF;
    const int b4 = B >> 2;
    for (int u = tid; u < TB_TF * b4; u += TB_NT) {
      const int t = u / b4, c = (u - t * b4) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};                      // frames past the row's last one: zeros, x is not read there
      if (t < nv) v = *reinterpret_cast<const f32x4*>(xr + (long long)(tile0 + t) * B + c);
      *reinterpret_cast<f32x4*>(xs + (size_t)t * B + c) = v;
    }
    // (the first barrier inside tb_gemm_group stands between these stores and the products' reads)
    for (int g0 = 0; g0 < H; g0 += TB_NT) {
      tb_gemm_group(k.W1, k.ldw1, H, B, g0, xs, ws, acc);
      const int h = g0 + tid;
      if (h < H) {
        const float bias = rbr ? rbr[h] : k.b1[h];
#pragma unroll
        for (int t = 0; t < TB_TF; ++t) ys[(size_t)t * H + h] = acc[t] + bias;
      }
    }
    int own0 = base + tile0;                               // < 2 cap
    tb_prelu_norm(ys, H, sl1, k.g1, k.be1, k.eps, red, rr, own0, cap, nv);
    // the taps, in place, latest frame first: z of frame t needs xn of frames <= t of the same channel, which this same
    // thread holds; frames before the tile come from the ring (written by an earlier launch, or by this workgroup in an
    // earlier tile: barriers lie between)
    for (int h = tid; h < H; h += TB_NT) {
      const float bdv = k.bd[h];
      for (int t = nv - 1; t >= 0; --t) {
        const long long a = t0 + tile0 + t;
        float z = bdv;
#pragma unroll 1
        for (int p = 0; p < P; ++p) {
          const int off = (P - 1 - p) * k.dil;
          if (a - off < 0) continue;                       // before the start: no term, no read
          float v;
          if (off <= t) {
            v = ys[(size_t)(t - off) * H + h];
          } else {
            long long sl = (long long)own0 + t - off;      // in (-cap, 2 cap)
            sl = sl < 0 ? sl + cap : sl;
            sl = sl >= cap ? sl - cap : sl;
            sl = sl >= cap ? sl - cap : sl;
            v = rr[sl * H + h];
          }
          z = __builtin_fmaf(k.wd[h * P + p], v, z);
        }
        ys[(size_t)t * H + h] = z;
      }
    }
    tb_prelu_norm(ys, H, sl2, k.g2, k.be2, k.eps, red, nullptr, 0, cap, nv);
    for (int g0 = 0; g0 < B; g0 += TB_NT) {
      tb_gemm_group(k.W2, H, B, H, g0, ys, ws, acc);
      const int b = g0 + tid;
      if (b < B) {
        const float bias = k.b2[b];
#pragma unroll
        for (int t = 0; t < TB_TF; ++t)
          if (t < nv) outr[(long long)(tile0 + t) * B + b] = xs[(size_t)t * B + b] + (acc[t] + bias);
      }
    }
    __syncthreads();                                       // the next tile overwrites xs and ys
  }
}

__global__ __launch_bounds__(TB_NT) void tcn_block_stream_kernel(TbArgs k, const float* __restrict__ x,
                                                                 const float* __restrict__ rb, int Tc, long long t0,
                                                                 int base, float* ring, float* __restrict__ out) {
  const long long r = blockIdx.x;
  tb_row(k, x + r * Tc * k.B, rb ? rb + r * k.H : nullptr, Tc, t0, base, ring + r * k.cap * k.H, out + r * Tc * k.B);
}

// Row i of the [A][Tc] rectangle: the stream in state slot slot[i], tc[i] valid frames from its frame t0[i] on.  The
// frames behind them get zeros; a row that names no slot (out of range, t0 < 0) or has no frame leaves after that, as one
// workgroup (the condition depends on blockIdx alone), and touches no state.
__global__ __launch_bounds__(TB_NT) void tcn_block_stream_rows_kernel(TbArgs k, const float* __restrict__ x,
                                                                      const float* __restrict__ rb, int Tc, int nslots,
                                                                      const int* __restrict__ slot,
                                                                      const long long* __restrict__ t0,
                                                                      const int* __restrict__ tc, float* ring,
                                                                      float* __restrict__ out) {
  const long long i = blockIdx.x;
  const int sl = slot[i];
  const long long first = t0[i];
  int n = tc[i];
  n = n > Tc ? Tc : n;
  if (n < 0 || sl < 0 || sl >= nslots || first < 0) n = 0;
  float* outr = out + i * Tc * k.B;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (long long u = (long long)n * (k.B >> 2) + threadIdx.x; u < (long long)Tc * (k.B >> 2); u += TB_NT)
    *reinterpret_cast<f32x4*>(outr + 4 * u) = z;
  if (n == 0) return;
  tb_row(k, x + i * Tc * k.B, rb ? rb + (long long)sl * k.H : nullptr, n, first, (int)(first % k.cap),
         ring + (long long)sl * k.cap * k.H, outr);
}

}  // namespace

#define TB_CHECK(who)                                                                                                            \
  WS_REQUIRE(x && W1 && a1 && gamma1 && beta1 && wd && bd && a2 && gamma2 && beta2 && W2 && b2 && ring && out,                   \
             who ": null pointer");                                                                                              \
  WS_REQUIRE((rb != nullptr) != (b1 != nullptr), who ": exactly one of rb (the row bias) and b1 must be given");                 \
  WS_REQUIRE(Tc > 0 && B > 0 && H > 0 && dil >= 1, who ": bad geometry (Tc=%d, B=%d, H=%d, dil=%d)", Tc, B, H, dil);             \
  WS_REQUIRE(B % 4 == 0 && H % 4 == 0 && ldw1 % 4 == 0, who ": B=%d, H=%d and ldw1=%d must be multiples of 4", B, H, ldw1);      \
  WS_REQUIRE(ldw1 >= B, who ": ldw1=%d is below B=%d", ldw1, B);                                                                 \
  WS_REQUIRE(H <= WS_TCN_BLOCK_MAXH && B <= WS_TCN_BLOCK_MAXB,                                                                   \
             who ": H=%d above %d or B=%d above %d (a tile of both is staged in LDS)", H, WS_TCN_BLOCK_MAXH, B,                  \
             WS_TCN_BLOCK_MAXB);                                                                                                 \
  WS_REQUIRE(P >= 1 && P <= TN_MAXP && (P & 1), who ": P=%d (odd P <= %d)", P, TN_MAXP);                                         \
  {                                                                                                                              \
    const long long need = (long long)(P - 1) * dil + Tc;                                                                        \
    WS_REQUIRE(cap >= need, who ": cap=%d is below (P - 1) * dil + Tc = %lld", cap, need);                                       \
  }

extern "C" int ws_tcn_block_stream_fwd(const float* x, const float* rb, const float* W1, int ldw1, const float* b1,
                                       const float* a1, const float* gamma1, const float* beta1, const float* wd,
                                       const float* bd, const float* a2, const float* gamma2, const float* beta2,
                                       const float* W2, const float* b2, int R, int Tc, int B, int H, int P, int dil,
                                       float eps, long long t0, int cap, float* ring, float* out, void* stream) {
  TB_CHECK("ws_tcn_block_stream_fwd");
  WS_REQUIRE(R > 0, "ws_tcn_block_stream_fwd: R=%d", R);
  WS_REQUIRE(t0 >= 0, "ws_tcn_block_stream_fwd: t0=%lld is negative", t0);
  WS_REQUIRE((long long)R * Tc < (1LL << 31), "ws_tcn_block_stream_fwd: R * Tc reaches 2^31");
  const long long n = (long long)R * Tc * B;
  WS_REQUIRE(out + n <= x || x + n <= out, "ws_tcn_block_stream_fwd: out overlaps x");
  const TbArgs k{W1, b1, a1, gamma1, beta1, wd, bd, a2, gamma2, beta2, W2, b2, B, H, ldw1, P, dil, cap, eps};
  hipLaunchKernelGGL(tcn_block_stream_kernel, dim3((unsigned)R), dim3(TB_NT), tb_lds_floats(B, H) * sizeof(float),
                     (hipStream_t)stream, k, x, rb, Tc, t0, (int)(t0 % cap), ring, out);
  return ws_check_launch("ws_tcn_block_stream_fwd");
}

extern "C" int ws_tcn_block_stream_rows_fwd(const float* x, const float* rb, const float* W1, int ldw1, const float* b1,
                                            const float* a1, const float* gamma1, const float* beta1, const float* wd,
                                            const float* bd, const float* a2, const float* gamma2, const float* beta2,
                                            const float* W2, const float* b2, int A, int Tc, int B, int H, int P, int dil,
                                            float eps, int nslots, const int* slot, const long long* t0, const int* tc,
                                            int cap, float* ring, float* out, void* stream) {
  TB_CHECK("ws_tcn_block_stream_rows_fwd");
  WS_REQUIRE(slot && t0 && tc, "ws_tcn_block_stream_rows_fwd: a NULL table (slot, t0 and tc are device arrays of A entries)");
  WS_REQUIRE(A > 0 && nslots > 0, "ws_tcn_block_stream_rows_fwd: bad tables (A=%d rows, nslots=%d)", A, nslots);
  WS_REQUIRE((long long)A * Tc < (1LL << 31), "ws_tcn_block_stream_rows_fwd: A * Tc reaches 2^31");
  const long long n = (long long)A * Tc * B;
  WS_REQUIRE(out + n <= x || x + n <= out, "ws_tcn_block_stream_rows_fwd: out overlaps x");
  const TbArgs k{W1, b1, a1, gamma1, beta1, wd, bd, a2, gamma2, beta2, W2, b2, B, H, ldw1, P, dil, cap, eps};
  hipLaunchKernelGGL(tcn_block_stream_rows_kernel, dim3((unsigned)A), dim3(TB_NT), tb_lds_floats(B, H) * sizeof(float),
                     (hipStream_t)stream, k, x, rb, Tc, nslots, slot, t0, tc, ring, out);
  return ws_check_launch("ws_tcn_block_stream_rows_fwd");
}
