// The depthwise dilated convolution's operand load and tap accumulation, shared by dwconv_fwd_kernel (tasnet.hip) and
// dwconv_stream_kernel (stream.hip): both build a result from the same expressions in the same order, so the chunked
// kernel's output is bit for bit the whole-sequence kernel's.
#pragma once
#include "common.h"

#define TN_MAXP 7

struct DwGeom {
  int R, Tp, C, P, dil, st_div, ctr;
};

// xn[row][c .. c+3] = (x - mean_s) * rstd_s * gamma + beta,  s = row / st_div
__device__ __forceinline__ f32x4 dw_xn(const float* __restrict__ x, const float* __restrict__ stats,
                                       const f32x4& gm, const f32x4& bt, const DwGeom& g, long long row, int c) {
  const long long s = row / g.st_div;
  const float mean = stats[2 * s], rstd = stats[2 * s + 1];
  return (*reinterpret_cast<const f32x4*>(x + row * g.C + c) - mean) * rstd * gm + bt;
}

// acc[j] += w[c + j][p] * v[j]: one tap; the callers walk the taps in ascending p
__device__ __forceinline__ void dw_tap(f32x4& acc, const float* __restrict__ w, int c, int P, int p, const f32x4& v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] += w[(c + j) * P + p] * v[j];
}
