// dW_proj^T = h^T dout on the fp16 hi plane of h (H2P storage, include/wesep_hip.h) -- ws_gemm_tnb_h16.
//
//   slab[split][g][a] = sum_{b in split} sum_i G[(b,i)][g_off + g] * A0[(b,i)][a0_off + a]        (128 A columns)
//   aslab[split][a]   = sum A0[(b,i)][a0_off + a]                                                 (db_proj)
//
// G: fp16 elements in BLH(g_width) -- the hi plane the forward recurrences write: its 8-byte cells ARE the operand, nothing is
// converted.  A0: the incoming gradient as BLS pairs in BL(a0_width) (ws_gemm_p2b's A_bl): each bf16 term is multiplied by the
// power of two S = ws_dgates_scale(*amax) and converted to fp16, round to nearest -- exact wherever the scaled term is a normal
// fp16 number (a bf16 term has 8 significant bits), off by at most 2^-25 / S in fp16's subnormals -- so a product is TWO MFMAs
// (G A_hi + G A_lo) on v_mfma_f32_32x32x16_f16 where ws_gemm_tnb runs three bf16 ones on the pair format of h, and a workgroup
// loads 24 KB per block instead of 32.  The slab leaves multiplied by 1 / S (exact).  Precondition (the caller's, like
// |A| <= 1020 of ws_gemm_tnb): |A0| S <= 65504, i.e. max |dout| < 2^7 max |d(hcat)| -- dout and d(hcat) = dout Wp are the same
// gradient one Linear apart.  Where it does not hold (a projection weight of nearly zero: amax = 0 gives S = 1) the lifted term
// is +-Inf, the slab and with it dW_proj non-finite, and the optimizer's guard skips the step: loud, as for d(gates) itself.
//
// Tiling as gemm_tnb_kernel<1, .> of gemm_blk.hip: one workgroup (8 waves, 2 x 4) owns 128 G columns x the 128 A columns over
// the blocks of its split, the contraction index is the slot; [column][slot] LDS images with row stride TB_LD, double-buffered,
// one barrier per block.  Global loads run PF blocks ahead of the MFMAs.
#include "common.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

#define TB_LD 40   // fp16 elements per LDS row (32 slots + 8: conflict-free 16-byte fragment reads)
#define PF 4       // blocks in flight per thread

__global__ __launch_bounds__(512, 2) void gemm_tnb_h16_kernel(const ws_gemm_tnb_args p) {
  constexpr int PLANE = 128 * TB_LD;                               // fp16 elements of one [128 columns][slot] image
  __shared__ __attribute__((aligned(16))) _Float16 lds[2][3 * PLANE];   // [buf][G | A hi | A lo]   60 KB
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;
  const int gt = blockIdx.y, split = blockIdx.x;
  const int b_begin = split * p.blocks_per_split;
  const int b_end = min(p.nblk, b_begin + p.blocks_per_split);
  const int nb = b_end - b_begin;          // <= 0: a split behind nblk writes zeros
  const float S = ws_dgates_scale(*p.amax), inv_s = ws_dgates_scale_inv(*p.amax);

  // G piece: quad qg of the tile, slots 2 sp and 2 sp + 1 (two adjacent 8-byte cells)
  const int qg = tid >> 4, sp = tid & 15;
  const unsigned short* gsrc = reinterpret_cast<const unsigned short*>(p.G) + ((long long)((p.g_off + gt * 128) / 4 + qg) * 32 + 2 * sp) * 4;
  const long long gstep = 32LL * p.g_width;    // 2-byte elements per block
  // A piece: quad qg again, slots as .. as + 1 (two 16-byte cells of BLS words)
  const int as = 2 * sp;
  const float* asrc = p.A0 + (long long)(p.a0_off / 4 + qg) * 128 + as * 4;
  const long long astep = 32LL * p.a0_width;   // floats per block

  u32x4 gq[PF], aq[PF][2];
  auto load_block = [&](int b, int k) {
    aq[k][0] = *reinterpret_cast<const u32x4*>(asrc + (long long)b * astep);
    aq[k][1] = *reinterpret_cast<const u32x4*>(asrc + (long long)b * astep + 4);
    gq[k] = *reinterpret_cast<const u32x4*>(gsrc + (long long)b * gstep);
  };
  float asum[4] = {0.f, 0.f, 0.f, 0.f};
  // registers of ring slot k -> LDS image `img`: every column's two slots as one 32-bit word
  auto store_block = [&](int k, _Float16* img) {
    const u32x4 d = gq[k];
    unsigned* gw = reinterpret_cast<unsigned*>(img + (4 * qg) * TB_LD + 2 * sp);
    gw[0 * TB_LD / 2] = __builtin_amdgcn_perm(d[2], d[0], WS_SEL_LO16);
    gw[1 * TB_LD / 2] = __builtin_amdgcn_perm(d[2], d[0], WS_SEL_HI16);
    gw[2 * TB_LD / 2] = __builtin_amdgcn_perm(d[3], d[1], WS_SEL_LO16);
    gw[3 * TB_LD / 2] = __builtin_amdgcn_perm(d[3], d[1], WS_SEL_HI16);
    unsigned* ah = reinterpret_cast<unsigned*>(img + PLANE + (4 * qg) * TB_LD + as);
    unsigned* al = reinterpret_cast<unsigned*>(img + 2 * PLANE + (4 * qg) * TB_LD + as);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned e0 = aq[k][0][c], e1 = aq[k][1][c];
      const float h0 = __uint_as_float(e0 & 0xffff0000u) * S, h1 = __uint_as_float(e1 & 0xffff0000u) * S;
      const float l0 = __uint_as_float(e0 << 16) * S, l1 = __uint_as_float(e1 << 16) * S;
      // round to nearest, not cvt_pkrtz: a lifted term beyond fp16's range has to become +-Inf (and reach the optimizer's guard
      // through the slab, like an overflowing d(gates) of WS_GATES_H2F), where round-toward-zero would clip it to 65504 in silence
      const f16x2 ph = {(_Float16)h0, (_Float16)h1}, pl = {(_Float16)l0, (_Float16)l1};
      ah[c * TB_LD / 2] = __builtin_bit_cast(unsigned, ph);
      al[c * TB_LD / 2] = __builtin_bit_cast(unsigned, pl);
      asum[c] += (h0 + l0) + (h1 + l1);     // (scaled; hi + lo is the stored value exactly)
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[e][r] = 0.f;

  if (nb > 0) {
#pragma unroll
    for (int k = 0; k < PF; ++k) load_block(b_begin + min(k, nb - 1), k);
    store_block(0, lds[0]);
  }
  __syncthreads();
  for (int ib = 0; ib < nb; ib += PF) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int i = ib + k;
      if (i < nb) {   // uniform; only the tail skips
        // ring slot k held block i (converted one iteration ago, or in the prologue) -> block i + PF
        load_block(b_begin + min(i + PF, nb - 1), k);
        const _Float16* img = lds[k & 1];
#pragma unroll
        for (int ks = 0; ks < 32; ks += 16) {
          const int ra = (wn * 32 + l31) * TB_LD + ks + 8 * half;
          const f16x8 a_hi = *reinterpret_cast<const f16x8*>(img + PLANE + ra);
          const f16x8 a_lo = *reinterpret_cast<const f16x8*>(img + 2 * PLANE + ra);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const f16x8 g = *reinterpret_cast<const f16x8*>(img + (wm * 64 + e * 32 + l31) * TB_LD + ks + 8 * half);
            acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_f16(g, a_hi, acc[e], 0, 0, 0);
            acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_f16(g, a_lo, acc[e], 0, 0, 0);
          }
        }
        if (i + 1 < nb) store_block((k + 1) % PF, lds[(k + 1) & 1]);   // block i + 1 -> the other image
        __syncthreads();  // image k & 1 fully read, the other fully written
      }
    }
  }

  float* out = p.slab + (long long)split * p.slab_stride;
  const int acol = wn * 32 + l31;
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int grow = gt * 128 + wm * 64 + e * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      out[(long long)grow * 128 + acol] = acc[e][r] * inv_s;
    }
  if (p.aslab && gt == 0) {   // column sums of A0: over the 16 slot pairs of a quad = the lanes sharing tid >> 4
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float t = asum[c];
      t += __shfl_xor(t, 1, 64);
      t += __shfl_xor(t, 2, 64);
      t += __shfl_xor(t, 4, 64);
      t += __shfl_xor(t, 8, 64);
      if (sp == 0) p.aslab[(long long)split * p.aslab_stride + 4 * qg + c] = t * inv_s;
    }
  }
}

extern "C" int ws_gemm_tnb_h16(const ws_gemm_tnb_args* a, void* stream) {
  WS_REQUIRE(a && a->G && a->A0 && a->slab && a->amax, "ws_gemm_tnb_h16: null pointer (G, A0, slab and amax are required)");
  WS_REQUIRE(a->g_cols > 0 && a->g_cols % 128 == 0 && a->g_off >= 0 && a->g_off % 4 == 0 && a->g_width % 4 == 0 &&
                 a->g_off + a->g_cols <= a->g_width,
             "ws_gemm_tnb_h16: G column range");
  WS_REQUIRE(a->a0_cols == 128 && a->a0_off >= 0 && a->a0_off % 4 == 0 && a->a0_width % 4 == 0 && a->a0_off + 128 <= a->a0_width &&
                 a->a0_shift == 0,
             "ws_gemm_tnb_h16: A0 must contribute exactly 128 unshifted columns");
  WS_REQUIRE(!a->A1 && a->a1_cols == 0 && !a->bslab && a->g_fmt == 0 && a->a_fmt == 0,
             "ws_gemm_tnb_h16: no A1, no bslab; g_fmt / a_fmt stay 0 (the formats are this entry point's own)");
  WS_REQUIRE(a->nblk > 0 && a->L > 0 && a->nblk % a->L == 0 && a->nsplit > 0 && a->blocks_per_split > 0 &&
                 (long long)a->nsplit * a->blocks_per_split >= a->nblk,
             "ws_gemm_tnb_h16: bad block split");
  WS_REQUIRE(a->slab_stride >= (long long)a->g_cols * 128 && (!a->aslab || a->aslab_stride >= 128), "ws_gemm_tnb_h16: slab strides");
  hipStream_t s = (hipStream_t)stream;
  ws_prof_begin(WS_PROF_GEMM_TN, s);
  hipLaunchKernelGGL(gemm_tnb_h16_kernel, dim3(a->nsplit, a->g_cols / 128), dim3(512), 0, s, *a);
  ws_prof_end(WS_PROF_GEMM_TN, s);
  return ws_check_launch("ws_gemm_tnb_h16");
}
