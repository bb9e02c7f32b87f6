/* wesep_hip.h -- C ABI of libwesep_hip.so, the MI355X (gfx950) device library behind
 * wesep_amd's pBSRNN training path.
 *
 * wesep (the reference) has no FFI/operator interface of its own: its device boundary is
 * the set of stock ATen operators its Python modules call.  Each entry
 * point below replaces the ATen operator sequence of the reference lines it cites.  All
 * pointers are DEVICE pointers to fp32 unless stated; all tensors are caller-allocated;
 * `stream` is a hipStream_t (the caller's current stream); no call allocates, frees or
 * synchronises.  Return value: WS_OK or a negative WS_ERR_* code, message via
 * ws_last_error().  Host-side binding: wesep_amd/_lib.py (ctypes); see INTEGRATION.md.
 *
 * Activation layout ("Z layout"): [R][K][Tf][N] fp32, N = feature_dim contiguous, one
 * "position" p = (r*K + k)*Tf + t per row.  The reference's [B, K*N, T] / [B*K, N, T] /
 * [B*T, N, K] views (bsrnn.py:73-81) are strided row sets of this one buffer, so its two
 * permute().contiguous() copies per BSNet do not exist here.
 */
#ifndef WESEP_HIP_H_
#define WESEP_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define WS_ABI_VERSION 20
#define WS_OK 0
#define WS_ERR_INVALID (-1)
#define WS_ERR_LAUNCH (-2)

int ws_abi_version(void);
const char* ws_last_error(void);

/* ---- profiling: HIP-event brackets recorded on the launch stream ------------------- */
#define WS_PROF_LSTM_FWD 0
#define WS_PROF_LSTM_BWD 1
#define WS_PROF_GEMM_NT 2
#define WS_PROF_GEMM_TN 3
#define WS_PROF_NKINDS 4
int ws_prof_enable(int on);                       /* 1: bracket every launch of the kinds above */
int ws_prof_collect(int kind, double* total_ms, long long* launches); /* syncs the events; resets */
/* Test support: fills 60 KB of LDS per workgroup with `value` (NaN) on `stream` and keeps the workgroups alive for
 * `spins` LDS reads per thread; beside product kernels on another stream it exposes reads of LDS a kernel never wrote. */
int ws_debug_dirty_lds(float value, int nblocks, int spins, float* sink, void* stream);
/* Test support (ABI v15): holds `nblocks` compute units (112 KB of LDS each: no workgroup of the co-resident recurrences or
 * of the weight-gradient GEMM fits beside it) for `usec` microseconds of wall clock, or until *stop != 0 (optional
 * device word) -- a resident-collective-shaped occupant for the robustness tests.  Bounded: usec <= 2 000 000.        */
int ws_debug_occupy(int nblocks, int usec, const unsigned* stop, float* sink, void* stream);

/* ---- row addressing used by the GEMMs ---------------------------------------------------
 * row m of a matrix lives at  base + (m / div) * s1 + (m % div) * s2   (elements).       */

/* Per-group overrides for grouped (per-band) launches; array lives in DEVICE memory.      */
typedef struct ws_group_nt {
  const float* W;
  const float* bias;
  const float* gamma;
  const float* beta;
  long long a_off;    /* added to A                                     */
  long long c_off;    /* added to C (and to R, T)                       */
  long long st_base;  /* stat-index base                                */
  int K, N, ldw, pad_;
} ws_group_nt;

/* Implicit patch matrix (ABI v8): with conv.on != 0 the A operand of ws_gemm_nt / ws_gemm_tn (split-bf16 kernels
 * only) is the im2col matrix of a channels-last image x [R][H][W][C] that is never materialised -- A points to x and
 *   A[m][(ky*k + kx)*C + c],  m = (r*Ho + ho)*Wo + wo,  is
 *   mode 0 (convolution view):  x[r][ho*sh + ky*dil - p][wo*sw + kx*dil - p][c]
 *   mode 1 (transposed view):   x[r][(ho + p - ky*dil)/sh][(wo + p - kx*dil)/sw][c] where both divisions are exact,
 * and 0 outside the image (dil = 0 means 1).  A dilated Conv1d over [R][T][C] is the view H = 1, W = T, k x k taps,
 * p = dil * (k / 2): the rows ky != k/2 fall outside the one-row image (ECAPA-TDNN's Res2Net branches).  K = k*k*C, C % 4 == 0, a_div / a_s1 / a_s2 are ignored; mode 1 needs sh, sw in {1, 2}.
 * Conv2d = mode 0 on the input; its input gradient = mode 1 on the output gradient (K = k*k*Cout);
 * ConvTranspose2d = mode 1 on the input, its input gradient = mode 0 on the output gradient; the weight gradients
 * are ws_gemm_tn with the mode-0 view as A.  Replaces F.conv2d / F.conv_transpose2d of wesep/modules/dpccn/convs.py:28-110
 * and of the wespeaker ResNet (round 1 wrote the 9x larger patch matrix to HBM and read it back).          */
typedef struct ws_conv_view {
  int on, mode;
  int H, W, C;       /* the image A points to */
  int Ho, Wo;        /* patch grid (rows of the implicit matrix per image: Ho*Wo) */
  int k, sh, sw, p;
  int dil;           /* tap spacing; 0 = 1 */
  int ldp;           /* floats between consecutive pixels of the image (0 = C): the image may be the first C columns
                        of a wider channels-last tensor, e.g. the growing feature map of a dense block */
} ws_conv_view;

/* C[m][n] = epi( sum_k pro(A[m][k]) * W[n][k] )        (torch Linear / Conv1d(k=1) layout)
 *   pro : optional GroupNorm-on-load  a' = (a - mean[s]) * rstd[s] * gamma[k] + beta[k],
 *         s = (m / st_div1) * st_m1 + (m % st_div2) * st_m2 + st_base, stats = [S][2]
 *   epi : + bias[n]; act (0 none, 1 tanh, 2 ReLU); * (1 - T^2) if T (act 4: * (T > 0), the ReLU
 *         derivative from the saved output); + R if R                 (T, R addressed like C)
 * Replaces: F.group_norm + F.linear / Conv1d(k=1) (+tanh, +residual) at bsrnn.py:38-46,
 * 252-258, 271-282 and their autograd data-gradients.                                      */
typedef struct ws_gemm_nt_args {
  const float* A;
  const float* W;
  const float* bias;
  float* C;
  const float* R;
  const float* T;
  const float* stats;
  const float* gamma;
  const float* beta;
  const ws_group_nt* groups; /* NULL or device array [ngroups] */
  long long a_s1, a_s2, c_s1, c_s2, st_m1, st_m2, st_base;
  int a_div, c_div, st_div1, st_div2;
  int M, N, K, ldw;
  int act, ngroups, max_n, vec; /* max_n: max N over groups; vec bit0: A float4-loadable, bit1: W,
                                   bit2: split-bf16 (hi/lo, 3 MFMAs, fp32 accumulate) products;
                                   bit3 (round 6, with bits 0-2): W is stored TRANSPOSED, W'[n][k] = W[k * ldw + n] (per group:
                                   ws_group_nt.ldw >= N) -- C = A [M, K] x B [K, N] with B as it lies ("NN"): N % 4 == 0 and
                                   ldw % 4 == 0 (16-byte rows of W); no conv view, no norm-on-load                       */
  ws_conv_view conv;            /* conv.on: A is an implicit patch matrix (above), either mode */
} ws_gemm_nt_args;
int ws_gemm_nt(const ws_gemm_nt_args* a, void* stream);

typedef struct ws_group_tn {
  const float* gamma;
  const float* beta;
  long long g_off, a_off, st_base, out_off, bout_off;
  int Nn, Kk, pad0_, pad1_;
} ws_group_tn;

/* Weight gradients: slab[split][out_off + n*Kk + k] = sum_{m in split} G[m][n] * pro(A[m'][k]),
 * bslab[split][bout_off + n] = sum_m G[m][n]; the caller then sums the splits with
 * ws_reduce_slabs (deterministic, no atomics).  m' = m + shift_rows with the row zeroed
 * when the step index ((m / seq_div) % seq_len) +/- 1 leaves [0, seq_len) (h_{t-1} for dW_hh).
 * With a shift M is a whole number of sequences, M % (seq_div * seq_len) == 0 (checked: row m' then lies in [0, M)); it is
 * the OPERAND that is zeroed -- with norm-on-load too a zeroed row contributes 0, not beta -- and the stat index is taken
 * from m, not m'.  Split s covers the rows [s * rows_per_split, min(M, (s + 1) * rows_per_split)): rows_per_split is any
 * positive number (no multiple of the kernels' 32-row tile is needed), nsplit * rows_per_split >= M (checked), and a
 * trailing split whose range is empty writes zeros to its slab and bias slab.  Per group, ws_group_tn's gamma / beta /
 * st_base / out_off / bout_off / Nn / Kk REPLACE the argument's, g_off / a_off are added (ws_group_nt likewise: W / bias /
 * gamma / beta / st_base / K / N / ldw replace, a_off / c_off are added).
 * Replaces the autograd weight-gradient of the same reference lines as ws_gemm_nt.         */
typedef struct ws_gemm_tn_args {
  const float* G;
  const float* A;
  float* slab;
  float* bslab;              /* NULL: no bias gradient */
  const float* stats;
  const float* gamma;
  const float* beta;
  const ws_group_tn* groups; /* NULL or device array [ngroups] */
  long long g_s1, g_s2, a_s1, a_s2, st_m1, st_m2, st_base;
  long long slab_stride, bslab_stride, out_off, bout_off;
  int g_div, a_div, st_div1, st_div2;
  int M, Nn, Kk, rows_per_split, nsplit;
  int shift_rows, seq_div, seq_len;
  int ngroups, max_n, max_k, vec; /* vec bit0: A float4-loadable, bit2: split-bf16 products */
  ws_conv_view conv;              /* conv.on: A is an implicit patch matrix, mode 0 only (Kk = k*k*C) */
} ws_gemm_tn_args;
int ws_gemm_tn(const ws_gemm_tn_args* a, void* stream);

/* Weight gradient of a convolution with at most 32 output channels, one pass over the activation (conv_wgrad.hip):
 *   slab[split][n * Kk + kk] = sum_{m in split} G[m * ldg + n] * P[m][kk],   bslab[split][n] = sum_m G[m * ldg + n]
 * P = the mode-0 implicit patch matrix `conv` of the image X (Kk = k*k*C, C % 4 == 0, k <= 5; a workgroup owns up to 768
 * columns, wider matrices run one pass per 768-column chunk); a split is tiles_per_split tiles of 32 consecutive rows.  Same result as ws_gemm_tn with conv.on, which sends every 128-column
 * slice of P to another workgroup and so streams X k*k times; this one owns all of P's columns per tile.
 * Replaces autograd's weight gradient of F.conv2d / F.conv_transpose2d (wesep/modules/dpccn/convs.py:28-110).     */
typedef struct ws_conv_wgrad_args {
  const float* G;      /* [M][ldg] output gradient (conv2d) or the layer input (conv_transpose2d) */
  const float* X;      /* channels-last image the patch view is taken of */
  float* slab;
  float* bslab;        /* or NULL */
  long long ldg, slab_stride, bslab_stride;
  int M, Nn, nsplit, tiles_per_split;
  ws_conv_view conv;
} ws_conv_wgrad_args;
int ws_conv_wgrad(const ws_conv_wgrad_args* a, void* stream);

/* out[(i / w) * ldo + (i % w)] = sum_s slab[s * stride + i],  i < count                    */
int ws_reduce_slabs(const float* slab, int nsplit, long long stride, long long count,
                    float* out, int w, long long ldo, void* stream);

/* dst[c][r] = src[r][c]  (src [rows][cols] with leading dim lds)                           */
int ws_transpose(const float* src, int rows, int cols, long long lds, float* dst, void* stream);

/* ---- GroupNorm(1, C, eps) pieces (bsrnn.py:26,256,275; eps = FLT_EPSILON) ---------------
 * A "group" g covers L rows x W_g contiguous floats:
 *   base(g) = (g / gdiv) * gs1 + (g % gdiv) * gs2 (+ band_off[g % nbands]),  row stride rs,
 *   W_g = band_w ? band_w[g % nbands] : W;  means and variances are over the L * W_g floats of the group.
 * band_off, like band_w and gamma_tab, is indexed by the BAND of the group, g % nbands, whatever gdiv is (the band-split
 * norm passes gdiv == nbands; tests/norm_contract.py holds a geometry with gdiv != nbands to this reading).
 * Alignment: with band_w == NULL, band_off == NULL and W, rs, gs1, gs2 all multiples of 4 the kernels use 16-byte accesses;
 * every data pointer of the call (x, dxn, dxn2, res, dx, gamma and the gamma_tab entries) must then be 16-byte aligned.  Any
 * other geometry takes the scalar kernels, which need 4-byte alignment only.  ws_gn_bwd_fused2, ws_gn_bwd_apply_pg, ws_rowln_*
 * and ws_flat_stats* are vectorised always (x, dy, res, dx, y, gamma, beta 16-byte aligned).
 * W <= 128 binds ws_gn_param_grad and the band_w tables (its slabs are [..][2][W], 128 column threads) only: ws_group_stats,
 * ws_gn_bwd_reduce and ws_gn_bwd_apply take any W > 0 (Conv-TasNet's cLN: L = 1, W = C up to 3N).                */
typedef struct ws_groups_geom {
  const int* band_w;   /* device int[nbands], or NULL */
  const int* band_off; /* device int[nbands], or NULL; indexed by g % nbands */
  long long gs1, gs2, rs;
  int ngroups, gdiv, L, W; /* W: width (max width when band_w is given; then and for ws_gn_param_grad <= 128) */
  int nbands, pad_;        /* band of group g = g % nbands (per-band widths / offsets / gammas) */
} ws_groups_geom;
int ws_group_stats(const float* x, const ws_groups_geom* geo, float eps, float* stats, void* stream);
/* Ragged batches (inference): the statistics of group g cover its first glen[g / glen_div] rows only (device int table,
 * every entry in [1, L]; pBSRNN's three norms over time: g = r * K + band, glen = the rows' frame counts, glen_div = K).
 * The rows behind them are neither read nor counted, so nothing a caller left there (NaN included) reaches the result. */
int ws_group_stats_len(const float* x, const ws_groups_geom* geo, const int* glen, int glen_div, float eps, float* stats,
                       void* stream);

/* GroupNorm backward, two passes over the same geometry:
 *   pass 1  ab[g] = (mean_g(dxn*gamma), mean_g(dxn*gamma*xhat))
 *   pass 2  dx = rstd*(dxn*gamma - ab0 - xhat*ab1) (+ res)          (dx may alias dxn)
 * gamma_tab: NULL -> `gamma` (per column); else device table of per-band pointers indexed
 * by g % nbands.                                                                            */
int ws_gn_bwd_reduce(const float* x, const float* dxn, const float* stats, const float* gamma,
                     const float* const* gamma_tab, const ws_groups_geom* geo, float* ab,
                     void* stream);
int ws_gn_bwd_apply(const float* x, const float* dxn, const float* stats, const float* ab,
                    const float* gamma, const float* const* gamma_tab, const float* res,
                    const ws_groups_geom* geo, float* dx, void* stream);
/* dgamma/dbeta partials: slab[split][band][2][W] (row 0 dgamma, row 1 dbeta); band b owns groups {g : g % nbands == b}
 * (nbands = 1: every group).  Caller reduces the splits; which groups a split sums is the kernel's choice.  Every element
 * of the nsplit * nbands * 2 * W floats is written: columns [band_w[b], W) of band b hold zeros, and so does the whole slab
 * of a split that owns no group (nsplit above the groups of a band).  W <= 128, ngroups % nbands == 0.            */
int ws_gn_param_grad(const float* x, const float* dxn, const float* stats,
                     const ws_groups_geom* geo, int nsplit, float* slab, void* stream);

/* The three calls above in ONE pass for small single-band groups (the band view of ResRNN: L = K = 32 rows of
 * W = 128 floats per group; L even, <= 32): a wave owns a group in registers.
 *   dx = rstd * (dxn*gamma - mean(dxn*gamma) - xhat * mean(dxn*gamma*xhat)) (+ res);
 *   pslab[wg][0][c] / [wg][1][c] = this workgroup's share of dgamma[c] / dbeta[c] (sum over wg = the gradient).
 * Replaces autograd's GroupNorm backward of ResRNN.norm (bsrnn.py:26,39).                                  */
int ws_gn_bwd_fused(const float* x, const float* dxn, const float* stats, const float* gamma,
                    const float* res, const ws_groups_geom* geo, int nwg, float* dx, float* pslab,
                    float* pout, unsigned* counter, void* stream);
/* ABI v19: the same with d(xn) arriving as TWO addends (dxn + dxn2: the per-direction buffers ws_lstm_bwd writes through
 * ws_lstm_args.dxn); dxn2 = NULL is ws_gn_bwd_fused.                                                                */
int ws_gn_bwd_fused2(const float* x, const float* dxn, const float* dxn2, const float* stats, const float* gamma,
                     const float* res, const ws_groups_geom* geo, int nwg, float* dx, float* pslab,
                     float* pout, unsigned* counter, void* stream);
/* ABI v15: pout [2][128] (optional) = (dgamma, dbeta) summed over the workgroups BY the workgroups of the launch (the last
 * finisher of every 32 consecutive workgroups adds their shares up in index order, the last of those the group sums:
 * deterministic; no ws_reduce_slabs launch behind it).  pslab then needs nwg + ceil(nwg / 32) rows of [2][128]: the first
 * nwg rows are the workgroups' shares (all written; zeros where a workgroup owns no group), the ceil(nwg / 32) rows behind
 * them are SCRATCH of the two-level sum -- whatever they hold afterwards is no result.  Without pout exactly nwg rows are
 * written.  `counter`: 1 + ceil(nwg / 32) device words that are 0 at launch (the kernel leaves them at 0).
 * ws_gn_bwd_apply_pg: pass 2 of the two-pass form for single-band groups of 128-float rows (the time view of ResRNN.norm)
 * WITH the parameter sums: one partial [2][128] per group to pslab [ngroups][2][128], summed into pout [2][128] by the last
 * workgroup -- replaces ws_gn_bwd_apply + ws_gn_param_grad + ws_reduce_slabs there.  It sums in the same two levels: pslab
 * needs ngroups + ceil(ngroups / 32) rows (the extra ones scratch, as above) and `counter` 1 + ceil(ngroups / 32) zero words.  */
int ws_gn_bwd_apply_pg(const float* x, const float* dxn, const float* stats, const float* ab,
                       const float* gamma, const float* res, const ws_groups_geom* geo, float* dx,
                       float* pslab, float* pout, unsigned* counter, void* stream);

/* ---- speaker-fusion affine FOLDED into its consumers ------------------------------------------------------------------
 * The operand z' = z * (a0 + a[r]) + b[r] of ws_affine_fwd, formed in registers by the kernel that reads it instead of being
 * written by one launch and read back by five: r = position / rows_per_r selects the row of a / b ([R][128], device); position =
 * the row of the plain Z layout (element offset / 128).  a NULL means 0, b NULL means 0; both NULL switches the fold off (the
 * *_film entry points then ARE the plain ones).  One fused multiply-add per element (ws_film, csrc/common.h), the same one
 * ws_affine_fwd executes: a folded consumer sees the bits a materialised z' would hold.
 * New symbols only (WS_ABI_VERSION unchanged): no existing struct or signature moves.                                       */
typedef struct ws_film_desc {
  const float* a;
  const float* b;
  float a0;
  int rows_per_r;
} ws_film_desc;
/* ws_group_stats / ws_gn_bwd_reduce with x = film(z).  Vectorised geometries with single-band groups of 128-float rows whose
 * bases and strides are multiples of 128 floats (a row of a group = one position).                                          */
int ws_group_stats_film(const float* z, const ws_film_desc* film, const ws_groups_geom* geo, float eps, float* stats, void* stream);
int ws_gn_bwd_reduce_film(const float* z, const ws_film_desc* film, const float* dxn, const float* stats, const float* gamma,
                          const ws_groups_geom* geo, float* ab, void* stream);
/* ws_gn_bwd_apply_pg with xhat from film(z) and the affine's own backward on the way out: with r = the value
 * ws_gn_bwd_apply_pg writes (= d z'),  dx = r * (a0 + a[row]),  da[row][c] = sum r * z,  db[row][c] = sum r  over the positions
 * of the row.  Groups of contiguous rows that tile the positions (gdiv = 1, gs1 = L * 128, rs = 128, rows_per_r % L == 0: the
 * time view); every group leaves its partial [2][128] in fslab [ngroups][2][128] and the last workgroup of each ROW adds that
 * row's rows_per_r / L partials up in group order into da[row] / db[row] (deterministic).  fcounter: ngroups * L / rows_per_r
 * device words, zero at launch, left at zero.  da / db: NULL where a / b is NULL (multiply / additive fusion).  dgamma / dbeta
 * (pslab, pout, counter) exactly as ws_gn_bwd_apply_pg.                                                                     */
int ws_gn_bwd_apply_pg_film(const float* z, const ws_film_desc* film, const float* dxn, const float* stats, const float* ab,
                            const float* gamma, const float* res, const ws_groups_geom* geo, float* dx, float* pslab,
                            float* pout, unsigned* counter, float* fslab, float* da, float* db, unsigned* fcounter,
                            void* stream);

/* ---- bidirectional LSTM recurrence (nn.LSTM inside ResRNN, bsrnn.py:27-33,40) -----------
 * Sequence s, step t lives at row  p = (s / sq_div) * sq_s1 + (s % sq_div) * sq_s2 + t * step_rows.
 * gates [P][2][4H] holds x-projection + biases on entry (gate order i,f,g,o) and the
 * ACTIVATED gates on exit; cbuf/hcat [P][2H] (dir-major halves).  H = 256 only.            */
typedef struct ws_lstm_args {
  float* gates;
  float* cbuf;
  float* hcat;
  const float* dhcat;   /* bwd only: dL/dhcat [P][2H]                         */
  const float* wpack;   /* ws_lstm_pack output for this pass (fwd or bwd)     */
  long long sq_s1, sq_s2, step_rows;
  int nseq, sq_div, L, mode;   /* WS_LSTM_* below; must match the mode wpack was packed with */
  const unsigned* run_if;      /* split-bf16 ws_lstm_fwd and blocked-layout ws_lstm_bwd: optional device word; when given,
                                  the launch does nothing unless *run_if != 0 at kernel start (the predicated fall-back
                                  behind ws_lstm_fwd_cluster / ws_lstm_bwd_pair, see there)               */
  /* ABI v15, blocked-layout modes only: storage format of the saved recurrence state (WS_GATES_* below).  With
   * gfmt != 0 `gates` is a BLH(2 * 4H) buffer of 2-byte elements; the forward reads the fp32 pre-activations from
   * `gates_in` (BL(2 * 4H) fp32, not modified) instead of `gates`; the backward with WS_GATES_H2S writes d(gates)
   * to `dgates` (BL(2 * 4H), BLS elements) instead of in place; with WS_GATES_H2 `dgates` is optional: given, it
   * receives the bf16 d(gates) (BLH(2 * 4H)) and the saved gates stay intact -- what makes a BPTT launch repeatable
   * (the predicated fall-back behind ws_lstm_bwd_pair).                                                    */
  const float* gates_in;
  float* dgates;
  int gfmt;
  int rfmt;              /* ABI v18 (the former pad_: 0 = every earlier behaviour), ws_lstm_bwd with mode WS_LSTM_BF16X3_BLK and
                            WS_GATES_H2F only: 2 = the recurrent product d(h) = d(gates) W_hh on v_mfma_f32_32x32x16_f16 with the
                            STORED scaled-fp16 d(gates) as its one operand against W_hh as fp16 hi + scaled-FP8 lo of 256 w --
                            `wpack` from ws_lstm_pack_bwd_f8: two MFMAs per product instead of three, 96 instead of 128 KB of
                            weights streamed per wave and step (the arithmetic of ws_lstm_pair_args.rfmt = 2).  3 (ABI v20):
                            the same pack and stream with the lo term on v_mfma_scale_f32_32x32x64_f8f6f4 (the codes as A
                            operands of K = 64 against e4m3 of d(gates) / 256): four fp16 MFMAs + one FP8 MFMA per 64 gate
                            columns instead of eight fp16 MFMAs; not with `dxn`.
                            ws_lstm_fwd (which reads nothing else of this field), blocked-layout modes: WS_LSTM_FWD_H2P (16) =
                            hcat leaves as two fp16 planes (H2P, below) instead of BLS pairs -- what a launch that stands behind
                            ws_lstm_fwd_cluster2 with rfmt bit 1 has to leave.
                            Bit 5, WS_LSTM_C16 (32), or-ed to either (no new ABI version: 0 = every earlier behaviour): `cbuf` holds
                            the saved cell state as fp16 in BLH(2H) (C16, below).  WS_GATES_H2F and the blocked-layout modes only;
                            ws_lstm_fwd: together with WS_LSTM_FWD_H2P; ws_lstm_bwd: with rfmt 0 / 2 / 3, not with `dxn`        */
  const unsigned* amax;  /* WS_GATES_H2F, backward: max |dhcat| of this launch as float bits (see WS_GATES_H2F) */
  /* ABI v19 (three trailing fields, zero = every earlier behaviour), ws_lstm_bwd with rfmt = 2 only: d(normalised input) of
   * the ResRNN computed INSIDE the BPTT from the d(gates) image its recurrent product reads anyway (autograd's d(input) of
   * nn.LSTM, bsrnn.py:40) -- ws_gemm_b2p(a_fmt = 2) over d(gates), a 2.1 GB read per band-view layer at R = 32, is then not
   * launched.  dxn: plain rows [P][128] of direction 0, direction 1 at dxn + dxn_dir_stride floats; the row of (sequence,
   * step) is the ws_seqmap formula on this struct's sq_s1 / sq_s2 / sq_div / step_rows (which the blocked-layout modes
   * otherwise ignore); padded slots (sequence >= nseq) store nothing.  The consumer adds the two directions
   * (ws_gn_bwd_fused2).  wxpack: ws_lstm_pack_dx_f8 output.                                                           */
  float* dxn;
  long long dxn_dir_stride;
  const float* wxpack;
} ws_lstm_args;
/* Storage format of the saved activated gates and of d(pre-activation gates) on the blocked layout (ABI v15).
 * BLH(C): the BL(C) index formula with 2-byte elements -- element (b, slot i, column c) at 2-byte index
 * b*32*C + ((c >> 2)*32 + i)*4 + (c & 3); a lane's 4-column cell is 8 bytes, 32 lanes 256 contiguous bytes.
 *   WS_GATES_F32 (0): gates fp32 BL, d(gates) as BLS pairs IN PLACE (ABI <= 14: one 16E-byte buffer, three lives).
 *   WS_GATES_H2  (1): activated gates as unorm16 in BLH -- i, f, o in (0, 1): u = floor(x * 65535 + 0.5);
 *                     g in (-1, 1): u = floor((x + 1) * 32767.5 + 0.5) -- absolute error <= 7.7e-6 / 1.6e-5 where fp16
 *                     would leave 2.4e-4 near saturation; d(gates) IN PLACE as bf16 = the hi term of the split pair
 *                     (relative error 2^-9: consumers ws_gemm_b2p a_fmt = 1, ws_gemm_tnb g_fmt = 1).  Halves the
 *                     largest buffer of the step and every pass over it.
 *   WS_GATES_H2S (2): activated gates as in H2; d(gates) as BLS pairs (full split precision) to a separate
 *                     BL(2 * 4H) buffer.                                                                      */
#define WS_GATES_F32 0
#define WS_GATES_H2 1
#define WS_GATES_H2S 2
/*   WS_GATES_H2F (3): activated gates as in H2; d(gates) as SCALED fp16, in place or to `dgates` like H2:
 *                     stored = fp16(x * S),  S = ws_dgates_scale(*amax) = the power of two that puts max |d(hcat)| of the
 *                     launch -- the word `amax` (float bits), raised by the ws_gemm_p2b launch that produced d(hcat)
 *                     (ws_gemm_p2b_args.amax; the caller zeroes it) -- into [2^WS_DGATES_EXP, 2^(WS_DGATES_EXP + 1)):
 *                     2^7 of headroom for what the BPTT accumulates on top of d(hcat), and everything down to 2^-22 of
 *                     the largest keeps fp16's 11 bits -- 8x finer than bf16, at the same 2 bytes.  NOT clamped (ABI v17;
 *                     v15 / v16 stored fmed3(x * S, +-65504) and put the maximum into [2^10, 2^11)): a value beyond fp16's
 *                     range is stored as +-Inf, a NaN as NaN -- the consumers turn them into non-finite gradients, which
 *                     ws_grad_norms' guard catches: the optimizer step is skipped and counted instead of taken on
 *                     silently clipped gradients.  Consumers (ws_gemm_b2p a_fmt = 2, ws_gemm_tnb g_fmt = 2) read `amax`
 *                     themselves, feed the fp16 values to v_mfma_f32_32x32x16_f16 as they are and undo S (exact) in their
 *                     epilogues.  The default of the Python path.                                                     */
#define WS_GATES_H2F 3
#define WS_DGATES_EXP 8
#define WS_LSTM_F32_MT1 1 /* exact-fp32 MFMA, 16 sequences per workgroup                       */
#define WS_LSTM_F32_MT2 2 /* exact-fp32 MFMA, 32 sequences per workgroup                       */
#define WS_LSTM_BF16X3 3  /* split-bf16 (hi/lo, 3 bf16 MFMAs per product, fp32 accumulate), 32 */
#define WS_LSTM_BF16X3_BLK 4 /* as 3, but gates / cbuf / hcat / dhcat are in the blocked layout BL
                                (below): block b = tile * L + step, tile = 32 consecutive sequences;
                                the sq_* / step_rows fields are ignored.  hcat (fwd) and the d(gates)
                                left in `gates` (bwd) are written in split-bf16 storage BLS (below)  */
#define WS_LSTM_BF16X3_BLK16 5 /* as 4 with 16-sequence workgroups (two per tile): for views with too few
                                  sequences to fill the chip with 32-sequence workgroups         */
#define WS_LSTM_H 256
#define WS_LSTM_FWD_H2P 16 /* ws_lstm_args.rfmt of a forward launch: hcat as two fp16 planes */
#define WS_LSTM_C16 32     /* ws_lstm_args.rfmt / ws_lstm_pair_args.rfmt, or-ed in: cbuf as fp16 in BLH(2H) (C16, below) */
#define WS_LSTM_PACK_FLOATS (2 * 4 * WS_LSTM_H * WS_LSTM_H) /* per pass, both directions */
/* Packs weight_hh_l0 / _reverse [4H][H] into MFMA fragment order for the fwd and bwd pass
 * (fp32 for WS_LSTM_F32_*, bf16 hi/lo pairs for WS_LSTM_BF16X3; same byte size).           */
int ws_lstm_pack(const float* whh_f, const float* whh_r, float* pack_fwd, float* pack_bwd,
                 int mode, void* stream);
/* ABI v18: the BPTT pack of ws_lstm_args.rfmt = 2 (WS_LSTM_PACK_FLOATS floats like the others; per (direction, wave) region
 * of 128 KB: 16 chunks of 6 KB = four fp16 hi fragments of 256 w + four fragments of e4m3 codes of the remainder over the
 * scale of their group of 8 k-steps; the eight scales as floats at byte 96 K).  |w| < 255.                       */
int ws_lstm_pack_bwd_f8(const float* whh_f, const float* whh_r, float* pack_bwd, void* stream);
/* ABI v19: W_ih^T of both directions for ws_lstm_args.dxn -- wcat [2][4H][128] from ws_lstm_cat_ih; pack: WS_LSTM_DX_PACK_FLOATS
 * floats (16 regions of 48 KB + 64 B: fp16 hi fragments of 256 w for v_mfma_f32_16x16x32_f16, e4m3 codes of the remainder,
 * eight group scales).                                                                                              */
#define WS_LSTM_DX_PACK_FLOATS (16 * (48 * 1024 + 64) / 4)
int ws_lstm_pack_dx_f8(const float* wcat, float* pack, void* stream);
int ws_lstm_fwd(const ws_lstm_args* a, void* stream);
/* On exit gates holds dL/d(pre-activation gates).                                           */
int ws_lstm_bwd(const ws_lstm_args* a, void* stream);
/* Weight-stationary forward recurrence over clusters of 8 co-resident workgroups (blocked layout,
 * same gates / cbuf / hcat contract as WS_LSTM_BF16X3_BLK): W_hh stays in registers, h_t is exchanged
 * through `xchg` each step.  nseq % 64 == 0 and (nseq / 32) * 8 <= CUs of the device (checked).
 * xchg: (nseq / 32) * 128 KB scratch; flags: (nseq / 32) * 8 + 8 words (zeroed by the call on `stream`).
 * Residency of the whole grid is a precondition the launcher can only check against the CU count, not
 * against CUs held by other streams / processes, so every wait is bounded.  If one times out the outputs
 * are NaN-poisoned AND the launch's own timeout word  flags[(nseq / 32) * 8]  is set to 1 (it is 0 after a
 * clean launch); `status` (optional, sticky, never cleared by the library) is set to 1 as well.  Callers
 * enqueue the streaming kernels behind this launch with  run_if = &flags[(nseq / 32) * 8]  (ws_gemm_p2b to
 * rebuild the pre-activations, then ws_lstm_fwd): they cost an empty launch after a clean run and redo the
 * layer after a timeout, without a host round trip.                                               */
typedef struct ws_lstm_cluster_args {
  float* gates;
  float* cbuf;
  float* hcat;          /* fwd: output */
  const float* dhcat;   /* bwd: dL/dhcat, BL(512) */
  const float* whh_f;   /* weight_hh_l0          [4H][H] fp32 */
  const float* whh_r;   /* weight_hh_l0_reverse  [4H][H] fp32 */
  void* xchg;
  unsigned* flags;
  unsigned* status;
  int nseq, L;
  int dbg, gfmt;        /* dbg: probes / tests only: 1 skip the flag wait, 2 skip the gather, 4 skip the publish,
                           8 force a timeout in workgroup 0 at step 2 (exercises the fall-back).
                           gfmt (ABI v15, forward only; the cluster BPTT is WS_GATES_F32 only): WS_GATES_*; != 0: the
                           pre-activations come from gates_in (fp32 BL), `gates` receives unorm16 BLH      */
  const float* gates_in;
} ws_lstm_cluster_args;
int ws_lstm_fwd_cluster(const ws_lstm_cluster_args* a, void* stream);
/* Second-generation cluster forward (lstm_cluster2.hip; ABI v17): the same clusters, outputs and residency rules, for
 * WS_GATES_H2-style storage only (`gates` = unorm16 BLH(2 * 4H) out, cbuf fp32 BL, hcat BLS), with
 *   - the x-projection computed in the kernel from the normalised input as split pairs (xn: BL(128) of BLS elements, what
 *     ws_gemm_p2b writes as A_bl) against wcat [2][4H][128] (ws_lstm_cat_ih) and bcat [2][4H], the full three-term split-bf16
 *     product: no pre-activation buffer, no x-projection GEMM (bsrnn.py:39-40 fused into the recurrence);
 *   - the recurrent product on v_mfma_f32_32x32x16_f16: h_t as one fp16 operand, W_hh as fp16 hi / lo of 256 w;
 *   - a data-tagged hand-off (bit 14 of every fp16 h carries the step's tag; no flags).
 * xchg: (nseq / 32) * 64 KB scratch (filled by the call on `stream`); tword: the launch's time-out word (zeroed by the
 * call; 0 after a clean launch; callers enqueue ws_gemm_p2b + ws_lstm_fwd with run_if = tword behind the launch);
 * status: optional, sticky.  dbg (probes / tests): 1 skip the wait, 4 skip the publish, 8 force a time-out in workgroup 0
 * at step 2, 2048 cycle stamps into dbg_buf.                                                                                                       */
typedef struct ws_lstm_cluster2_args {
  float* gates;
  float* cbuf;
  float* hcat;
  const float* xn;
  const float* wcat;
  const float* bcat;
  const float* whh_f;
  const float* whh_r;
  void* xchg;
  unsigned* tword;
  unsigned* status;
  int nseq, L;
  int dbg, rfmt;        /* rfmt (ABI v20, the former pad_: 0 = every earlier behaviour): 1 = the lo term of the recurrent product on
                           v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 codes of 256 w - hi, one exponent per wave, against e4m3 of h): four
                           fp16 MFMAs + one FP8 MFMA per 64 columns instead of eight fp16 MFMAs.  Bit 1 (value 2): hcat leaves as
                           two fp16 planes (H2P, below) instead of BLS pairs.  Bit 2 (value 4): cbuf leaves as fp16 in BLH(2H)
                           (C16, below) instead of fp32 BL                                                               */
  float* dbg_buf;      /* dbg 2048: L * 2 * 8 64-bit cycle stamps of cluster 0 / member 0 (tools/r05_recur_probe.py) */
} ws_lstm_cluster2_args;
int ws_lstm_fwd_cluster2(const ws_lstm_cluster2_args* a, void* stream);
/* BPTT over the same clusters (reduce-scatter of partial dh each step): gates holds the activated
 * gates on entry and d(pre-activation gates) on exit; xchg: (nseq / 32) * 1 MB; flags / status as above
 * (in place on `gates`: there is no device-side fall-back, the caller checks the timeout word).  */
int ws_lstm_bwd_cluster(const ws_lstm_cluster_args* a, void* stream);
/* BPTT over PAIRS of workgroups (lstm_pair.hip; ABI v9): the two workgroups of a (32-sequence tile, direction) split
 * W_hh by gate rows -- each keeps the hi plane of its 512 rows in registers, streams only the lo plane, multiplies its
 * own d(gates) into a partial dh for all 256 units and hands the partner's half over (16 KB per step through `xchg`).
 * Same gates / cbuf / dhcat contract as ws_lstm_bwd(WS_LSTM_BF16X3_BLK): blocked layout, any nseq (padded slots),
 * gates = activated gates on entry, d(pre-activation gates) as BLS on exit -- replaces autograd through nn.LSTM for
 * the time view (bsrnn.py:38-46) on half of the chip's CUs.  wpack: ws_lstm_pack_pair output (WS_LSTM_PACK_FLOATS).
 * npair = 2 * ceil(nseq / 32); 2 * npair <= CUs of the device (checked).  xchg: npair * 64 KB scratch; flags:
 * npair * 8 + 8 words (zeroed by the call on `stream`).  Every wait is bounded: on a timeout d(gates) are NaN-poisoned,
 * flags[npair * 8] (0 after a clean launch) and *status (optional, sticky) are set to 1.  In place there is no
 * device-side repair; with `dgates` given (WS_GATES_H2 / H2S: the saved gates stay intact) callers enqueue the streaming
 * BPTT behind this launch with  run_if = &flags[npair * 8]  and the same `dgates`: an empty launch after a clean run,
 * the whole BPTT again after a timeout -- no NaN reaches a consumer, no host round trip (ABI v15).
 * dbg (probes / tests only): 1 skip the flag wait, 2 skip the exchange, 4 no weight reloads,
 * 8 force a timeout in pair 0 at step 2, 32 no wave priorities,
 * 64 full agent-scope release / acquire fences around the hand-off, 2048 (WS_GATES_F32 / H2F) cycle stamps of pair 0
 * into dbg_buf (tools/pair_diag.py --ts).                                                                         */
typedef struct ws_lstm_pair_args {
  float* gates;
  const float* cbuf;
  const float* dhcat;
  const float* wpack;
  void* xchg;
  unsigned* flags;
  unsigned* status;
  float* dbg_buf;       /* NULL, or npair * L * 2 * 2 * 4096 floats: per (pair, step, member) the partial it sent and
                           the partial it received (diagnosis only, tools/pair_diag.py)                       */
  int nseq, L;
  int dbg, gfmt;        /* gfmt (ABI v15): WS_GATES_*; H2 / H2F: unorm16 gates in, bf16 / scaled-fp16 d(gates) out -- to `dgates`
                           (BLH) when given, else in place; H2S: d(gates) as BLS pairs to `dgates`                     */
  float* dgates;
  const unsigned* amax; /* WS_GATES_H2F: max |dhcat| of this launch as float bits */
  int rfmt, pad_;       /* ABI v17: arithmetic of the recurrent product d(h) = d(gates) W_hh.  0: split-bf16, three
                           v_mfma_f32_32x32x16_bf16 per product (wpack from ws_lstm_pack_pair); 1 (WS_GATES_H2F only): the
                           STORED scaled-fp16 d(gates) as one operand of v_mfma_f32_32x32x16_f16 against W_hh as fp16 hi / lo
                           of 256 w (wpack from ws_lstm_pack_pair_f16): two MFMAs per product, what the kernel writes is
                           what its own recurrence and both consumers read.  2 (ABI v18; WS_GATES_H2F only): the same
                           product with the lo plane of W_hh as block-scaled FP8 (wpack from ws_lstm_pack_pair_f8): 16
                           instead of 22 significant bits of every weight, and the whole of W_hh stays on the compute
                           unit for the launch (hi plane in registers, lo plane in LDS) -- nothing of it is streamed.
                           3 (ABI v20; WS_GATES_H2F only): rfmt 2 with the lo term on v_mfma_scale_f32_32x32x64_f8f6f4 --
                           the same codes as A operands of K = 64 (wpack from ws_lstm_pack_pair_f8mx) against e4m3 of
                           d(gates) / 256 built in registers from the fp16 fragments: per 64 gate columns four fp16 MFMAs
                           + one FP8 MFMA at twice the rate instead of eight fp16 MFMAs.
                           Bit 5, WS_LSTM_C16 (32), or-ed to 2 or 3: `cbuf` holds fp16 cells in BLH(2H) (C16, below)   */
} ws_lstm_pair_args;
int ws_lstm_pack_pair(const float* whh_f, const float* whh_r, float* pack, void* stream);
/* ABI v17: the pack of rfmt = 1 (same size and unit order, fp16 hi / lo of 256 w; |w| < 255) */
int ws_lstm_pack_pair_f16(const float* whh_f, const float* whh_r, float* pack, void* stream);
/* ABI v18: the pack of rfmt = 2 (same size: 32 blocks of 64 KB, one per (direction, half, wave); per block the fp16 hi plane
 * of 256 w exactly as ws_lstm_pack_pair_f16 writes it (32 KB), then the lo plane as OCP e4m3 codes of (256 w - hi) / S, 8
 * bytes per lane and k-step (16 KB), then S as one float at byte 48 K; S = 2^(e - 20) for the block's max |256 w| in
 * [2^(e-1), 2^e): the largest possible remainder maps to 256 -- e4m3 has no saturation, it overflows to NaN above 448.
 * |w| < 255.) */
int ws_lstm_pack_pair_f8(const float* whh_f, const float* whh_r, float* pack, void* stream);
/* ABI v20: the pack of rfmt = 3 -- hi plane, codes and S of ws_lstm_pack_pair_f8; the codes as eight 2 KB operand fragments
 * (K = 64) per block: a lane's 32 bytes = its four 8-byte units of k-steps 4 kb .. 4 kb + 3, as two 16-byte pieces 1 KB apart;
 * the E8M0 byte of S as an int at byte 48 K + 4 */
int ws_lstm_pack_pair_f8mx(const float* whh_f, const float* whh_r, float* pack, void* stream);
int ws_lstm_bwd_pair(const ws_lstm_pair_args* a, void* stream);
/* wcat[2][4H][N] <- (w_ih_f, w_ih_r);  bcat[2][4H] <- b_ih + b_hh per direction             */
int ws_lstm_cat_ih(const float* wih_f, const float* wih_r, const float* bih_f, const float* bhh_f,
                   const float* bih_r, const float* bhh_r, int n_in, float* wcat, float* bcat,
                   void* stream);

/* ---- blocked layout BL and the GEMMs around the recurrence (bsrnn.py:38-46) ----------------
 * BL(C): a [rows][C] matrix whose rows are grouped in blocks of 32; block b = tile * L + step
 * holds the 32 consecutive sequences of an LSTM workgroup (`tile`) at one `step`;
 *   element (b, slot i, column c)  at  b*32*C + ((c >> 2)*32 + i)*4 + (c & 3).
 * Slots whose sequence index tile*32 + i >= nseq are padding: producers write zeros there.
 * Split-bf16 storage BLS (ABI v8): the BL buffers that are only ever consumed as MFMA operands -- hcat (h of the
 * blocked-layout recurrences), the d(pre-activation gates) that BPTT leaves in `gates`, and A_bl of ws_gemm_p2b
 * (normalised input / incoming gradient) -- hold each 4-byte element as the two terms of the split product:
 *   bits 31..16 = bf16 hi = bf16(x),  bits 15..0 = bf16 lo = bf16(x - hi),  value = hi + lo  (|error| <= 2^-17 |x|).
 * Producers have both terms at hand (they feed them to their own MFMAs); consumers (ws_gemm_b2p's A, all operands
 * of ws_gemm_tnb, xn of ws_lstm_fwd_fused) rebuild fragments with byte permutes instead of converting again -- the
 * products are bit-identical to splitting an fp32 copy.  Pre-activations / activated gates, cbuf and dhcat stay fp32.
 * Two-plane fp16 storage H2P of hcat (training with WS_GATES_H2F; selected per producer: ws_lstm_fused_args.hfmt bit 3,
 * ws_lstm_cluster2_args.rfmt bit 1, ws_lstm_args.rfmt = WS_LSTM_FWD_H2P): the same pointer and the same nblk * 32 * 2H * 4 bytes
 * hold two BLH(2H) planes of nblk blocks each -- first hi = fp16(h), then lo = fp16(h - hi), both round to nearest even; value =
 * hi + lo, >= 21 significant bits down to fp16's subnormal floor (|h| < 1).  The hi plane alone is the fp16 A operand of
 * ws_gemm_tnb (a_fmt = 1) and the G operand of ws_gemm_tnb_h16; ws_gemm_b2p reads both planes (a_fmt = 4).
 * fp16 storage C16 of cbuf (training with WS_GATES_H2F; selected per launch: ws_lstm_fused_args.hfmt bit 4,
 * ws_lstm_cluster2_args.rfmt bit 2, ws_lstm_args.rfmt / ws_lstm_pair_args.rfmt bit 5 = WS_LSTM_C16): cbuf is ONE BLH(2H) plane of nblk
 * blocks -- nblk * 32 * 2H * 2 bytes, the layout of H2P's hi plane -- holding fp16(c), round to nearest even, of the fp32 cell
 * the recurrence itself continues from; padded slots hold what the fp32 format holds there.  The BPTT kernels are the only
 * readers: tanh(c_t) in d(o) and d(c), and the factor c_{t-1} of d(f).  |c_t| <= t, so sequences of up to 32768 steps cannot
 * overflow fp16 (the callers' limit).  A fall-back launch behind ws_lstm_fwd_cluster2 / ws_lstm_bwd_pair must name the format
 * of the launch it stands behind.
 * ws_seqmap maps a slot to its position (row) in the plain Z-layout tensors:
 *   pos = (seq / sq_div) * sq_s1 + (seq % sq_div) * sq_s2 + step * step_rows.              */
typedef struct ws_seqmap {
  long long sq_s1, sq_s2, step_rows;
  int nseq, sq_div, L;
  int nvalid;   /* ABI v15: 0 = every sequence < nseq maps to rows; else sequences >= nvalid are PADDING (zeros on the way
                   into BL, dropped on the way out): nseq then only fixes the number of 32-sequence tiles -- strided maps
                   (TF-GridNet's inter-frame path in place, no transposed copy) whose sequence count the cluster
                   recurrence wants rounded up to a multiple of 64                                                  */
} ws_seqmap;

/* out (bf16 pairs, N*K*4 bytes) <- W'[n][k] = trans ? W[k*ldw + n] : W[n*ldw + k], split into
 * bf16 hi/lo and ordered for ws_gemm_p2b (order 0) or ws_gemm_b2p (order 1): hi = bf16(w), lo = bf16(w - hi), both round
 * to nearest even, in 16-byte units of 8 consecutive k for the MFMA lane that loads them --
 *   element j of unit u*64 + lane = part(W'[32*nt + (lane & 31)][16*ks + 8*(lane >> 5) + j]),  part 0 = hi, 1 = lo,
 *   u = (nt*(K/16) + ks)*2 + part (order 0)   or   u = (ks*(N/32) + nt)*2 + part (order 1).   N % 32 == 0, K % 16 == 0. */
int ws_pack_w(const float* W, int N, int K, long long ldw, int trans, int order, float* out,
              void* stream);
/* The same units with fp16 hi = fp16(256 w) / lo = fp16(256 w - hi) (|W'| < 255: 256 w has to fit fp16; 22 bits, less where
 * the remainder is an fp16 subnormal) (ABI v15): the weight operand of ws_gemm_b2p with a_fmt = 2 (whose A
 * operand, the scaled-fp16 d(gates) of WS_GATES_H2F, then feeds v_mfma_f32_32x32x16_f16 without conversion).   */
int ws_pack_w_f16(const float* W, int N, int K, long long ldw, int trans, int order, float* out,
                  void* stream);
/* ABI v20: the weight operand of ws_gemm_b2p with a_fmt = 3 (N = 128, K % 64 == 0; fits the N*K*4 bytes of the other packs):
 * per stage of 64 k the sixteen fp16 hi fragments of ws_pack_w_f16, then per column tile one 2 KB operand fragment of
 * v_mfma_scale_f32_32x32x64_f8f6f4 with the e4m3 codes of the residuals (one exponent per fragment); the exponents (E8M0,
 * one dword per stage) behind the last stage                                                                          */
int ws_pack_w_f16f8(const float* W, int N, int K, long long ldw, int trans, float* out, void* stream);

/* plain -> BL:  C[(b,i)][n] = sum_k pro(A[pos(b,i)][k]) * W'[n][k] + bias[n]   (K = 128, N % 64 == 0)
 * pro = optional GroupNorm-on-load as in ws_gemm_nt (stat index computed from pos).  If A_bl is
 * given, the (normalised) operand is also written in BL(K), as BLS elements.  Replaces F.group_norm + the
 * nn.LSTM input projection (bsrnn.py:39-40) and autograd's d(hcat) of proj (bsrnn.py:42-44). */
typedef struct ws_gemm_p2b_args {
  const float* A;
  const float* Wpack;
  const float* bias;
  float* C;          /* BL(N) */
  float* A_bl;       /* BL(K) or NULL */
  const float* stats;
  const float* gamma;
  const float* beta;
  ws_seqmap sm;
  long long lda, st_m1, st_m2, st_base;
  int st_div1, st_div2, N, K;
  const unsigned* run_if;   /* optional device word: the launch does nothing unless *run_if != 0 */
  unsigned* amax;           /* optional device word (ABI v15): raised (atomic max on the float bits) to max |C| of this
                               launch; the caller zeroes it.  The scale source of WS_GATES_H2F                     */
  void* A_bl16;             /* optional (ABI v16): the (normalised) operand once more as fp16 elements in BLH(K) -- the
                               2-byte A operand of ws_gemm_tnb (a_fmt = 1)                                          */
} ws_gemm_p2b_args;
int ws_gemm_p2b(const ws_gemm_p2b_args* a, void* stream);
/* Ragged batches (inference): per-sequence valid STEP counts, the counterpart of ws_seqmap.nvalid along the other axis.
 * Sequence s has steps[s / steps_div] valid steps (device int table, entries in [1, L]); the slots of every later step are
 * treated like padded slots: operand and output exactly ZERO (selected, not multiplied: the rows they stand for may hold
 * anything; the bias is not added).  A recurrence that enters such a slot with zero state leaves it with zero state
 * (tanh(0) = 0), so the reverse direction of a BLSTM over precomputed gates (ws_lstm_fwd_cluster, ws_lstm_fwd) reaches the
 * sequence's last valid step exactly as if it had started there; the forward direction's tail is finite and unused.
 * The recurrences that compute the x-projection themselves (ws_lstm_fwd_cluster2, ws_lstm_fwd_fused) have no such
 * operand: ragged callers take the precomputed-gates branch. */
int ws_gemm_p2b_len(const ws_gemm_p2b_args* a, const int* steps, int steps_div, void* stream);

/* BL -> plain:  C[pos(b,i)][n] = sum_k A[(b,i)][k] * W'[n][k] + bias[n] + R[pos][n]   (N = 128, K % 64 == 0)
 * Replaces ResRNN.proj + residual (bsrnn.py:42-46) and autograd's d(normalised input).      */
typedef struct ws_gemm_b2p_args {
  const float* A;    /* BL(K), BLS elements (hcat of the recurrences / d(gates) of BPTT) */
  const float* Wpack;
  const float* bias; /* or NULL */
  const float* R;    /* plain, addressed like C, or NULL */
  float* C;          /* plain rows, leading dimension ldc */
  ws_seqmap sm;
  long long ldc;
  int N, K;
  int a_fmt, pad_;   /* ABI v15: 0 = A holds BLS pairs (BL(K)); 1 = A holds bf16 elements (BLH(K)): d(gates) of WS_GATES_H2;
                        2 = A holds scaled fp16 elements (BLH(K)): d(gates) of WS_GATES_H2F, scale from `amax`; Wpack
                        is then a ws_pack_w_f16 pack.  3 (ABI v20): as 2 with the lo term of the product on
                        v_mfma_scale_f32_32x32x64_f8f6f4 (Wpack from ws_pack_w_f16f8; e4m3 of A / 256 built in registers).
                        4: A holds h as two fp16 planes (H2P, above: hi at A, lo nblk blocks of BLH(K) behind it), Wpack is a
                        ws_pack_w_f16 pack: hi w_hi + hi w_lo + lo w_hi on the fp16 MFMA (the dropped lo w_lo is 2^-22 of the
                        product); no amax, no a16_out                                                                    */
  const unsigned* amax;
  void* a16_out;     /* optional (ABI v16, a_fmt 0 only: any other a_fmt with a16_out is refused): the A operand once more as
                        fp16(hi + lo) elements in BLH(K), padded slots included -- every block is read by exactly one wave
                        here, so the copy costs no extra read (hcat -> ws_gemm_tnb a_fmt = 1) */
} ws_gemm_b2p_args;
int ws_gemm_b2p(const ws_gemm_b2p_args* a, void* stream);
/* The two GEMMs with a folded speaker-fusion affine (ws_film_desc, above; rows of a / b by the POSITION of a slot, which may differ
 * between the 32 slots of a block): ws_gemm_p2b_film passes A through film before the normalisation (A_bl / A_bl16 are those of
 * z'; lda = 128); ws_gemm_b2p_film adds film(R) instead of R (a_fmt 0 and 4, the projections; R required, ldc = 128).  A film
 * with both pointers NULL is the plain call.                                                                                */
int ws_gemm_p2b_film(const ws_gemm_p2b_args* a, const ws_film_desc* film, void* stream);
int ws_gemm_b2p_film(const ws_gemm_b2p_args* a, const ws_film_desc* film, void* stream);

/* BL x BL -> weight gradients, one pass over G:
 *   slab[split][g][a] = sum_{b in split} sum_i G[(b,i)][g_off + g] * Acat[(b + shift,i)][a]
 *   bslab[split][g]   = sum G[(b,i)][g_off + g]                                  (if bslab)
 * Acat = columns [a0_off, a0_off + a0_cols) of A0 (BL(a0_width), shifted by a0_shift steps
 * inside the tile, zero outside [0, L)) followed by a1_cols columns of A1 likewise; Acat has 128
 * or 384 columns, g_cols is a multiple of 128.  aslab[split][a] (optional) = column sums of Acat.
 * G, A0 and A1 hold BLS elements; a0_shift must be 0 (only A1 is ever the step-shifted h); a1_shift is any number of
 * steps (|a1_shift| >= L: every shifted term is zero).  Split s owns blocks [s, s + 1) * blocks_per_split; a split behind
 * nblk writes zero slabs.  With g_fmt = 2 and BLS A operands the product runs on the fp16 instruction (the pair's terms lifted
 * by 2^6): |A| <= 1020 (bf16(|A|) * 64 <= 65504) is a precondition (the callers pass the normalised input and h), terms below 2^-20 are truncated.
 * Replaces autograd's dW_ih / dW_hh / db (nn.LSTM) and dW_proj / db_proj.                       */
typedef struct ws_gemm_tnb_args {
  const float* G;
  const float* A0;
  const float* A1;   /* or NULL */
  float* slab;
  float* bslab;      /* or NULL */
  float* aslab;      /* or NULL */
  long long slab_stride, bslab_stride, aslab_stride;
  int g_width, g_off, g_cols;
  int a0_width, a0_off, a0_cols, a0_shift;
  int a1_width, a1_off, a1_cols, a1_shift;
  int nblk, L, nsplit, blocks_per_split;
  int g_fmt;         /* ABI v15: 0 = G holds BLS pairs; 1 = G holds bf16 elements (BLH(g_width)): d(gates) of WS_GATES_H2;
                        2 = scaled fp16 elements: d(gates) of WS_GATES_H2F, scale from `amax` (slab / bslab come out unscaled) */
  const unsigned* amax;
  int a_fmt, pad_;   /* ABI v16: 0 = A0 / A1 hold BLS pairs; 1 = fp16 elements (BLH(a0_width) / BLH(a1_width)), g_fmt = 2 only:
                        scaled-fp16 G times fp16 A is ONE v_mfma_f32_32x32x16_f16 per product, and a workgroup loads 32 KB
                        per block instead of 56 (the kernel is bound by the CU's global-load issue rate)                */
} ws_gemm_tnb_args;
int ws_gemm_tnb(const ws_gemm_tnb_args* a, void* stream);
/* dW_proj^T = h^T dout on the fp16 hi plane of h (H2P storage, above; a new symbol of ABI v20, the same argument struct):
 *   slab[split][g][a] = sum G[(b,i)][g_off + g] * A0[(b,i)][a0_off + a],  aslab[split][a] = column sums of A0 (optional).
 * G holds fp16 elements in BLH(g_width) -- the hi plane, used as it is --, A0 BLS pairs in BL(a0_width) with exactly 128 columns
 * and no shift; no A1, no bslab, g_fmt = a_fmt = 0, amax REQUIRED: both bf16 terms of A0 are lifted into fp16 by the power of two
 * S = 2^(WS_DGATES_EXP - floor(log2 max|d(hcat)|)) that `amax` defines (the scale of WS_GATES_H2F) -- exact for every term whose
 * scaled magnitude is a normal fp16 number, rounded to nearest (at most 2^-25 / S off) in fp16's subnormals -- and a product is
 * two fp16 MFMAs; slab and aslab come out unscaled.  Precondition: |A0| S <= 65504, i.e. max |A0| < 2^7 max |d(hcat)| (A0 is
 * the gradient whose projection d(hcat) is; a projection weight of nearly zero breaks it: amax = 0 gives S = 1).  Beyond it the
 * lifted term is +-Inf and the slab non-finite -- like an overflowing d(gates) of WS_GATES_H2F it reaches ws_grad_norms' guard
 * and the step is skipped and counted, never a silently clipped gradient.  Splits as ws_gemm_tnb.                        */
int ws_gemm_tnb_h16(const ws_gemm_tnb_args* a, void* stream);

/* ---- STFT / iSTFT (torch.stft / torch.istft at bsrnn.py:309-316, 382-389) ---------------
 * n_fft = 512, hop = 128, periodic Hann, center + reflect pad.  Band-split spectrogram
 * layout xbs [R*Tf][2*F]: band g (first bin f0, width bw) occupies columns
 * [2*f0, 2*f0 + 2*bw) as [re(bw) | im(bw)]  == the reference's subband_spec (bsrnn.py:319-328).
 * band_of_bin: device int[F] -> band id; band_f0/band_bw: device int[nband].               */
typedef struct ws_bands {
  const int* band_of_bin;
  const int* band_f0;
  const int* band_bw;
  int nband, nbins;
} ws_bands;
int ws_stft_bandsplit(const float* wav, int R, int T, const ws_bands* b, float* xbs, void* stream);
/* Ragged batches (inference): row r holds lengths[r] valid samples, NFFT / 2 < lengths[r] <= T = the row pitch (device int
 * table; the callers that have the lengths on the host -- the engine, wesep_amd.dev -- refuse values outside that range,
 * the kernel clamps them to [NFFT / 2 + 1, T], the range in which the reflected index stays inside the row, so that no
 * table entry can move a read out of its row).  The reflect padding turns at lengths[r];
 * frames t >= 1 + lengths[r] / 128 are written as zeros; nothing behind lengths[r] is read.  The valid frames of a row are
 * bit for bit those of ws_stft_bandsplit on that row alone with T = lengths[r]. */
int ws_stft_bandsplit_len(const float* wav, int R, int T, const int* lengths, const ws_bands* b, float* xbs, void* stream);
/* mask3 [R*Tf][4*F]: band g occupies columns [4*f0, 4*f0+4*bw) in the reference's channel
 * order c = glu*2*bw + ri*bw + f (bsrnn.py:366-370).  frames [R*Tf][512] = windowed irfft of
 * (mask * X)  (bsrnn.py:371-381 + the first half of istft).                                */
int ws_mask_istft_frames(const float* xbs, const float* mask3, int R, int Tf, const ws_bands* b,
                         float* frames, void* stream);
/* overlap-add + window-envelope normalisation + centre trim -> wav [R][T]                  */
int ws_istft_ola(const float* frames, int R, int Tf, int T, float* wav, void* stream);
/* Ragged batches (inference): only the frames t < 1 + lengths[r] / 128 of row r are added and counted in the window
 * envelope (the others are not read, so ws_mask_istft_frames runs over the rectangle unchanged); samples >= lengths[r]
 * are written as zeros.  lengths: the device int table of ws_stft_bandsplit_len; this kernel clamps an entry to [1, T]
 * (nothing is reflected here: any value in that range keeps the last frame read, lengths[r] / 128, at most Tf - 1 and
 * the samples inside the row); on a table that is valid for ws_stft_bandsplit_len the two clamps do nothing. */
int ws_istft_ola_len(const float* frames, int R, int Tf, int T, const int* lengths, float* wav, void* stream);
/* backward of the two calls above: dwav [R][T] -> dmask3 [R*Tf][4*F]                        */
int ws_mask_istft_bwd(const float* dwav, const float* xbs, const float* mask3, int R, int Tf,
                      int T, const ws_bands* b, float* dmask3, void* stream);

/* ---- speaker fusion (speaker.py:81-125, norm.py:118-139) ---------------------------------
 * out[p][n] = z[p][n] * (a0 + a[r][n]) + b[r][n],  r = p / rows_per_r; a or b may be NULL. */
int ws_affine_fwd(const float* z, const float* a, const float* b, float a0, long long rows,
                  int rows_per_r, int N, float* out, void* stream);
/* dz_in = dz*(a0+a) (dz_in may be NULL); da_slab[split][r][n] = sum dz*z_in; db_slab likewise sum dz.
 * Split s of row r owns the rows j in [s * chunk, min(rows_per_r, (s + 1) * chunk)) of that r, chunk = ceil(rows_per_r /
 * nsplit); every slab element [nsplit][R][N] is written, a split that owns no row (nsplit above rows_per_r) leaves exact
 * zeros.  da_slab NULL (then z_in may be NULL) / db_slab NULL: that slab is not written.  N <= 128; N % 4 != 0 takes the
 * scalar kernel (same sums, row lanes in a different order).                                                       */
int ws_affine_bwd(const float* dz, const float* z_in, const float* a, float a0, long long rows,
                  int rows_per_r, int N, int nsplit, float* dz_in, float* da_slab, float* db_slab,
                  float* da, float* db, unsigned* counter, void* stream);
/* ABI v15: da / db [R][N] (optional) = the slabs summed over the splits, in split order, by the last workgroup of each
 * row r to finish; `counter`: R device words that are 0 at launch (left at 0).                                    */

/* ---- SI-SDR loss (auraloss.time.SISDRLoss via wesep/utils/losses.py:24-25) ---------------
 * loss = -mean_r 10 log10(|a t|^2 / (|x - a t|^2 + eps) + eps), zero-mean, eps = 1e-8.
 * rowstat [R][8] keeps (mean_x, mean_t, alpha, c1, c2, sisdr_dB, 0, 0) for the backward.   */
int ws_sisdr_fwd(const float* est, const float* tgt, int R, int T, float eps, float* rowstat,
                 float* loss, void* stream);
int ws_sisdr_bwd(const float* est, const float* tgt, const float* rowstat, const float* gout,
                 int R, int T, float* dest, void* stream);

/* ---- per-tensor clip (funcs.py:79-88) + Adam with coupled L2 (train.py:237-238) ----------
 * tab: device array of ws_tensor_ref, one per parameter tensor.                            */
typedef struct ws_tensor_ref {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long numel;
} ws_tensor_ref;
/* guard (optional device words; ABI v17: FOUR words, see ws_guard_commit): guard[0] is set to 1 when any tensor's norm is
 * NaN / Inf.  The caller zeroes guard[0] before the first launch of a step (the skip word of that step's
 * ws_clip_adam_step launches).  The launch only ever writes 1: a guard[0] that is non-zero at launch stays non-zero (no
 * launch resets it; it is untouched when every norm is finite), one that is 0 stays 0 when every norm is finite.  An entry
 * whose grad is NULL is not read: its norm is exactly 0 (and ws_clip_adam_step leaves its tensors untouched).          */
int ws_grad_norms(const ws_tensor_ref* tab, int ntensors, float* norms, unsigned* guard, void* stream);
/* ABI v17: closes an optimizer step's book-keeping ON THE DEVICE, after the step's last ws_clip_adam_step launch.  With
 * skipped := guard[0] != 0 || (skip1 && *skip1 != 0):  skipped -> ++guard[1] (steps skipped so far: exact, monotonic),
 * ++guard[2] (consecutive skipped steps), ++guard[3] (the bias-correction lag, below); else guard[2] = 0.  One thread.  */
int ws_guard_commit(unsigned* guard, const unsigned* skip1, void* stream);
/* if clip > 0: coef = clip / (norm + 1e-6); grad *= coef when coef < 1  (per tensor)
 * skip0 / skip1 (optional device words, ABI v15): the launch does NOTHING when one of them is non-zero at kernel start --
 * the guard word of ws_grad_norms (a non-finite gradient: a BPTT launch that timed out, on any rank of a data-parallel
 * job once the gradients are all-reduced) and / or the sticky status word of an in-place BPTT launch.  The reference
 * would apply the NaN to every weight (funcs.py:79-88: NaN comparisons are false, Adam follows).
 * step_lag (optional device word, ABI v17; pass &guard[3]): the bias corrections of Adam use  step - *step_lag  (>= 1), read
 * at kernel start: the host counts every ATTEMPTED step without waiting for the device, the device knows which of them
 * were skipped -- a skipped step must not advance the bias correction (torch.optim.Adam under a GradScaler does not call
 * step() at all).  The host subtracts what it has learnt asynchronously from both sides (FusedClipAdam._poll_guard).  */
int ws_clip_adam_step(const ws_tensor_ref* tab, int ntensors, const float* norms, float clip,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                      int clip_only, const unsigned* skip0, const unsigned* skip1, const unsigned* step_lag,
                      void* stream);

/* ---- Conv-TasNet / SpEx+, channels-last activations [R*T'][C] ----------
 * Everything that is not a 1x1 / framing convolution (those are ws_gemm_nt / ws_gemm_tn on row views).
 * Replaces, with their autograd: nn.PReLU (convs.py:60,73,123,137), GlobalChannelLayerNorm /
 * ChannelWiseLayerNorm (norm.py:7-59), the depthwise dilated Conv1d (convs.py:63-70,125-133), the
 * concatConv speaker fusion's broadcast half (convs.py:143-148), the decoder's mask product and
 * ConvTranspose1d overlap-add (decoder.py:92-114).                                                   */

/* mean / rstd of `ngroups` contiguous groups of n_per_group floats (gLN: one row's T'*C), chunked over
 * nchunk workgroups per group; scratch [ngroups][nchunk][4]; stats [ngroups][2] = (mean, 1/sqrt(var+eps)).
 * n_per_group % 4 == 0, x 16-byte aligned; any nchunk > 0: a chunk is ceil(n / 4 / nchunk) quads, the chunks behind the
 * group's end are empty and count for nothing (nchunk may exceed n / 4); above 64 chunks a lane merges several in turn.  */
int ws_flat_stats(const float* x, int ngroups, long long n_per_group, float eps, int nchunk,
                  float* scratch, float* stats, void* stream);
/* x += rb[m / rows_per_r] (rb may be NULL; x is updated in place = the saved pre-activation);
 * y = x > 0 ? x : a[0] * x                                                                         */
int ws_prelu_fwd(float* x, const float* rb, const float* a, long long rows, int C, int rows_per_r,
                 float* y, void* stream);
/* dx = dy * (pre > 0 ? 1 : a[0]) (dx may alias dy); slab[i < nslab] partial sums of dy * min(pre, 0): every entry is
 * written, a block that owns no quad (nslab above n / 1024) leaves an exact 0                        */
int ws_prelu_bwd(const float* pre, const float* dy, const float* a, long long n, float* dx, float* slab,
                 int nslab, void* stream);
/* y = b + depthwise_conv(norm(x)), norm applied on load with stats index m / st_div, zero "same" padding,
 * w [C][P] (odd P <= 7), dilation dil                                                               */
int ws_dwconv_fwd(const float* x, const float* stats, const float* gamma, const float* beta,
                  const float* w, const float* b, int R, int Tp, int C, int P, int dil, int st_div,
                  float* y, void* stream);
/* dxn = d(norm(x)); slab[split][P + 1][C]: rows 0..P-1 = dw[.][p] partials, row P = db partials.  Split s owns the rows
 * [s * rows_per_split, (s + 1) * rows_per_split) below R * Tp (nsplit * rows_per_split >= R * Tp; a split may straddle
 * two sequences); every slab element is written, a split that owns no row as exact zeros.  Every odd P <= 7 with any
 * C % 4 == 0 launches: above 64 KB of dynamic LDS (C >= 516 with P = 7, C >= 772 with P = 5) the entry raises the
 * kernel's limit once per device and returns WS_ERR_LAUNCH, before any launch, if the device refuses.  */
int ws_dwconv_bwd(const float* dy, const float* x, const float* stats, const float* gamma,
                  const float* beta, const float* w, int R, int Tp, int C, int P, int dil, int st_div,
                  float* dxn, int nsplit, int rows_per_split, float* slab, void* stream);
/* The same pair with a `causal` flag: non-zero puts every tap at or before t (taps t - (P-1-p)*dil), the causal
 * Conv1DBlock of wesep/modules/tasnet/convs.py:61-62,91-92 (padding dil*(P-1), last dil*(P-1) outputs cut)      */
int ws_dwconv_ex_fwd(const float* x, const float* stats, const float* gamma, const float* beta,
                     const float* w, const float* b, int R, int Tp, int C, int P, int dil, int st_div, int causal,
                     float* y, void* stream);
int ws_dwconv_ex_bwd(const float* dy, const float* x, const float* stats, const float* gamma,
                     const float* beta, const float* w, int R, int Tp, int C, int P, int dil, int st_div, int causal,
                     float* dxn, int nsplit, int rows_per_split, float* slab, void* stream);
/* slab[split * ngroups + grp][2][C]: per-channel sums of g and of g * xhat over the rows of group grp
 * (rows_per_group consecutive rows) that fall into the split; xhat = (x - mean_s) * rstd_s, s = m / st_div
 * (stats NULL: xhat = x; x NULL: second row exactly zero).  Split s owns the rows [s * per, (s + 1) * per) of every group,
 * per = ceil(rows_per_group / nsplit); every slab element is written, a split that owns no row as exact zeros.  */
int ws_chan_sums(const float* g, const float* x, const float* stats, int st_div, int rows_per_group,
                 int ngroups, int nsplit, int C, float* slab, void* stream);
/* ab[grp] = (sum_c gamma[c] * S0[grp][c], sum_c gamma[c] * S1[grp][c]) / n_per_group, sums [ngroups][2][C] */
int ws_norm_ab(const float* sums, const float* gamma, int ngroups, int C, long long n_per_group,
               float* ab, void* stream);
/* dx = rstd_s * (dxn * gamma - ab0_s - xhat * ab1_s) (+ res), s = m / st_div (dx may alias dxn)        */
int ws_norm_bwd_apply_cl(const float* x, const float* dxn, const float* stats, const float* ab,
                         const float* gamma, const float* res, long long rows, int C, int st_div,
                         float* dx, void* stream);
/* s = w * m (w with leading dimension ldw); backward: dw = ds * m (leading dimension ld_dw),
 * dm = ds * w * (m > 0)  (m is the ReLU output of the mask GEMM)                                     */
int ws_maskmul_fwd(const float* w, long long ldw, const float* m, long long rows, int N, float* s,
                   void* stream);
int ws_maskmul_bwd(const float* ds, const float* w, long long ldw, const float* m, long long rows, int N,
                   float* dw, long long ld_dw, float* dm, void* stream);
/* d *= (y > 0), in place                                                                            */
int ws_relu_mask(float* d, const float* y, long long n, void* stream);
/* est[r][j] = bias[0] + sum_t frames[r*Tp + t][j - hop*t], j < Tout <= (Tp-1)*hop + L; and the adjoint
 * gather dframes[m][k] = hop*t + k < Tout ? dest[r][hop*t + k] : 0                                     */
int ws_ola_fwd(const float* frames, const float* bias, int R, int Tp, int L, int hop, int Tout,
               float* est, void* stream);
int ws_ola_bwd(const float* dest, int R, int Tp, int L, int hop, int Tout, float* dframes, void* stream);
/* slab[i < nslab] = partial sums of x[0..n): every entry written, exactly 0 for a block that owns nothing */
int ws_sum_partial(const float* x, long long n, float* slab, int nslab, void* stream);

/* ---- SpEx+ speaker encoder (wesep/modules/tasnet/speaker.py:7-64), channels-last [M][C] ------------------
 * nn.BatchNorm1d in training mode: stats [2][C] = (batch mean, 1/sqrt(biased var + eps)), two passes;
 * running_mean / running_var (both or neither) are updated with `momentum` (unbiased variance tracked).
 * scratch: nsplit * C floats.                                                                          */
int ws_bn_stats(const float* x, long long M, int C, float eps, float momentum, float* running_mean,
                float* running_var, int nsplit, float* scratch, float* stats, void* stream);
/* u = gamma * (x - mean_c) * rstd_c + beta (+ res);  y = PReLU(u, a[0])                                  */
int ws_bn_prelu_fwd(const float* x, const float* stats, const float* gamma, const float* beta,
                    const float* res, const float* a, long long M, int C, float* u, float* y, void* stream);
/* BatchNorm backward from du: sums [2][C] = (sum du, sum du * xhat) = (dbeta, dgamma);
 * dx = gamma * rstd * (du - sums0/M - xhat * sums1/M) (dx may alias du); slab: nsplit * 2 * C floats, split s = the rows
 * [s * ceil(M / nsplit), +ceil(M / nsplit)) below M, exact zeros where it owns none                      */
int ws_bn_bwd(const float* x, const float* du, const float* stats, const float* gamma, long long M, int C,
              int nsplit, float* slab, float* sums, float* dx, void* stream);
/* nn.MaxPool1d(3) over time on [R][T][C] -> [R][T/3][C]; backward to the first maximal position        */
int ws_maxpool3_fwd(const float* x, int R, int T, int C, float* y, void* stream);
int ws_maxpool3_bwd(const float* x, const float* dy, int R, int T, int C, float* dx, void* stream);
/* out[m][c] = scale * src[m / rows_per_r][c]                                                            */
int ws_bcast_rows(const float* src, float scale, int rows_per_r, long long M, int C, float* out, void* stream);
/* nn.CrossEntropyLoss (mean) on [R][S] logits, int64 labels: loss[0] and dlogits = d loss / d logits     */
int ws_cross_entropy(const float* logits, const long long* label, int R, int S, float* loss, float* dlogits,
                     void* stream);

/* ---- forward recurrence with the input projection fused in (blocked layout, 32-sequence workgroups) --------
 * Replaces ws_gemm_p2b(x-projection) + ws_lstm_fwd(WS_LSTM_BF16X3_BLK) for views with many sequences:
 * xn is the normalised ResRNN input in BL(128); gates (BL(2048)) receives the ACTIVATED gates, cbuf / hcat
 * (BL(512)) as in ws_lstm_fwd; bias [2][4H] = b_ih + b_hh per direction.  wpack: ws_lstm_pack_fused output,
 * WS_LSTM_FUSED_PACK_FLOATS floats ([W_ih | W_hh] as one K = 384 stream of bf16 hi/lo MFMA fragments).       */
typedef struct ws_lstm_fused_args {
  float* gates;
  float* cbuf;
  float* hcat;
  const float* xn;
  const float* wpack;
  const float* bias;
  int nseq, L;
  int gfmt;             /* ABI v15: WS_GATES_* (!= 0: `gates` receives unorm16 BLH) */
  int hfmt;             /* ABI v19 (the former pad_: 0 = every earlier behaviour): 1 = the recurrent part of the stream on
                           v_mfma_f32_32x32x16_f16 with h as ONE fp16 operand and W_hh as fp16 hi / lo of 256 w (two MFMAs per
                           product instead of three; the arithmetic of ws_lstm_fwd_cluster2) -- wpack from
                           ws_lstm_pack_fused_h16, 2-byte gate formats only.  Bit 1 (value
                           2, measurement): the 64-sequence kernels drain every store of a step before the next one starts
                           (the wait of rounds 3-5).  Bit 2 (ABI v20; with bit 0: hfmt = 5): the lo term of that product on
                           v_mfma_scale_f32_32x32x64_f8f6f4 -- the residuals 256 w - hi as e4m3 codes with one exponent per
                           fragment against an e4m3 image of h: four fp16 MFMAs + one FP8 MFMA (K = 64, twice the rate) per
                           recurrent k-step instead of eight; wpack from ws_lstm_pack_fused_h8 (64- and 32-sequence kernels).
                           Bit 3 (value 8, with bit 0): hcat leaves as two fp16 planes (H2P, above) instead of BLS pairs; gates
                           and cbuf are bit-identical to the launch without it.
                           Bit 4 (value 16, with bit 3; no new ABI version): cbuf leaves as fp16 in BLH(2H) (C16, above) instead
                           of fp32 BL; gates and both planes of h are bit-identical to the launch without it              */
} ws_lstm_fused_args;
#define WS_LSTM_FUSED_PACK_FLOATS (2 * 8 * 24 * 4 * 2 * 64 * 4)
int ws_lstm_pack_fused(const float* wih_f, const float* wih_r, const float* whh_f, const float* whh_r,
                       float* pack, void* stream);
/* ABI v19: the pack of hfmt = 1 -- same size and unit order; both parts hold 256 w: W_ih as bf16 hi / lo, W_hh as fp16 hi / lo */
int ws_lstm_pack_fused_h16(const float* wih_f, const float* wih_r, const float* whh_f, const float* whh_r,
                           float* pack, void* stream);
/* ABI v20: the pack of hfmt = 5 (fits the same WS_LSTM_FUSED_PACK_FLOATS): per (direction, wave) the W_ih k-steps of the h16
 * pack, then 16 recurrent k-steps of four fp16 hi fragments + one 2 KB FP8 fragment, then the 16 fragment exponents (E8M0)  */
int ws_lstm_pack_fused_h8(const float* wih_f, const float* wih_r, const float* whh_f, const float* whh_r,
                          float* pack, void* stream);
int ws_lstm_fwd_fused(const ws_lstm_fused_args* a, void* stream);

/* ---- wespeaker ResNet speaker encoder (third-party model, call sites
 * wesep/models/bsrnn.py:9,217,352-356), channels-last [R][H][W][C] ------------------------------------------
 * conv2d(k x k, stride s, padding p, bias-free) = ws_im2col + ws_gemm_nt (K = k*k*C); input gradient =
 * ws_gemm_nt + ws_col2im (gather, deterministic); weight gradient = ws_gemm_tn on the patch matrix.
 * patches [R*Ho*Wo][ldp], column (ky*k + kx)*C + c; Ho = (H + 2p - k)/s + 1.  C == 1 (ldp >= k*k; only the first k*k
 * columns of a row are written, the padding [k*k, ldp) is left untouched) or C % 4 == 0 (then ldp == k*k*C and x, patches
 * 16-byte aligned).  im2col is a copy: bit-exact, taps outside the image are exact zeros.  ws_col2im needs C % 4 == 0 (no
 * C == 1 form) and 16-byte aligned dpatches / dx; a pixel that no patch covers (stride above k, or the tail behind the last
 * whole stride when (H + 2p - k) % s != 0) is written as an exact zero.  ws_im2col / ws_col2im are ws_im2col_hw /
 * ws_col2im_hw with sh = sw = s.  BatchNorm2d / ReLU / residual are the channels-last ws_bn_* / ws_prelu_* entry points. */
int ws_im2col(const float* x, int R, int H, int W, int C, int k, int s, int p, long long ldp, float* patches,
              void* stream);
int ws_col2im(const float* dpatches, int R, int H, int W, int C, int k, int s, int p, float* dx, void* stream);
/* TSTP pooling: x [R][F][T][C] -> stats [R][2][C*F] = (mean over T, sqrt(unbiased var + eps)), feature c*F + f; two
 * passes, var = sum (x - mean)^2 / (T - 1); T = 1: var = 0, std = sqrt(eps)                                        */
int ws_tstp_fwd(const float* x, int R, int F, int T, int C, float eps, float* stats, void* stream);
int ws_tstp_bwd(const float* x, const float* stats, const float* dstats, int R, int F, int T, int C, float* dx,
                void* stream);
/* ASTP (attentive statistics pooling, wespeaker ECAPA-TDNN; wesep/models/bsrnn.py:217,352-356 via bsrnn.yaml:66-71) on
 * channels-last x, logits [R][T][C]: alpha = softmax_T(logits), out [R][2C] = sum alpha x || sqrt(max(sum alpha x^2 -
 * mean^2, floor)), aux [R][4][C] = (max logit, sum exp, mean, sum alpha x^2) saved for ws_astp_bwd (aux[3] is E[x^2],
 * not the variance).  ws_astp_bwd takes the gradient through std where aux[3] - aux[2]^2 > floor (strict), 0 otherwise. */
int ws_astp_fwd(const float* x, const float* logits, int R, int T, int C, float floor_, float* out, float* aux,
                void* stream);
int ws_astp_bwd(const float* x, const float* logits, const float* out, const float* aux, const float* dout, int R, int T,
                int C, float floor_, float* dx, float* dlogits, void* stream);
/* MHASTP / MQMHASTP (wespeaker multi-head / multi-query multi-head attentive statistics pooling; csrc/mhastp.hip) on
 * channels-last x [R][F][T][C]: Q queries x H heads, head h = channels [h*C/H, (h+1)*C/H) x all F rows, d_model
 * dm = C/H*F, upstream feature index c*F + f.  layers 2: logits = W2 tanh(W1 x + b1) + b2 (W1 [64][dm], W2 [ds][64]);
 * layers 1: logits = W1 x + b1 (W1 [ds][dm]); ds = 1 (one logit row per head) or dm (one per feature).
 * pack = Q*H blocks of ws_mhastp_sizes(..., block_floats) floats, block (q, h) at (q*H + h): W1 with columns in the
 * order f*(C/H) + c, b1, then (layers 2) W2, b2 as they are; ws_mhastp_pack writes one block.
 * fwd: out [R][Q][H][2][dm] = (mean, sqrt(max(var, 1e-7))) per head in upstream order; aux [R][Q][H][4][dm] = (max logit,
 * sum exp, mean, var), features in the kernel order f*(C/H) + c, for ws_mhastp_bwd (aux[3] is the raw, unclamped
 * variance sum alpha x^2 - mean^2, where ASTP's is E[x^2]).  One launch for any T.  ws_mhastp_bwd takes the gradient
 * through std where aux[3] >= 1e-7 (not strict), 0 otherwise.
 * bwd: dx [R][F][T][C] (written, not accumulated).  dpack NULL: no weight gradients (one launch).  Otherwise work =
 * ws_mhastp_sizes(..., work_floats) floats, slab = nsplit * Q*H*block floats (unused when nsplit == 1) and
 * dpack gets the weight gradients in the pack layout but with W1's columns in the upstream order c*F + f, i.e.
 * every block is (dW1, db1, dW2, db2) as the parameters are shaped (two more launches, deterministic: no atomics).
 * Split s of the weight gradients sums the rows m = r*T + t in [s*ceil(R*T/nsplit), ...); a split that owns no row is
 * legal and leaves exact zeros in its slab. */
/* block_floats: one (query, head) block of the pack; work_floats: the backward's workspace (either pointer may be NULL) */
int ws_mhastp_sizes(int R, int T, int Q, int H, int layers, int ds, int d_model, long long* block_floats,
                    long long* work_floats);
int ws_mhastp_pack(const float* w1, const float* b1, const float* w2, const float* b2, int F, int Ch, int layers, int ds,
                   float* blk, void* stream);
int ws_mhastp_fwd(const float* x, const float* pack, int R, int F, int T, int C, int Q, int H, int layers, int ds,
                  float* out, float* aux, void* stream);
int ws_mhastp_bwd(const float* x, const float* pack, const float* aux, const float* dout, int R, int F, int T, int C,
                  int Q, int H, int layers, int ds, float* dx, float* work, float* slab, int nsplit, float* dpack,
                  void* stream);
/* The same pooling on a grid split over T (the 1-D speaker encoders, which pool at the full frame rate: ECAPA-TDNN,
 * CAM++).  ws_mhastp_split_sizes: tsplit, the T splits that cover about two workgroups per CU (cus) over the R*H
 * (row, head) pairs, and part_floats = tsplit*R*Q*H*4*d_model, the forward's workspace.  fwd_split: workgroup (r*H + h, s)
 * keeps the online-softmax state of frames [s*ceil(T/tsplit), ...) in part, then one merge launch combines the splits in
 * ascending order and writes out and aux exactly as ws_mhastp_fwd lays them out (two launches, no atomics).
 * bwd_split: ws_mhastp_bwd with its dx launch on the (R*H, tsplit) grid; the weight gradients are unchanged.
 * 1 <= tsplit <= T.  A T split that owns no frame (ceil(T/tsplit)*s >= T) is legal: it leaves the state
 * (-inf, 0, 0, 0) in part, the merge skips it, and the backward writes nothing for it.                              */
int ws_mhastp_split_sizes(int R, int F, int T, int C, int Q, int H, int cus, int* tsplit, long long* part_floats);
int ws_mhastp_fwd_split(const float* x, const float* pack, int R, int F, int T, int C, int Q, int H, int layers, int ds,
                        int tsplit, float* part, float* out, float* aux, void* stream);
int ws_mhastp_bwd_split(const float* x, const float* pack, const float* aux, const float* dout, int R, int F, int T,
                        int C, int Q, int H, int layers, int ds, int tsplit, float* dx, float* work, float* slab,
                        int nsplit, float* dpack, void* stream);
/* y = act(x + rb[row / rows_per_r]) on [rows][C] (act 1 tanh, 3 sigmoid; rb NULL or [ceil(rows / rows_per_r)][C]: the
 * last bias row may serve fewer than rows_per_r rows) and dx = dy * act'(y) from the saved output (dx = dy (1 - y^2) or
 * dy y (1 - y)): ECAPA's attention bottleneck (tanh) and SE gate (sigmoid).  Scalar accesses: any C, n and alignment. */
int ws_rowbias_act_fwd(const float* x, const float* rb, long long rows, int C, int rows_per_r, int act, float* y,
                       void* stream);
int ws_act_bwd(const float* y, const float* dy, long long n, int act, float* dx, void* stream);

/* Segment pooling of the CAM++ context-aware mask (wespeaker `CAMPPlus`, the recipe's alternative speaker encoder:
 * wesep/models/bsrnn.py:217 via examples/librimix/tse/v2/confs/bsrnn.yaml:66-74; F.avg_pool1d(seg_len, ceil_mode) expanded
 * back over the frames) on channels-last [R][T][C], nseg = ceil(T / seg_len), last segment of an utterance shorter:
 *   ws_seg_sums : out[r][s][c] = sum_{t in segment s} a[r][t][c] (* b[r][t][c] when b)
 *   ws_seg_scale: out[r][t][c] = (x ? x[r][t][c] : 1) * m[r][t / seg_len][c]            (out may alias x)          */
int ws_seg_sums(const float* a, const float* b, int R, int T, int C, int seg_len, float* out, void* stream);
int ws_seg_scale(const float* x, const float* m, int R, int T, int C, int seg_len, float* out, void* stream);

/* ---- in-model enrollment front-end (bsrnn.py:231-242,343-350) -------------------
 * out[r][j] = y[reflect(j - pad)], y = pre-emphasis of x (speaker.py:10-23), row stride ldo >= T + 2*pad:
 * the centred, reflect-padded signal whose hop-strided row views are the STFT frames.  y[0] = x[0] - coef*x[1]
 * (a reflect pad of 1), so T > 1 and T > pad; columns [T + 2*pad, ldo) are not written.                    */
int ws_preemph_pad(const float* x, int R, int T, int pad, int ldo, float coef, float* out, void* stream);
/* p[m][f] = re^2 + im^2 of interleaved spectra [M][lds] (nf bins); columns nf..ldp-1 zeroed               */
int ws_power_spec(const float* spec, long long M, int nf, int lds, int ldp, float* p, void* stream);
/* x = log(x + eps) in place                                                                               */
int ws_log_eps(float* x, long long n, float eps, void* stream);

/* ---- DPCCN pieces (wesep/modules/dpccn/convs.py, wesep/models/dpccn.py) -----------
 * channels-last [B][H][W][C], H = frame, W = frequency bin.  Conv2d / ConvTranspose2d with per-axis strides:
 * ws_im2col_hw + GEMM, and GEMM + ws_col2im_hw (the transposed convolution is the col2im gather of a GEMM output).*/
int ws_im2col_hw(const float* x, int R, int H, int W, int C, int k, int sh, int sw, int p, long long ldp,
                 float* patches, void* stream);
int ws_col2im_hw(const float* dpatches, int R, int H, int W, int C, int k, int sh, int sw, int p, float* dx,
                 void* stream);
/* ALIGNMENT of the DPCCN / TF-GridNet entry points below: ws_elu_*, ws_inorm_apply / bwd_apply, ws_in_act_*, ws_avgpool_*,
 * ws_bilinear_*, ws_scale_bf_fwd and ws_freq_linear_fwd (x, y) move 16 bytes per access -- every tensor pointer and every
 * row stride (C, ldy, ldd, lddx; a column offset into a wider map likewise) must be a multiple of 4 floats from a 16-byte
 * aligned base.  The entry points check C % 4 and the strides, not the pointers.  ws_inorm_finalize, ws_rowbias_act_fwd,
 * ws_act_bwd, ws_scale_bf_bwd with its scalar kernel and ws_softmax_rows_* with theirs take any alignment.
 * nn.ELU: y = x > 0 ? x : expm1(x);  dx = dy * (x > 0 ? 1 : exp(x)) (dx may alias dy);  n % 4 == 0.  x > 0 is a copy. */
int ws_elu_fwd(const float* x, long long n, float* y, void* stream);
int ws_elu_bwd(const float* x, const float* dy, long long n, float* dx, void* stream);
/* InstanceNorm{1,2}d without affine over the P positions of each of G batch rows ([G*P][C] channels-last):
 * sums [G][2][C] = ws_chan_sums(g = x, x = x) = (sum u, sum u^2) -> stats [G][2][C] = (mean, rstd) in ONE pass:
 *   mean = S0 / P,  rstd = 1 / sqrt(max(S1 / P - mean^2, 0) + eps)     (fp32; the clamp absorbs the cancellation of a
 *   constant group, whose rstd is then 1 / sqrt(eps); with |mean| >> std the variance carries ~ P * 2^-24 * mean^2 of error)
 * y = (x - mean) * rstd;  backward with sums = ws_chan_sums(g = dy, x = y): dx = rstd * (dy - S0/P - y * S1/P), dx may
 * alias dy.  ws_inorm_finalize: any C; apply / bwd_apply: C % 4 == 0, rows % P == 0 (rows = G * P).           */
int ws_inorm_finalize(const float* sums, int G, int C, long long P, float eps, float* stats, void* stream);
int ws_inorm_apply(const float* x, const float* stats, long long rows, int P, int C, float* y, void* stream);
int ws_inorm_bwd_apply(const float* y, const float* dy, const float* stats, const float* sums, long long rows, int P,
                       int C, float* dx, void* stream);
/* 3 x 3, stride-1, padding-1 convolution of a channels-last image through an LDS halo tile (conv3x3.hip): every input
 * pixel crosses the L2 -> CU path ~1.2 times instead of the 9 of the implicit patch matrix.  Replaces F.conv2d of the
 * dense blocks (wesep/modules/dpccn/convs.py:80-112) and, with the flipped / channel-swapped weights, its input gradient:
 *   Y[m][n] = bias[n] + R[m][n] + sum_{ky,kx,c} X[pixel(m) + (ky-1, kx-1)][c] * W[n][(ky*3 + kx)*Cin + c],  m = (b*H + h)*Wd + w
 * X: pixel stride ldx >= Cin; Y and R (bias / R may be NULL; R may alias Y): row stride ldy >= Cout.
 * W: the weights PACKED as bf16 hi / lo MFMA fragments, ceil(Cin / 16) * 9 * NTP * 2 units of 64 lanes x 8 bf16, NTP =
 * ceil(Cout / 32) rounded up to even when above 2 (wesep_amd.dev.conv3x3_pack writes the layout: unit
 * (((chunk*9 + tap)*NTP + t)*2 + part)*64 + lane = W[t*32 + (lane & 31)][tap][16 chunk + 8 (lane >> 5) + j], zero beyond
 * Cout / Cin; part 0 = bf16(w), part 1 = bf16(w - hi)); ldw is ignored.  Cin % 4 == 0, Cout % 4 == 0, Cout <= 1024.
 * Split-bf16 products, fp32 accumulation. */
typedef struct ws_conv3x3_args {
  const float* X;
  const float* W;
  const float* bias;
  const float* R;
  float* Y;
  long long ldx, ldw, ldy;
  int B, H, Wd, Cin, Cout, pad_;
} ws_conv3x3_args;
int ws_conv3x3(const ws_conv3x3_args* a, void* stream);
/* ABI v19: the packed weights of ws_conv3x3 in ONE launch from up to WS_C3_NSRC strided views of weight tensors -- the logical
 * W[n][tap][c] (n < Cout rows, c < Cin columns, zero-padded to the fragment grid) takes column c from the source k whose range
 * [col_off, col_off + cols) holds it:  W = w_k[n * s_row + (c - col_off) * s_col + (flip ? 8 - tap : tap) * s_tap].
 * A column that no source covers is zero.  The sources' column ranges must not overlap.
 * A layer's forward: one source, nn.Conv2d weight [co][ci][3][3] -> (s_row, s_col, s_tap) = (9 Ci, 9, 1), flip 0.  The input
 * gradient of a channel block [lo, hi) of a dense block (convs.py:80-112): sources = the weights of the layers that read the
 * block, pointers advanced to input channel lo, rows = the block's channels (s_row = 9), columns = the layers' output channels
 * side by side (s_col = 9 Ci_k), flip 1.  out: ceil(Cin / 16) * 9 * NTP * 2 * 64 * 8 bf16 (= half as many floats).        */
#define WS_C3_NSRC 5
typedef struct ws_conv3x3_pack_src {
  const float* w;
  long long s_row, s_col, s_tap;
  int col_off, cols;
} ws_conv3x3_pack_src;
typedef struct ws_conv3x3_pack_args {
  ws_conv3x3_pack_src src[WS_C3_NSRC];
  float* out;
  int Cin, Cout, nsrc, flip;
} ws_conv3x3_pack_args;
int ws_conv3x3_pack(const ws_conv3x3_pack_args* a, void* stream);
/* Weight (and bias) gradient of a 3 x 3 convolution with padding 1, stride 1 along h and sw = 1 or 2 along w, one pass
 * over the image (conv3x3.hip; replaces ws_conv_wgrad / the implicit TN GEMM for these shapes: the dense blocks, the
 * (1, 2)-strided encoder convolutions and -- with image = dy, G = x -- the decoder's transposed convolutions of
 * wesep/modules/dpccn/convs.py, and the 3 x 3 convolutions of the ResNet speaker encoder):
 *   slab[split][n][(ky*3 + kx)*Cin + c] = sum over the split's pixels m = (b, h, w) of G[m][n] * X[b][h + ky - 1][sw*w + kx - 1][c]
 *   bslab[split][n]                    = sum over the split's pixels of G[m][n]                       (bslab may be NULL)
 * G [B*H*Wd rows, stride ldg >= Nn]; X [B][H][Wx] pixels of stride ldx >= Cin, Wd = (Wx - 1) / sw + 1.  The gradient grid
 * is cut into tiles of 30 rows x 4 columns (B * ceil(H / 30) * ceil(Wd / 4) of them, column-fastest); split s owns tiles
 * [s, s + 1) * tiles_per_split.  A split that owns no tile writes zeros to its slab and its bslab.  The caller sums the
 * nsplit slabs (ws_reduce_slabs: deterministic, no atomics).
 * Cin % 4 == 0, Nn % 4 == 0. */
typedef struct ws_conv3x3_wgrad_args {
  const float* G;
  const float* X;
  float* slab;
  float* bslab;
  long long ldg, ldx, slab_stride, bslab_stride;
  int B, H, Wd, Wx, sw, Cin, Nn, nsplit, tiles_per_split, pad_;
} ws_conv3x3_wgrad_args;
int ws_conv3x3_wgrad(const ws_conv3x3_wgrad_args* a, void* stream);

/* InstanceNorm fused with its neighbouring ELU (convs.py:28-77: conv - ELU - IN; convs.py:115-152: IN - ELU - conv):
 *   flags bit 0: y = IN(ELU(x));  bit 1: y = ELU(IN(x));  statistics [G][2][C] as ws_inorm_finalize writes them.
 * ws_in_act_sums: slab[nsplit][G][2][C] partial sums over the P rows of each group -- forward (dy NULL): (sum u, sum u^2)
 * of u = pre(x), to be reduced and finalised by ws_reduce_slabs + ws_inorm_finalize; backward: (sum d, sum d * n) with
 * n = (u - mean) * rstd and d = dy * (bit 1 ? ELU'(n) : 1).  ws_in_act_apply: y from x and the statistics (one pass).
 * ws_in_act_bwd_apply: dx = pre'(x) * rstd * (d - S0/P - n * S1/P) from x, dy, the statistics and the reduced sums
 * (dx may alias dy when both strides agree).  ws_in_act_sums writes EVERY element of the slab: split s owns the rows
 * [s * per, min(P, (s + 1) * per)), per = ceil(P / nsplit), and a split that owns no row (nsplit does not divide P, or
 * nsplit > P) leaves exact zeros; any nsplit >= 1 is legal and the reduced sums agree within rounding.  The backward sums need
 * the statistics (stats NULL with dy is refused); flags outside 0..3 are refused.  ws_in_act_apply / bwd_apply write the
 * columns [0, C) of every row of y / dx and nothing between C and the row stride.
 * Only the pre-activation x has to be kept for the backward.  x is dense
 * [rows][C]; y (apply) has row stride ldy, dy (sums, bwd_apply) row stride ldd and dx row stride lddx -- 0 = C, else >= C and % 4: the
 * dense blocks write y into / read dy from a column range of their one wide feature map (no torch.cat, no slices). */
int ws_in_act_sums(const float* x, const float* dy, long long ldd, const float* stats, int P, int G, int nsplit, int C,
                   int flags, float* slab, void* stream);
int ws_in_act_apply(const float* x, const float* stats, long long rows, int P, int C, int flags, float* y, long long ldy,
                    void* stream);
int ws_in_act_bwd_apply(const float* x, const float* dy, long long ldd, const float* stats, const float* sums, long long rows,
                        int P, int C, int flags, float* dx, long long lddx, void* stream);
/* nn.AvgPool2d(sz) (stride sz, floor: H >= sz, W >= sz) and its adjoint: dx = dy / sz^2 on the covered pixels, EXACT zeros
 * on the H % sz rows / W % sz columns the floor drops (all of dx is written).  nn.Upsample(size = (H, W), mode = "bilinear")
 * (align_corners False: src = max((dst + 1/2) * h / H - 1/2, 0), taps floor(src) and min(floor(src) + 1, h - 1); any h, w,
 * H, W >= 1, up- or downsampling) and its adjoint (a gather over destination pixels).  C % 4 == 0.              */
int ws_avgpool_fwd(const float* x, int B, int H, int W, int C, int sz, float* y, void* stream);
int ws_avgpool_bwd(const float* dy, int B, int H, int W, int C, int sz, float* dx, void* stream);
int ws_bilinear_fwd(const float* x, int B, int h, int w, int H, int W, int C, float* y, void* stream);
/* tmp: scratch of B * H * w * C floats (the adjoint runs as two separable passes: destination columns, then rows): all of
 * it is overwritten, nothing behind it; its contents afterwards are unspecified.                                       */
int ws_bilinear_bwd(const float* dy, int B, int h, int w, int H, int W, int C, float* tmp, float* dx, void* stream);
/* SpeakerFuseLayer multiply (mode 0) / additive (mode 1) on [B][T][F][C] with s [B][F] (speaker.py:102-121);
 * backward: dx (mode 1: a copy of dy), and ds [B][F] = sum over (t, c) of dy * x (mode 0) or dy (mode 1).  The forward needs
 * C % 4 == 0.  The backward takes any C: C % 4 == 0, C <= 1024 and (C / 4) dividing 256 select the 16-byte kernel (C / 4
 * threads per row, 256 / (C / 4) rows per pass, two passes in flight; x, dy, dx 16-byte aligned), every other C -- 6, 12,
 * 1028 -- the scalar kernel, which has no alignment requirement.  One workgroup per (b, f): deterministic.      */
int ws_scale_bf_fwd(const float* x, const float* s, int B, int T, int F, int C, int mode, float* y, void* stream);
int ws_scale_bf_bwd(const float* x, const float* dy, const float* s, int B, int T, int F, int C, int mode, float* dx,
                    float* ds, void* stream);
/* ABI v17: SpeakerFuseLayer 'concat' (speaker.py:95-101) on [B][T][F][C]: the Linear over the frequency axis of cat[x, e] --
 * y[b][t][f'][c] = sum_f W[f' * ldw + f] x[b][t][f][c] + rb[b][f'];  W: the first F columns of fc.linear.weight [F][F + E]
 * (ldw = F + E >= F; the columns [F, ldw) of W are not read), rb [B][F] = We e + bias (ws_gemm_nt).  Exact fp32; C % 4 == 0,
 * F * C <= 16384 (the [F][C] tile of one (b, t) in 64 KB of LDS; more is refused).  Forward only: the native runtime's
 * form of the fusion (runtime/engine.cc); training composes it from GEMMs on a transposed view.                    */
int ws_freq_linear_fwd(const float* x, const float* W, long long ldw, const float* rb, int B, int T, int F, int C, float* y,
                       void* stream);

/* ---- TF-GridNet: everything but this row softmax is composed from the entry points
 * above (gridnet_block.py:212-213): y = softmax(scale * x) per row of n (the maximum of scale * x is subtracted first);
 * dx = scale * y * (dy - sum(dy * y)).  Any n >= 1 and any alignment: n <= 1024, n % 4 == 0 and 16-byte aligned x, y (y, dy,
 * dx) select the one-pass 16-byte kernels, everything else the scalar ones; both give the same values within rounding.  */
int ws_softmax_rows_fwd(const float* x, long long rows, int n, float scale, float* y, void* stream);
int ws_softmax_rows_bwd(const float* y, const float* dy, long long rows, int n, float scale, float* dx, void* stream);

/* nn.LayerNorm over short rows (gridnet_block.py:139-160 `intra_norm` / `inter_norm`, width = emb_dim; also any
 * [M][W] with W <= 256, W % 4 == 0): one pass forward (y and the (mean, rstd) pairs stats[M][2]), one pass backward:
 *   dx = rstd * (gamma*dy - mean_row(gamma*dy) - xhat * mean_row(gamma*dy*xhat)) (+ res; dx may alias dy)
 *   slab[ws_rowln_grid(M, W)][2][W]: per-workgroup partial sums of d(beta) (row 0) and d(gamma) (row 1); the caller
 *   reduces them (ws_reduce_slabs) -- the grid is a function of (M, W) only, so the sums are reproducible.      */
int ws_rowln_grid(long long M, int W);
int ws_rowln_fwd(const float* x, const float* gamma, const float* beta, long long M, int W, float eps, float* y,
                 float* stats, void* stream);
int ws_rowln_bwd(const float* x, const float* dy, const float* stats, const float* gamma, const float* res, long long M,
                 int W, float* dx, float* slab, void* stream);

/* The attention heads of a TF-GridNet block in one pass (heads.hip; gridnet_block.py:176-199: per head Conv2d(1x1) ->
 * PReLU -> LayerNormalization4DCF over (E, F), heads concatenated along the batch, `.transpose(1, 2).flatten(2)`):
 *   y[(h*B + b)*Tp + t][q*ch + e] = gamma[h][q*ch + e] * (u - mean) * rstd + beta[h][q*ch + e],
 *   u = PReLU(x[(b*T + t)*Q + q][h*ch + e]; slope[h]),  mean / biased variance over the Q*ch elements of (b, t, h)
 * x: the projection's columns (pointer at the first of them) in rows of stride ldx -- Q, K and V are one GEMM with
 * concatenated weights; y rows t in [T, Tp) are written as zeros (keys / values padded to 16-byte rows of the logits);
 * stats[h][b*T + t][2] = (mean, rstd).  ws_heads_bwd: dx (layout of x, row stride lddx) from x, dy (layout of y), the
 * statistics; slab[nwg][2*W + 8], W = Q*nh*ch: per-workgroup partial sums of d(gamma) (elements [0, W) in the order
 * (q, h, e)), d(beta) ([W, 2W)) and d(slope) ([2W, 2W + nh)) for ws_reduce_slabs; nwg = the launch grid (any > 0: the
 * sums are reproducible for a given nwg).  Workgroup i owns the rows b*T + t = i, i + nwg, ...; every slab row is
 * written whole (the 8 - nh pad words as zeros), and a workgroup that owns no row (nwg above B*T) writes a row of exact
 * zeros.  The columns of dx outside the nh*ch written stay untouched.  ch % 4 == 0, nh <= 8, W <= 9216. */
typedef struct ws_heads_args {
  const float* x;
  const float* dy;
  const float* slope;
  const float* gamma;
  const float* beta;
  float* y;
  float* stats;
  float* dx;
  float* slab;
  long long ldx, lddx;
  int B, T, Tp, Q, nh, ch, nwg;
  float eps;
} ws_heads_args;
int ws_heads_fwd(const ws_heads_args* a, void* stream);
int ws_heads_bwd(const ws_heads_args* a, void* stream);

/* Ragged speaker stage (ragged_spk.hip): enrollments of different lengths in ONE encoder pass over the
 * rectangle.  Invariant at the input of every layer: row r is exactly zero at time positions w >= W_r, its own valid
 * width there -- a convolution at w < W_r' then reads what it reads on the row alone.  Length tables are device int[R];
 * every kernel clamps the entries it reads so that none moves an access out of its row; a NULL table is WS_ERR_INVALID.
 * Zeros are selected, not multiplied: NaN / Inf behind a row's end never reach a valid output.
 * The clamp ranges: tlen[r] to [1, T] in ws_tstp_fwd_len, ws_astp_fwd_len, ws_time_mean_len and ws_cmn_len, to [0, T] in
 * ws_tail_select_len; wlen[r] to [0, W] in ws_bn_prelu_fwd_len; lengths[r] to [max(pad + 1, 2), T] in ws_preemph_pad_len.
 *   ws_bn_prelu_fwd_len  ws_bn_prelu_fwd on rows [M][C]; row m belongs to r = m / rows_per_r and sits at w = m % W
 *                        (W divides rows_per_r, rows_per_r divides M): u and y are zeros where w >= wlen[r], and bit for
 *                        bit what ws_bn_prelu_fwd writes elsewhere; x and res are not read behind wlen[r]
 *   ws_tstp_fwd_len      ws_tstp_fwd over t < tlen[r] (callers guarantee tlen[r] >= 2); F = 1: ASTP's global context
 *   ws_astp_fwd_len      ws_astp_fwd with softmax, mean and second moment over t < tlen[r]
 *   ws_time_mean_len     mean [R][C] over t < tlen[r] of x [R][T][C] (the SE squeeze)
 *   ws_cmn_len           y[r][t][:] = t < tlen[r] ? x[r][t][:] - mean_r[:] : 0, mean_r over t < tlen[r]; y may be x
 *   ws_tail_select_len   y[r][t][:] = t < tlen[r] ? x[r][t][:] : 0 on [R][T][C], C % 4 == 0; y may be x
 *   ws_preemph_pad_len   ws_preemph_pad whose reflect padding turns at lengths[r] (clamped to [max(pad + 1, 2), T]:
 *                        pre-emphasis with its reflect pad of 1 needs two samples); zeros from lengths[r] + 2 pad on up
 *                        to T + 2 pad; nothing behind the clamped lengths[r] is read */
int ws_bn_prelu_fwd_len(const float* x, const float* stats, const float* gamma, const float* beta, const float* res,
                        const float* a, long long M, int C, int rows_per_r, int W, const int* wlen, float* u, float* y,
                        void* stream);
int ws_tstp_fwd_len(const float* x, int R, int F, int T, int C, const int* tlen, float eps, float* stats, void* stream);
int ws_astp_fwd_len(const float* x, const float* logits, int R, int T, int C, const int* tlen, float floor_, float* out,
                    float* aux, void* stream);
int ws_time_mean_len(const float* x, int R, int T, int C, const int* tlen, float* mean, void* stream);
int ws_cmn_len(const float* x, int R, int T, int C, const int* tlen, float* y, void* stream);
int ws_tail_select_len(const float* x, int R, int T, int C, const int* tlen, float* y, void* stream);
int ws_preemph_pad_len(const float* x, int R, int T, int pad, int ldo, float coef, const int* lengths, float* out,
                       void* stream);

/* Ragged TF-GridNet (ragged_grid.hip): mixtures of different lengths in ONE forward over the rectangle
 * [R][Tf][Q][C].  Per-frame layers run over the rectangle unchanged; these take the row's frame count where the model
 * reduces over time, and replace per-(head, row) launch loops of the attention by one launch.  Length tables as above:
 * device int[R], clamped where read, NULL is WS_ERR_INVALID; zeros are selected, never multiplied.
 *   ws_flat_stats_len     ws_flat_stats whose group g covers its first glen[g] * per_step floats (glen[g] clamped to
 *                         [1, n_per_group / per_step]; per_step % 4 == 0 divides n_per_group): stats[g] = (mean, 1 / sqrt(
 *                         biased var + eps)) of them.  The chunked two-pass (count, mean, M2) scheme and fixed merge order
 *                         of ws_flat_stats; a group's nchunk chunks divide its own count; scratch [ngroups][nchunk][4];
 *                         nothing behind the count is read
 *   ws_ola_norm_len       frames [R][Tf][n] (windowed synthesis frames, hop = n / 2, n % 8 == 0, Tf = 1 + T / hop), win [n]
 *                         (the synthesis window) -> est [R][T]: est[r][i] = (sum over t < Tf_r of frames[r][t][i + n/2 - t hop])
 *                         / (sum over the same t of win[i + n/2 - t hop]^2) for i < lengths[r] (clamped to [0, T]), Tf_r =
 *                         1 + lengths[r] / hop; exact zeros from lengths[r] on.  The envelope is summed and inverted in
 *                         double and rounded once.  Frames t >= Tf_r are not read
 *   ws_transpose_batched  dst[g][c][r] = src[g][r][c] for G matrices in one launch (rows % 4 == 0, cols % 4 == 0; no overlap)
 *   ws_heads_merge_fwd    o[r][p][h * cp + e] = ov[h][r][p][e]: the attention's head merge, [nh][R][P][cp] -> [R][P][nh * cp]
 *                         (cp % 4 == 0; P = frames * bins of a row) */
int ws_flat_stats_len(const float* x, int ngroups, long long n_per_group, const int* glen, int per_step, float eps,
                      int nchunk, float* scratch, float* stats, void* stream);
int ws_ola_norm_len(const float* frames, const float* win, int R, int Tf, int n, int T, const int* lengths, float* est,
                    void* stream);
int ws_transpose_batched(const float* src, int G, int rows, int cols, float* dst, void* stream);
int ws_heads_merge_fwd(const float* ov, int nh, int R, long long P, int cp, float* o, void* stream);

/* Long recordings (longform.hip): one mixture x [n] as W overlapping windows of S samples, overlap O with
 * 0 <= O <= S / 2, hop H = S - O.  The layout is a pure function of (n, S, O): n <= S is one window [0, n) of L = n
 * samples; otherwise W = 1 + ceil((n - S) / H) windows of L = S samples with start_w = min(w H, n - S) -- the last window is
 * aligned to the end, so every window has full length.  The kernels compute the starts; no table of them is passed.
 * NULL x / rows / y / out, an overlap outside [0, S / 2] and a W that is not the one of (n, S, H) are WS_ERR_INVALID
 * before any launch.  Offsets are 64-bit (n up to 2^31 - 1).
 *   ws_window_rows  rows[(k W + w)][j] = x[start_w + j] * (scale ? scale[w] : 1), k < reps, j < L: every window once per
 *                   target speaker.  No alignment of the starts is assumed.  scale: device [W] or NULL (the runtime's
 *                   TF-GridNet plan scales a window by 1 / its standard deviation)
 *   ws_xfade_ola    y [K][W][L] -> out [K][n].  Window w weighs its local sample j with
 *                     g_w(j) = (w > 0 ? min(1, (j + 1) / (O + 1)) : 1) * (w < W - 1 ? min(1, (L - j) / (O + 1)) : 1)
 *                   and out[k][i] = (sum over the windows that cover i, ascending w, of g_w y (* scale[w])) / (sum of the
 *                   same g_w).  Two regular neighbours' ramps add up to 1: a linear cross-fade.  The end-aligned last
 *                   window may overlap its predecessor by up to S - 1 samples and a third window with it; the division
 *                   covers that (every g > 0; at most ceil(S / H) + 1 terms).  Fixed order, no atomics; every out[k][i],
 *                   i < n, is written; y is read inside [0, L) of a window only.  scale: device [W] or NULL */
int ws_window_rows(const float* x, int n, int W, int S, int H, int reps, const float* scale, float* rows, void* stream);
int ws_xfade_ola(const float* y, int K, int W, int S, int O, int n, const float* scale, float* out, void* stream);

/* Live windows (longform.hip; runtime/live.cc) -- a new symbol, ABI 20 unchanged.  ws_xfade_ola over the absolute
 * sample positions [i0, i0 + count) of a recording whose windows arrive one by one:
 *   ring [K][cap][S]   window w's estimate in slot w % cap;  scale_ring [cap] or NULL: its factor, in the same slot
 *   windows_run        the regular windows 0 .. windows_run - 1 (start w H) have been written
 *   final == 0         no last window exists yet: every covering window is regular with its tail ramp, no end-aligned term is
 *                      added, and the range must end at or before (windows_run - 1) H -- the start of the newest window, behind
 *                      which every later window, regular or end-aligned, starts.  W and n are ignored
 *   final != 0         the layout of ws_xfade_ola for (n, S, O) with its W windows, all run (windows_run == W): the end-aligned
 *                      last window sits in slot (W - 1) % cap; n < S is the one short window of L = n samples in slot 0
 *   out [K][ld_out]    out[k][i - i0], ld_out >= count
 * The per-sample arithmetic is the body ws_xfade_ola inlines (same weights, ascending w, num / den), so the concatenated
 * ranges equal ws_xfade_ola on the same estimates bit for bit.  One thread per output sample, 64-bit window and sample indices,
 * no atomics; a slot is read only for a window that covers the sample.  WS_ERR_INVALID before any launch: NULL ring / out, O
 * outside [0, S / 2], count < 0 (count == 0 launches nothing), a range past the windows run unless final, a final (W, n) that
 * is not the layout or not all run, and a cap that does not hold the windows the range reads (they must be among the newest
 * cap). */
int ws_xfade_stream_fwd(const float* ring, int K, int cap, int S, int O, const float* scale_ring, long long i0, long long count,
                        long long windows_run, int final, long long W, long long n, float* out, long long ld_out, void* stream);

/* Live pool (longform.hip; runtime/live_pool.cc, DESIGN 7 "Live pool") -- new symbols, ABI 20 unchanged.  The rows forms of the
 * gather and of the ring cross-fade: ONE launch for A table rows that share nothing but the launch, with the two-table
 * convention of ws_rows_copy_fwd -- `rows` is a HOST pointer, validated, and sizes the grid; `d_rows` is a DEVICE pointer to the
 * same bytes, uploaded by the caller on the same stream before the call.  Offsets count floats into arenas whose lengths are
 * arguments.  Grid (blocks of the largest row, A); a workgroup beyond its own row's count leaves at once.  Plain C++, no packed
 * FP32, no atomics, 64-bit offsets, no LDS.
 *   ws_window_slots_fwd  row i: dst[dst_off + j] = fl(src[src_off + j] * scale), j < len -- ws_window_rows with the start, the
 *                   destination and the factor taken from the table (scale = 1: a copy).  Sources are read with scalar loads
 *                   (no start alignment is assumed), a destination quad is stored as 16 bytes where its address allows.  A row
 *                   equals bit for bit what ws_window_rows writes for that window.
 *   ws_xfade_stream_rows_fwd  row i is ws_xfade_stream_fwd with K = 1 for one target of one slot: its ring [cap][S] at
 *                   ring + ring_off, its factor ring [cap] at scale_ring + scale_off (scale_off = -1: none), and `count`
 *                   samples from position i0 written to out + out_off, with (windows_run, final, W, n) as in the solo call --
 *                   the short final window n < S included.  Every sample comes from the one cross-fade body with exactly the
 *                   arguments the solo call derives, so a row is bit for bit the solo call.  A row with count == 0 is skipped
 *                   (a call whose rows are all empty launches nothing).  S, O and cap are shared by the rows.
 * WS_ERR_INVALID before any launch, each with the row index: every check of the solo entry point, per row; a range that leaves
 * its arena; a dst / out range that overlaps any other range of the call (by address); and A outside [1, 65535], a NULL
 * pointer (scale_ring may be NULL when no row names a factor ring). */
typedef struct ws_window_slot_row {
  long long src_off, dst_off;
  int len;
  float scale;
} ws_window_slot_row;
typedef struct ws_xfade_stream_row {
  long long ring_off, scale_off, out_off, i0, count, windows_run, W, n;
  int final;
} ws_xfade_stream_row;
int ws_window_slots_fwd(const ws_window_slot_row* rows, const ws_window_slot_row* d_rows, int A, const float* src, long long n_src,
                        float* dst, long long n_dst, void* stream);
int ws_xfade_stream_rows_fwd(const ws_xfade_stream_row* rows, const ws_xfade_stream_row* d_rows, int A, int S, int O, int cap,
                             const float* ring, long long n_ring, const float* scale_ring, long long n_scale, float* out,
                             long long n_out, void* stream);

/* Tail pool (longform.hip; runtime/tail_pool.cc, DESIGN 7 "Tail pool") -- a new symbol, ABI 20 unchanged.  The emission of one
 * tick as ONE launch, in the rows form and with the two-table convention above.  Row i is one target of one slot: of its
 * window's estimate y [L] at y + y_off it emits the m samples from local index p on, and holds the last c_new samples back for
 * the next window to cross-fade into.  With v = fl(y * scale) (scale exactly 1: y itself), the roundings spelled out as the
 * cross-fade body of ws_xfade_ola spells its own and contraction off:
 *     out[out_off + j]       = j < h ? fma(ramp[j], fl(v - hold[hold_in_off + j]), hold[hold_in_off + j]) : v,     j < m
 *     hold[hold_out_off + q] = fl(y[y_off + p + m + q] * scale),                                                 q < c_new
 * ramp [C] is the caller's, ramp[j] = float(j + 1) / float(C + 1) in the tail pool; h and c_new are 0 or C.  A row's new hold
 * is another buffer than the one it reads (the caller double-buffers), so no thread reads what another thread of the launch
 * writes.  Grid (blocks of the largest m + c_new, A); a workgroup beyond its own row's count leaves at once; a thread owns four
 * consecutive floats of one destination counted from the 16-byte boundary below its first float, so whole quads are stored as
 * 16 bytes wherever a destination starts; sources are read with scalar loads.  64-bit offsets, no LDS, no atomics, plain C++.
 * WS_ERR_INVALID before any launch, each with the row index: A outside [1, 65535]; a NULL pointer (ramp may be NULL when
 * C == 0); C < 0; h or c_new that is neither 0 nor C; h > m; p < 0; p + m + c_new != L; m + c_new < 1; a range that leaves its
 * arena; an out or hold_out range that overlaps any other range of the call (by address), so also a hold_in range that meets a
 * hold_out range. */
typedef struct ws_tail_emit_row {
  long long y_off, hold_in_off, hold_out_off, out_off;
  int L, p, h, m, c_new;
  float scale;
} ws_tail_emit_row;
int ws_tail_emit_rows_fwd(const ws_tail_emit_row* rows, const ws_tail_emit_row* d_rows, int A, int C, const float* ramp,
                          const float* y, long long n_y, float* hold, long long n_hold, float* out, long long n_out, void* stream);

/* ---- streaming Conv-TasNet (stream.hip; wesep_amd/streaming.py) -- new symbols, ABI 20 unchanged --------
 * The two kernels of a causal Conv-TasNet that look across time, in a chunked form with state carried on the device.
 *   ws_dwconv_stream_fwd  ws_dwconv_ex_fwd(causal = 1) on one chunk of Tc frames whose first frame has absolute index t0.
 *                   x [R][Tc][C] is the pre-norm activation, normalised on load with statistics row m / st_div over the
 *                   chunk's rows (cLN: 1; eval-mode BN: identity statistics, st_div = R * Tc).  ring [R][cap][C] holds the
 *                   NORMALISED frame of absolute index a in slot a % cap.
 *                     y[r][t][c] = b[c] + sum_p w[c][p] * xn(r, t0 + t - (P - 1 - p) * dil),  ascending p,
 *                   xn(a) = the chunk's own value for a >= t0, the ring slot for 0 <= a < t0, and no term for a < 0 (the
 *                   ring is not read there: it needs no initialisation).  The same launch writes every chunk frame's
 *                   normalised value to its slot.  Contract: cap >= (P - 1) * dil + Tc -- then the slot written for frame
 *                   a last held frame a - cap, which no output of this chunk reads, and the launch is race-free without a
 *                   second buffer.  Over any chunking the outputs are bit for bit ws_dwconv_ex_fwd(causal = 1) on the
 *                   concatenated sequence (given the same statistics).  WS_ERR_INVALID before any launch: cap below the
 *                   bound, C % 4 != 0, P not odd or above 7, t0 < 0, a NULL pointer, y overlapping x.
 *   ws_ola_stream_fwd  frames [R][Tc][L] -> est [R][Tc * hop], carry [R][L - hop] updated in place.  carry holds, for the
 *                   L - hop samples that are not final yet, bias + the contributions of earlier frames, accumulated in
 *                   ascending frame order (the association of ws_ola_fwd).  The call emits the Tc * hop samples that become
 *                   final and leaves the new carry; samples past the old carry start from bias[0] (NULL: 0).  A reset fills
 *                   carry with the bias; after the last chunk, carry is the last L - hop samples.  The concatenation is bit
 *                   for bit ws_ola_fwd over all frames with Tout = (T' - 1) * hop + L.  Any L >= hop with L % hop == 0
 *                   (L - hop <= 16384; carry may be NULL when L == hop). */
int ws_dwconv_stream_fwd(const float* x, const float* stats, const float* gamma, const float* beta, const float* w,
                         const float* b, int R, int Tc, int C, int P, int dil, int st_div, long long t0, int cap,
                         float* ring, float* y, void* stream);
int ws_ola_stream_fwd(const float* frames, const float* bias, int R, int Tc, int L, int hop, float* carry, float* est,
                      void* stream);
/*   ws_tcn_mid_stream_fwd  everything between the two GEMMs of a causal cLN block on one chunk, in ONE launch (in place of
 *                   ws_prelu_fwd, ws_group_stats, ws_dwconv_stream_fwd, ws_prelu_fwd, ws_group_stats).  c [R][Tc][H] is the
 *                   first 1x1 convolution's output for the frames t0 .. t0 + Tc - 1 (read only), rb [R][H] the concatConv
 *                   row bias or NULL.  For row r, chunk frame t:
 *                     y1 = prelu(c[r][t][:] + rb[r][:], a1[0]);  (m1, s1) = mean and 1 / sqrt(biased var + eps) of y1 over H
 *                     (two passes, as ws_group_stats);  xn(r, t0 + t) = (y1 - m1) * s1 * gamma1 + beta1, written to
 *                     ring[r][(t0 + t) % cap][:];  z = bd + sum_p wd[ch][p] * xn(r, t0 + t - (P - 1 - p) * dil), ascending p,
 *                     with the tap rules of ws_dwconv_stream_fwd (chunk frames from the chunk -- recomputed from c, never read
 *                     from the ring --, 0 <= a < t0 from slot a % cap, a < 0 no term and no read);
 *                     y2[r][t][:] = prelu(z, a2[0]);  st2[r * Tc + t] = (mean, rstd) of y2 over H.
 *                   The block's second GEMM normalises on load from st2.  Contract: cap >= (P - 1) * dil + Tc (race-free, as
 *                   above), and over any chunking y2, st2 and the written ring slots are bit for bit those of one chunk with
 *                   the whole sequence: a frame's xn is one expression reduced in one fixed order (inside a wave, then across
 *                   waves through LDS) wherever it is computed.  No atomics, nothing waits on another workgroup; results are
 *                   the same from run to run.  WS_ERR_INVALID before any launch: a NULL pointer other than rb, H % 4 != 0,
 *                   H above WS_TCN_MID_MAXH (2 H + 16 floats of LDS per workgroup), P not odd or above 7, dil < 1, t0 < 0, cap
 *                   below the bound, y2 overlapping c (other frames' workgroups re-read c). */
#define WS_TCN_MID_MAXH 4096
int ws_tcn_mid_stream_fwd(const float* c, const float* rb, const float* a1, const float* gamma1, const float* beta1,
                          const float* wd, const float* bd, const float* a2, int R, int Tc, int H, int P, int dil,
                          float eps, long long t0, int cap, float* ring, float* y2, float* st2, void* stream);
/* ---- stream pool (stream.hip; runtime/stream_pool.cc) -- new symbols, ABI 20 unchanged -------------------
 * The two kernels above for MANY independent streams in one launch: every stream at its own position, with its own number
 * of new frames.  Data rows are compact, state is addressed by slot: row i of the [A][Tc] rectangle belongs to the stream
 * whose state is row slot[i] of the [nslots] state arrays.  Three DEVICE tables of A entries, one entry per row:
 *   slot [A] int        0 <= slot[i] < nslots
 *   t0   [A] long long  absolute index of the row's first frame in this launch
 *   tc   [A] int        valid frames of the row in this launch, 0 <= tc[i] <= Tc
 * As for every length table of this header, an entry can never move an access out of its buffer: an out-of-range slot or a
 * negative t0 skips the row (it is treated as tc[i] = 0: its outputs are the zeros below, no state row is touched), tc is
 * clamped to [0, Tc].  Distinct rows naming the same slot would race on its state: that is the caller's contract (the
 * engine checks it on the host).  State rows of slots that no entry names are neither read nor written.
 *   ws_tcn_mid_stream_rows_fwd  ws_tcn_mid_stream_fwd with c [A][Tc][H], rb [nslots][H] (read at slot[i]) or NULL, ring
 *                   [nslots][cap][H], y2 [A][Tc][H], st2 [A][Tc][2].  One workgroup per (i, t), the same number of threads
 *                   (a function of H alone), the same expressions in the same order: frame t < tc[i] of row i -- y2, st2
 *                   and the ring slot it writes -- is bit for bit what ws_tcn_mid_stream_fwd(R = 1, Tc = tc[i], t0 = t0[i])
 *                   gives on that row's c, rb[slot[i]] and ring row.  A tap inside the chunk is recomputed from c only for
 *                   frames below tc[i]; everything earlier comes from the ring.  A frame t >= tc[i] gets exact zeros in y2
 *                   and (0, 1) in st2 (a norm-on-load GEMM behind it stays finite) and writes no ring slot; c behind tc[i]
 *                   is never read into a valid output (NaN included).  Contract: cap >= (P - 1) * dil + Tc.
 *                   WS_ERR_INVALID before any launch: as ws_tcn_mid_stream_fwd, and A < 1, nslots < 1, a NULL table.
 *   ws_ola_stream_rows_fwd  ws_ola_stream_fwd with frames [A][Tc][L], carry [nslots][L - hop], est [A][Tc * hop].  Row i
 *                   emits the tc[i] * hop samples that become final after tc[i] frames, exact zeros behind them up to the
 *                   row pitch Tc * hop, and leaves carry[slot[i]] as ws_ola_stream_fwd(R = 1, Tc = tc[i]) would -- the
 *                   additions in ascending frame order, so bit for bit.  With tc[i] = 0 the carry row is neither read nor
 *                   written.  frames behind tc[i] are not read.  WS_ERR_INVALID before any launch: as ws_ola_stream_fwd, and
 *                   A < 1, nslots < 1, a NULL table. */
int ws_tcn_mid_stream_rows_fwd(const float* c, const float* rb, const float* a1, const float* gamma1, const float* beta1,
                               const float* wd, const float* bd, const float* a2, int A, int Tc, int H, int P, int dil,
                               float eps, int nslots, const int* slot, const long long* t0, const int* tc, int cap,
                               float* ring, float* y2, float* st2, void* stream);
int ws_ola_stream_rows_fwd(const float* frames, const float* bias, int A, int Tc, int L, int hop, int nslots,
                           const int* slot, const long long* t0, const int* tc, float* carry, float* est, void* stream);

/* ---- the whole block (stream_block.hip; DESIGN section 7, "The whole block") -- new symbols, ABI 20 unchanged ---------------
 *   ws_tcn_block_stream_fwd  a whole causal cLN block on one chunk in ONE launch, in place of ws_gemm_nt, ws_tcn_mid_stream_fwd
 *                   and ws_gemm_nt.  x [R][Tc][B] is the block input for the frames t0 .. t0 + Tc - 1, W1 [H][ldw1] is read in
 *                   its first B columns only (the concatConv block passes ldw1 = B + E; its embedding half is the row bias
 *                   rb [R][H]), W2 is [B][H], ring [R][cap][H] as for ws_tcn_mid_stream_fwd.  For row r, chunk frame t with
 *                   absolute index a = t0 + t:
 *                     c   = W1[:, :B] . x[r][t] + (rb ? rb[r] : b1)
 *                     y1  = prelu(c, a1[0]);  (m1, s1) = mean, 1 / sqrt(biased var + eps) of y1 over H   (two passes)
 *                     xn(a) = (y1 - m1) * s1 * gamma1 + beta1              -> ring[r][a % cap][:]
 *                     z   = bd + sum_p wd[ch][p] * xn(a - (P - 1 - p) * dil),  ascending p, the tap rules of
 *                           ws_dwconv_stream_fwd (a' < 0: no term and no read; 0 <= a' < t0: ring slot a' % cap; a' >= t0: a
 *                           chunk frame, never taken from a ring slot that another workgroup of the launch writes)
 *                     y2  = prelu(z, a2[0]);  (m2, s2) of y2 over H
 *                     out[r][t] = x[r][t] + (b2 + W2 . ((y2 - m2) * s2 * gamma2 + beta2))
 *                   One workgroup per row walks the row's frames in tiles of 8, in order; a weight pass is shared by a
 *                   tile's frames; a tap before the tile is read from the ring, which holds what an earlier launch or this
 *                   same workgroup wrote.  Each dot product of a frame is one fp32 accumulator started at 0 and advanced by
 *                   fmaf in ascending k, the bias added last; statistics are reduced per thread (channels i, i + 256, ...),
 *                   per wave, then over the four waves in ascending order.  So out[r][t] and the ring slot a frame leaves are
 *                   the same BITS under any chunking of the sequence (one chunk with all of it included), any position of the
 *                   frame in a chunk or tile, any R and whatever the other rows hold, and from run to run.  No atomics,
 *                   nothing waits on another workgroup.  Contract: cap >= (P - 1) * dil + Tc.  out may not overlap x; x, the
 *                   weights and rb are read only.  WS_ERR_INVALID before any launch: a NULL pointer other than rb and b1
 *                   (exactly one of the two must be given), B % 4, H % 4 or ldw1 % 4 non-zero, ldw1 < B, H above
 *                   WS_TCN_BLOCK_MAXH or B above WS_TCN_BLOCK_MAXB (8 (B + H) + 4192 floats of LDS per workgroup), P not odd
 *                   or above 7, dil < 1, t0 < 0, cap below the bound, out overlapping x.
 *   ws_tcn_block_stream_rows_fwd  the same for the rows of a stream pool, with the three device tables and the exact
 *                   semantics of ws_tcn_mid_stream_rows_fwd: x [A][Tc][B], rb [nslots][H] (read at slot[i]) or NULL, ring
 *                   [nslots][cap][H], out [A][Tc][B].  One workgroup per row i runs the solo form's body (one shared inline
 *                   function) on (tc[i], t0[i], rb and ring row slot[i]): a valid frame and the ring slot it leaves are bit
 *                   for bit those of ws_tcn_block_stream_fwd(R = 1, Tc = tc[i], t0 = t0[i]).  An out-of-range slot or a
 *                   negative t0 is treated as tc[i] = 0, tc is clamped to [0, Tc]; frames t >= tc[i] write exact zeros to
 *                   out and touch no state; x behind tc[i] is never read (NaN there reaches nothing).  WS_ERR_INVALID before
 *                   any launch: as above (no t0 argument), and A < 1, nslots < 1, a NULL table. */
#define WS_TCN_BLOCK_MAXH 768
#define WS_TCN_BLOCK_MAXB 512
int ws_tcn_block_stream_fwd(const float* x, const float* rb, const float* W1, int ldw1, const float* b1, const float* a1,
                            const float* gamma1, const float* beta1, const float* wd, const float* bd, const float* a2,
                            const float* gamma2, const float* beta2, const float* W2, const float* b2, int R, int Tc, int B,
                            int H, int P, int dil, float eps, long long t0, int cap, float* ring, float* out, void* stream);
int ws_tcn_block_stream_rows_fwd(const float* x, const float* rb, const float* W1, int ldw1, const float* b1, const float* a1,
                                 const float* gamma1, const float* beta1, const float* wd, const float* bd, const float* a2,
                                 const float* gamma2, const float* beta2, const float* W2, const float* b2, int A, int Tc,
                                 int B, int H, int P, int dil, float eps, int nslots, const int* slot, const long long* t0,
                                 const int* tc, int cap, float* ring, float* out, void* stream);

/* ---- sample rates (resample.hip; DESIGN section 7, "Sample rates") -- new symbols, ABI 20 unchanged -------------------------
 * Polyphase windowed-sinc rate conversion: the published sinc_interp_hann design with lowpass_filter_width = 6 and
 * rolloff = 0.99.  For rate_in -> rate_out: g = gcd, D = rate_in / g, U = rate_out / g, base = min(D, U) * 0.99,
 * w = ceil(6 D / base), K = 2 w + D.  The tap table taps[p][k], p < U, k < K, is computed in double and rounded to float once:
 *   t = clamp((-p / U + (k - w) / D) * base, -6, 6);   taps[p][k] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos^2(pi t / 12) * base / D
 * and  y[q] = sum_{k < K} taps[q % U][k] * x[(q / U) * D + k - w]  for q < ceil(U n_in / D), x = 0 outside [0, n_in).
 *   ws_resample_geom  (U, D, w, K) of a pair of rates.  Host code.
 *   ws_resample_taps  the table, HOST float [U][K].  Host code in double; the ONE place the table is made (the engine and
 *                   the Python binding both call it and upload the result).
 *   ws_resample_fwd   the whole signal: x [R][ldx] with n_in >= 1 valid samples a row -> y [R][ldy], ceil(U n_in / D) samples
 *                   a row; taps: the DEVICE copy of the table.  Nothing behind n_in is read (NaN included), nothing behind
 *                   the last output is written.  Rows have any pitch.
 *   ws_resample_stream_fwd  the same filter on a stream's buffer buf [R][ldb] = history | new samples, n_valid >= 1 valid
 *                   samples a row.  Groups of U outputs are numbered from the buffer: group g reads buf[g D - lead + k],
 *                   k < K -- lead (0 <= lead <= w) is the number of taps of group 0 that lie before buf[0], which is sample 0
 *                   of the signal when lead > 0.  The call writes n_out outputs, starting at phase 0 of group g_first, to
 *                   y [R][ldy].  final = 0: every tap of every output must fall on a valid sample (refused otherwise);
 *                   final = 1: the signal ends at n_valid, taps behind it are skipped (the zero extension of the whole-signal
 *                   form), and outputs past ceil(U (n_valid + lead - w) / D) are refused.  The same launch copies
 *                   buf[r][hist_from .. hist_from + hist_len) to hist [R][ldh] (another buffer; hist_len = 0: none) -- the
 *                   history of the next call; n_out = 0 with hist_len > 0 only moves the history.
 * One thread owns one output sample of one row: ONE fp32 accumulator started at 0 and advanced by fmaf in ascending k over
 * the taps that fall on valid samples -- a tap before sample 0 or behind the end is skipped, not multiplied.  Both forms run
 * the same device function on buffer-relative int offsets; nothing depends on the grid, R, the chunk or the position.  So an
 * output sample has the same BITS in the whole-signal call, under any chunking of the streaming call, alone or beside other
 * rows, and from run to run.  No atomics.  The caller keeps 64-bit sample and group counters.
 * Streaming emission rule (wesep_amd/resample.py StreamResampler, runtime/rate.cc): group g is final once g D + w + D <= N, so
 * after N input samples U max(0, floor((N - w) / D)) outputs have been returned; the flush returns the rest up to
 * ceil(U N / D).  The history a stream keeps is the input from max(0, G D - w) on, G the groups returned: fewer than K samples.
 * A table of U K <= 2048 floats is staged in LDS per workgroup; a larger one (44.1 kHz, 22.05 kHz) is read from global
 * memory through the caches.  WS_ERR_INVALID before any launch, by name: a NULL pointer, rates <= 0, U or D above
 * WS_RESAMPLE_MAX_UD, K above WS_RESAMPLE_MAX_K, R outside [1, 65535], n_in / n_valid < 1, a row pitch below its row, offsets
 * reaching 2^31, lead outside [0, w], a history range outside the valid samples or overlapping buf, outputs beyond what the
 * valid samples allow. */
#define WS_RESAMPLE_MAX_UD 1024
#define WS_RESAMPLE_MAX_K 4096
int ws_resample_geom(int rate_in, int rate_out, int* U, int* D, int* w, int* K);
int ws_resample_taps(int rate_in, int rate_out, float* taps);
int ws_resample_fwd(const float* x, long long ldx, int R, int n_in, int rate_in, int rate_out, const float* taps, float* y,
                    long long ldy, void* stream);
int ws_resample_stream_fwd(const float* buf, long long ldb, int R, int rate_in, int rate_out, const float* taps, int lead,
                           int n_valid, int final, int g_first, int n_out, float* y, long long ldy, int hist_from, int hist_len,
                           float* hist, long long ldh, void* stream);

/* Rows forms (new symbols, ABI 20 unchanged): ONE launch for A rows that share nothing but the launch.
 *   ws_resample_stream_rows_fwd  row i is ws_resample_stream_fwd with R = 1 on its own geometry, table, buffer, position,
 *                   output range and history destination, all named by its descriptor rows[i]:
 *                     buf + in_off    the row's `history | new samples`, n_valid valid ones
 *                     taps + taps_off its table [U][K], any table that ws_resample_taps made, or the identity U = D = K = 1
 *                                     with the one tap 1.0f (y = the input samples, bit for bit: the container's own rate)
 *                     y + out_off     n_out outputs from phase 0 of group g_first
 *                     hist + hist_off buf[in_off + hist_from .. + hist_len)
 *                   with U, D, K explicit (w = (K - D) / 2) and lead, n_valid, final, g_first, n_out, hist_from, hist_len as
 *                   in the solo call.  Offsets count floats into four arenas whose lengths are arguments.  The table comes
 *                   twice: `rows`, a HOST pointer, is validated and sizes the grid; `d_rows` is a DEVICE pointer to the same
 *                   bytes, uploaded by the caller on the same stream before the call (the convention of slot / t0 / tc above).
 *                   Every row runs the device function of the two calls above, so its outputs and history are bit for bit
 *                   what ws_resample_stream_fwd gives with R = 1 and the same arguments, whatever the other rows are.  Grid
 *                   (max_i(nb_out_i + nb_hist_i), A); a workgroup beyond its row's count leaves before any barrier.  A row
 *                   with U K <= 2048 stages its table in LDS (8 KB of dynamic LDS when any row does), another row of the
 *                   same launch reads its table from global memory.  No atomics.  WS_ERR_INVALID before any launch, each
 *                   with the row index: every check of ws_resample_stream_fwd, and U or D outside [1, WS_RESAMPLE_MAX_UD],
 *                   K outside [1, WS_RESAMPLE_MAX_K], K < D, K - D odd, a range that leaves its arena, a y or hist range
 *                   that overlaps any other range of the call (by address: the arenas may be parts of one allocation);
 *                   A outside [1, 65535], a NULL pointer.
 *   ws_rows_copy_fwd  row i: dst[dst_off + j] = src[src_off + j], j < len, then `fill` zeros behind them.  Pure data
 *                   movement (a gather of per-slot samples into a rectangle, or the scatter back); the same two-table
 *                   convention.  WS_ERR_INVALID before any launch, with the row index: len or fill negative or both 0, a range
 *                   that leaves its arena, a dst range that overlaps any other range of the call.
 *   ws_window_resample_rows_fwd  (a new symbol, ABI 20 unchanged) the gather of a rate tail pool (runtime/rate_tail_pool.cc): row
 *                   i is L consecutive outputs of the whole-signal filter that start at ANY phase, computed from the span of
 *                   the input that their taps cover.  Its descriptor names
 *                     buf + in_off    the span, n_valid valid samples, numbered as a stream's buffer is: group g of the buffer
 *                                     reads buf[in_off + g D - lead + k], k < K; lead in [0, w] is the number of taps of group
 *                                     0 that lie before the span, which starts at sample 0 of the signal when lead > 0
 *                     taps + taps_off its table [U][K] (or the identity U = D = K = 1), U, D, K explicit, w = (K - D) / 2
 *                     g_first, p_first  the first output: phase p_first in [0, U) of the buffer's group g_first
 *                     y + out_off     the L outputs, then `fill` zeros
 *                     final           0: every tap of every output must fall on a valid sample; 1: the signal ends at
 *                                     n_valid and taps behind it are skipped
 *                   Output j is resample_one -- the device function of every call above -- on output g_first U + p_first + j of
 *                   the buffer's numbering: with the buffer's group 0 the signal's group G0, the BITS ws_resample_fwd gives
 *                   for output (G0 + g_first) U + p_first + j of the whole signal (final = 1: of the signal that ends with
 *                   the span).  Nothing behind n_valid is read (NaN there reaches nothing), nothing behind L + fill is
 *                   written.  Rows may share a span.  Grid (max_i ceil((L_i + fill_i) / 256), A); the tables as above (U K <=
 *                   2048 floats: staged in LDS; larger: global memory); 64-bit offsets, no atomics, plain C++; the two-table
 *                   convention.  WS_ERR_INVALID before any launch, each with the row index: U, D, K, lead, g_first as for
 *                   ws_resample_stream_rows_fwd; p_first outside [0, U); n_valid < 1, L or fill negative or both 0; with
 *                   final = 0 an output whose taps fall behind n_valid, with final = 1 outputs past ceil(U (n_valid + lead -
 *                   w) / D); offsets reaching 2^31; a range that leaves its arena; a y range that meets any other range of
 *                   the call; A outside [1, 65535]; a NULL pointer. */
typedef struct ws_resample_row {
  long long in_off, taps_off, out_off, hist_off;
  int U, D, K;
  int lead, n_valid, final, g_first, n_out, hist_from, hist_len;
} ws_resample_row;
typedef struct ws_rows_copy_row {
  long long src_off, dst_off;
  int len, fill;
} ws_rows_copy_row;
typedef struct ws_window_resample_row {
  long long in_off, taps_off, out_off;
  int U, D, K;
  int lead, n_valid, final, g_first, p_first, L, fill;
} ws_window_resample_row;
int ws_resample_stream_rows_fwd(const ws_resample_row* rows, const ws_resample_row* d_rows, int A, const float* buf,
                                long long n_buf, const float* taps, long long n_taps, float* y, long long n_y, float* hist,
                                long long n_hist, void* stream);
int ws_rows_copy_fwd(const ws_rows_copy_row* rows, const ws_rows_copy_row* d_rows, int A, const float* src, long long n_src,
                     float* dst, long long n_dst, void* stream);
int ws_window_resample_rows_fwd(const ws_window_resample_row* rows, const ws_window_resample_row* d_rows, int A, const float* buf,
                                long long n_buf, const float* taps, long long n_taps, float* y, long long n_y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WESEP_HIP_H_ */
