// engine_internal.h -- private header of libwesep_engine.so (include/wesep_engine.h is the public C ABI).
//
// The runtime is one translation unit per part:
//   engine.cc        weight container, arena helpers, shared launch helpers, load dispatch by meta "arch", the C ABI
//   speaker.cc       speaker stage: kaldi fbank / MelSpectrogram front-ends, ResNet / ECAPA-TDNN / CAM++ encoders,
//                    their pooling layer, SpeakerTransform
//   bsrnn_plan.cc    pBSRNN (arch 0)
//   tasnet_plan.cc   Conv-TasNet / SpEx+ (arch 1)
//   dpccn_plan.cc    DPCCN (arch 2)
//   gridnet_plan.cc  TF-GridNet (arch 3)
//   longform.cc      ws_engine_separate_long: one long mixture as overlapping windows through the rectangular plans
//   live.cc          ws_engine_live_*: the windows of ws_engine_separate_long run as their samples arrive, any architecture
//   live_pool.cc     ws_engine_live_pool_*: many live recordings, the windows one push completes in the same forwards
//   tail_pool.cc     ws_engine_tail_pool_*: many live recordings on their trailing windows, fired by the caller's tick
//   rate_tail_pool.cc  ws_engine_rate_tail_pool_*: the tail pool with a sample rate per slot
//   stream.cc        what every streaming front end shares -- the launch chain of a group of frames (stream_chain), the state
//                    block (StreamCore) and the speaker stage of a stream (stream_enroll) -- and ws_engine_stream_*: causal
//                    cLN Conv-TasNet fed audio as it arrives, state carried on the device
//   stream_pool.cc   ws_engine_pool_*: many such streams, each at its own position, through one launch chain per round; the
//                    slot checks of both pools
//   rate.cc          audio at the caller's sample rate: ws_engine_resample, ws_engine_separate_rate, ws_engine_rate_stream_*
//   rate_pool.cc     ws_engine_rate_pool_*: the stream pool with a sample rate per slot, on the rows forms of the resampler
// The emission rule of all four (Geom, plan_step, plain_emitted, ...) and their copy / synchronise helpers are below.
// Everything here lives in namespace wsrt and is built with -fvisibility=hidden: the library exports the C ABI only
// (WS_ENGINE_API).  Host code only: no kernels in the runtime.
#ifndef WESEP_ENGINE_INTERNAL_H_
#define WESEP_ENGINE_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../include/wesep_engine.h"
#include "../include/wesep_hip.h"

#define WS_ENGINE_API extern "C" __attribute__((visibility("default")))

namespace wsrt {

constexpr int kN = 128;                 // feature_dim
constexpr int kH = 256;                 // LSTM hidden size
constexpr int kG4 = 4 * kH;             // gate rows per direction
constexpr int kNBin = 257;              // n_fft / 2 + 1
constexpr int kHop = 128;
constexpr int kBig = 1 << 30;           // row divisor meaning "never wraps"
constexpr int kDpBins = 257;            // DPCCN: n_fft / 2 + 1
constexpr float kGnEps = 1.1920928955078125e-07f;   // torch.finfo(float32).eps, bsrnn.py:23
constexpr float kBnEps = 1e-5f;
constexpr float kLnEps = 1e-5f;

struct Tensor {
  std::vector<int64_t> dims;
  size_t off = 0;   // floats into the weight blob
  size_t n = 0;
};

void set_err(const char* fmt, ...);

// ---- device memory: chunked bump allocator with stack discipline --------------------------------------------
struct Arena {
  struct Chunk {
    char* base;
    size_t cap;
  };
  std::vector<Chunk> chunks;
  size_t cur = 0, top = 0;      // current chunk and offset inside it
  size_t live_bytes = 0, peak_bytes = 0;
  bool dry = false;
  bool poison = getenv("WS_ENGINE_POISON") != nullptr;

  struct Mark {
    size_t cur, top, live;
  };

  static size_t round_up(size_t b) { return (b + 255) & ~size_t(255); }

  bool add_chunk(size_t bytes) {
    Chunk c{nullptr, bytes};
    if (dry) {
      c.base = static_cast<char*>(malloc(bytes));
    } else if (hipMalloc(reinterpret_cast<void**>(&c.base), bytes) != hipSuccess) {
      c.base = nullptr;
    }
    if (!c.base) return false;
    chunks.push_back(c);
    return true;
  }

  float* alloc(size_t nfloats) {
    const size_t bytes = round_up(nfloats * 4 + 4);
    while (true) {
      if (cur < chunks.size() && top + bytes <= chunks[cur].cap) break;
      if (cur + 1 < chunks.size()) {           // move on to the next existing chunk
        ++cur;
        top = 0;
        continue;
      }
      const size_t want = bytes > (size_t(256) << 20) ? bytes : (size_t(256) << 20);
      if (!add_chunk(want)) {
        set_err("engine: device allocation of %zu bytes failed", want);
        return nullptr;
      }
      cur = chunks.size() - 1;
      top = 0;
    }
    float* p = reinterpret_cast<float*>(chunks[cur].base + top);
    // WS_ENGINE_POISON=1 (tests): every allocation starts as NaN (0xFF bytes), so a launch plan that reads memory no
    // kernel has written shows up as NaN output instead of depending on what the arena held before (device-wide
    // syncs around it: the engine's stream is non-blocking).
    if (poison && !dry) {
      (void)hipDeviceSynchronize();
      (void)hipMemset(p, 0xFF, bytes);
      (void)hipDeviceSynchronize();
    }
    top += bytes;
    live_bytes += bytes;
    if (live_bytes > peak_bytes) peak_bytes = live_bytes;
    return p;
  }

  Mark mark() const { return Mark{cur, top, live_bytes}; }
  void release(const Mark& m) {
    cur = m.cur;
    top = m.top;
    live_bytes = m.live;
  }
  void reset() {
    cur = 0;
    top = 0;
    live_bytes = 0;
  }
  // after a forward that had to add chunks: one chunk of the peak size for the next call
  void consolidate() {
    if (chunks.size() <= 1 || live_bytes != 0) return;
    const size_t want = round_up(peak_bytes + (size_t(16) << 20));
    free_all();
    add_chunk(want);
  }
  void free_all() {
    for (auto& c : chunks) {
      if (dry)
        free(c.base);
      else
        (void)hipFree(c.base);
    }
    chunks.clear();
    reset();
  }
};

struct ArenaScope {         // what is allocated while it lives goes back to the arena on every path out
  Arena& a;
  const Arena::Mark mk;
  explicit ArenaScope(Arena& arena) : a(arena), mk(arena.mark()) {}
  ~ArenaScope() { a.release(mk); }
  ArenaScope(const ArenaScope&) = delete;
  ArenaScope& operator=(const ArenaScope&) = delete;
};

struct RnnPrep {            // one ResRNN (bsrnn.py:26-46) or TF-GridNet BLSTM, everything the forward needs, device pointers
  const float *norm_w, *norm_b, *whf, *whr, *proj_b;
  float *bcat, *wih_pack, *proj_pack, *fpack, *pack16, *pack32;
};

// ---- speaker encoder, its front-end and pooling layer (speaker.cc) ----
struct ConvPrep {           // conv (bias-free) + BatchNorm(eval) (+ ReLU) of the speaker encoder
  int cin, cout, k, stride, ldp;
  int sw = 0;               // stride along W when it differs from `stride` (CAM++'s FCM head strides the mel axis only); 0: same
  bool relu;
  const float *gamma, *beta;
  float *w2, *st;           // [cout][ldp] in im2col column order; [2][cout] = (running mean, rstd)
};

struct BlockPrep {          // BasicBlock: c1 (3x3, stride) c2 (3x3); Bottleneck: c1 (1x1) c2 (3x3, stride) c3 (1x1, x4)
  ConvPrep c1, c2, c3, sc;
  bool has_sc;
};

struct TdnnPrep {           // Conv1d (bias) -> ReLU -> BatchNorm1d(eval): wespeaker ECAPA-TDNN's Conv1dReluBn
  int cin, cout, k, dil;
  const float *w, *bias, *gamma, *beta;   // w: k == 1 the checkpoint's [cout][cin]; else the one-row-image view weight
  float* st;                              // [2][cout] = (running mean, rstd)
};

struct SeRes2Prep {         // SE_Res2Block: 1x1 TDNN, Res2Net branches, 1x1 TDNN, squeeze-excitation, + input
  TdnnPrep in, out;
  std::vector<TdnnPrep> branch;
  std::string se;           // "...se_res2block.3." (linear1 / linear2)
};

struct CamBn {              // BatchNorm1d(eval) of a pre-activation D-TDNN layer: (mean, rstd) + affine operands (or ones / zeros)
  int c;
  float* st;
  const float *gamma, *beta;
};
struct CamLayer {           // CAMDenseTDNNLayer: BN-ReLU, 1x1 to 128, BN-ReLU, dilated k = 3 conv to 32, context-aware mask
  int cin, dil;
  CamBn bn1, bn2;
  const float *w1, *wloc;   // linear1 [128][cin]; linear_local as the 3 x 3 view of the one-row image [32][9 * 128]
  const float *l1w, *l1b, *l2w, *l2b;
};
struct CamTransit {         // BN-ReLU + 1x1 (bias-free) to half the channels
  int cin, cout;
  CamBn bn;
  const float* w;
};

struct SpeakerEncoder {
  // meta: kind 0 wespeaker ResNet, 1 ECAPA-TDNN (wesep_amd/models/ecapa_tdnn.py), 2 CAM++ (wesep_amd/models/campplus.py)
  int kind = 0, channels = 512, glob = 0, emb_bn = 0, feat_dim = 80;
  int blocks[4] = {0, 0, 0, 0};
  int bottleneck = 0, two_emb = 0;    // wespeaker ResNet50 / 101 / 152 blocks; seg_1 -> ReLU -> BN -> seg_2
  // pooling (meta spk_pool: 0 TSTP, 1 MHASTP, 2 MQMHASTP, 3 ASTP, 4 TAP, 5 TSDP; absent: ASTP for ECAPA-TDNN, TSTP
  // otherwise).  MHASTP / MQMHASTP: queries x heads of attentive statistics, the weights of every (query, head) in one
  // pack (include/wesep_hip.h, ws_mhastp_fwd; the 1-D encoders launch ws_mhastp_fwd_split)
  int pool = 0, pool_q = 1, pool_h = 1, pool_layers = 2, pool_ds = 1;
  float* pool_pack = nullptr;
  // ResNet
  ConvPrep stem;
  std::vector<BlockPrep> res_blocks;
  float* seg_bn_st = nullptr;
  // ECAPA-TDNN
  TdnnPrep tdnn1;
  std::vector<SeRes2Prep> se_blocks;
  float *pool_bn_st = nullptr, *emb_bn_st = nullptr;
  // CAM++
  std::vector<ConvPrep> cam_fcm;      // conv1, then per BasicResBlock (conv1, [shortcut], conv2), then conv2
  std::vector<int> cam_fcm_kind;      // 0 plain, 1 block conv1, 2 shortcut, 3 block conv2 (+ residual)
  const float* cam_tdnn_w = nullptr;  // xvector.tdnn as the 5 x 5 view weight
  CamBn cam_tdnn_bn, cam_out_bn, cam_dense_bn;
  std::vector<std::vector<CamLayer>> cam_blocks;
  std::vector<CamTransit> cam_transit;
  int cam_init = 128, cam_growth = 32, cam_bn = 128;
  float *cam_one = nullptr, *cam_zero = nullptr, *cam_id_st = nullptr;   // ones / zeros / (0 x C | 1 x C), C = 1024
  // front-end: kaldi fbank (meta spk_feat = 1), or the in-model PreEmphasis + MelSpectrogram of spk_feat = False models
  // (bsrnn.py:231-242,343-350)
  int feat = 1;
  float *fb_basis = nullptr, *fb_bank = nullptr, *fb_floor = nullptr;
  int fb_win = 400, fb_shift = 160, fb_padded = 512;
  float *mel_basis = nullptr, *mel_fbt = nullptr, mel_coef = 0.97f;
  int mel_lds = 516, mel_ldp = 260;
};

// ---- pBSRNN (arch 0; bsrnn_plan.cc) ----
struct Bsrnn {
  int num_repeat = 6, fuse = 2, multi_fuse = 0;
  // band tables (bsrnn.py:190-209)
  std::vector<int> bw, f0;
  int K = 0;
  int *d_band_of_bin = nullptr, *d_f0 = nullptr, *d_bw = nullptr, *d_bw2 = nullptr, *d_off2 = nullptr;
  std::vector<RnnPrep> rnn;       // 2 per BSNet: band_rnn (time view), band_comm (band view)
  std::vector<int> sep_kind;      // per entry of separator.separation: 0 fuse layer, 1 BSNet
  // grouped-GEMM descriptor tables, rebuilt when (R, Tf) changes
  int desc_R = -1, desc_Tf = -1;
  ws_group_nt *d_bn = nullptr, *d_l1 = nullptr, *d_l2 = nullptr, *d_l3 = nullptr;
};

// ---- Conv-TasNet / SpEx+ (arch 1; wesep/models/convtasnet.py; tasnet_plan.cc): geometry and prepared operands ----
struct TasNet {
  int N = 512, L = 16, B = 128, H = 512, P = 3, X = 8, R = 3;
  int causal = 0, norm = 0;  // meta "causal" / "norm" (0 gLN, 1 cLN): (0, 0) the shipped model, (1, 1) the streamable one
  float* dec_wt = nullptr;   // decoder_1d_1 weight transposed to [L][N]
  float* bn_st[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};  // eval BN (mean, rstd) [2][C]
};

// ---- DPCCN (arch 2; wesep/models/dpccn.py; dpccn_plan.cc): prepared operands, in the order the forward consumes them ----
struct Dpccn {
  int fuse = 2, causal = 0, tcn_blocks = 10, tcn_layers = 2;
  float *ana4 = nullptr, *syn4 = nullptr;       // analysis basis [4 * 257][512] (re, im, 0, 0 per bin), synthesis [512][4 * 257]
  float* w_in = nullptr;                        // conv2d (2 -> 16) as [16][9 * 4] on the (re, im, 0, 0) pixels
  float *w_out = nullptr, *b_out = nullptr;     // deconv2d (32 -> 2) as [4][9 * 32] + bias[4]: (re, im, 0, 0) per bin
  float *ones = nullptr, *zeros = nullptr;      // gamma 1, beta 0 of the plain depthwise conv
  std::map<std::string, float*> w;              // per-layer GEMM weights / conv3x3 packs, keyed by the layer's state_dict prefix
};

// ---- TF-GridNet (arch 3; gridnet_plan.cc) ----
struct GridBlock {
  RnnPrep intra, inter;
  float *wqkv, *bqkv;                    // [nh*(2E + cp)][C] rows (Q heads | K heads | V heads), bias
  float *gam[3], *bet[3];                // per projection: [nh][Q*ch], index q*ch + e
  float *proj_g, *proj_b;                // [Q*C], index q*C + c
};
struct GridNet {
  int n_fft = 128, hop = 64, Q = 65, C = 128, hid = 192, nh = 4, E = 8, layers = 6, fuse = 2;
  float *ana4 = nullptr, *syn4 = nullptr, *w_in = nullptr, *w_out = nullptr, *b_out = nullptr;
  float *ones_c = nullptr, *zeros_c = nullptr, *ones_qc = nullptr, *zeros_qc = nullptr;
  float *id_st = nullptr, *slope1 = nullptr, *film_bias1 = nullptr;
  std::vector<GridBlock> blocks;
};

}  // namespace wsrt

struct ws_engine {
  bool dry = false;
  int device = 0, cu_count = 0;
  hipStream_t stream = nullptr;
  std::map<std::string, int64_t> meta;
  std::map<std::string, wsrt::Tensor> tensors;
  std::vector<float> hw;          // host copy of the weight blob
  float* dw = nullptr;            // device copy
  wsrt::Arena persist, work;
  long long n_launches = 0;
  long long long_windows = 0, long_forwards = 0;   // of the last ws_engine_separate_long
  long long live_state_bytes = 0;                  // device state of the live handle opened last (ws_engine_live_open)
  long long live_windows = 0, live_groups = 0;     // windows run since that handle's open / reset; groups of its last call
  long long live_pool_state_bytes = 0;             // device state of the live pool opened last (ws_engine_live_pool_open)
  long long live_pool_rounds = 0, live_pool_forwards = 0;   // rounds and forwards of the last live-pool push or flush
  long long tail_pool_state_bytes = 0;             // device state of the tail pool opened last (ws_engine_tail_pool_open)
  long long tail_pool_forwards = 0, tail_pool_rows = 0;     // forwards and separator rows of the last tail-pool tick or flush
  long long rate_tail_pool_state_bytes = 0;        // device state of the rate tail pool opened last (ws_engine_rate_tail_pool_open)
  long long rate_tail_pool_forwards = 0, rate_tail_pool_rows = 0;     // forwards and separator rows of its last tick or flush
  long long stream_state_bytes = 0;                // device state of the stream opened last (ws_engine_stream_open)
  long long cluster_fallbacks = 0;   // forwards in which a cluster recurrence timed out and the streaming kernels took over
  unsigned* cl_status = nullptr;     // sticky device word set by ws_lstm_fwd_cluster on a timeout
  std::map<std::pair<int, int>, const float*> rs_taps;   // (rate_in, rate_out) -> device tap table (rate.cc), made on first use
  // configuration shared by the plans
  int arch = 0;                   // 0 pBSRNN, 1 Conv-TasNet, 2 DPCCN, 3 TF-GridNet
  int sr = 16000, E = 256, use_xform = 0, joint = 0;
  float *id_st = nullptr, *id_one = nullptr, *id_zero = nullptr;   // identity BatchNorm operands: y = x + res
  // ragged speaker pass (speaker.cc): device int[R] tables of this forward, one per distinct set of per-row widths
  std::vector<std::pair<std::vector<int>, const int*>> spk_tabs;
  float *slope0 = nullptr, *slope1 = nullptr;     // PReLU slopes 0 (ReLU) and 1 (identity)
  // the parts
  wsrt::SpeakerEncoder spk;
  wsrt::Bsrnn bs;
  wsrt::TasNet tas;
  wsrt::Dpccn dp;
  wsrt::GridNet grid;

  const wsrt::Tensor* find(const std::string& name) const {
    auto it = tensors.find(name);
    return it == tensors.end() ? nullptr : &it->second;
  }
  const float* dev(const std::string& name) const {
    const wsrt::Tensor* t = find(name);
    return t ? dw + t->off : nullptr;
  }
  const float* host(const std::string& name) const {
    const wsrt::Tensor* t = find(name);
    return t ? hw.data() + t->off : nullptr;
  }
};

namespace wsrt {

// A launch "passes" when it succeeded, or -- in a dry run -- when it failed for any reason other than its
// argument validation (there is no device to launch on).
bool passes(ws_engine* e, int rc, const char* what);

#define WS_RUN(e, call)                              \
  do {                                               \
    const int rc__ = (call);                         \
    if (!passes((e), rc__, #call)) return rc__ ? rc__ : WS_ERR_LAUNCH; \
  } while (0)

#define WS_PTR(p)                  \
  do {                             \
    if (!(p)) return WS_ERR_LAUNCH; \
  } while (0)

// ---- shared helpers (engine.cc) ----
int to_device(ws_engine* e, void* dst, const void* src, size_t bytes);
int to_host(ws_engine* e, void* dst, const void* src, size_t bytes);
int zero_device(ws_engine* e, void* p, size_t bytes);
float* upload(ws_engine* e, Arena& a, const float* src, size_t n);
int* upload_ints(ws_engine* e, Arena& a, const std::vector<int>& v);
int64_t meta_or(const ws_engine* e, const char* key, int64_t dflt);
bool require(ws_engine* e, const std::string& name, std::initializer_list<int64_t> dims);
float* bn_eval_stats(ws_engine* e, const std::string& bn, int c);
int vec_bits(std::initializer_list<long long> dims, int base = 3);
int linear(ws_engine* e, const float* x, int M, int k, const float* W, long long ldw, int nout, const float* bias,
           int act, float* y);
int copy_cols(ws_engine* e, float* dst, long long ldd, const float* src, long long lds, int width, long long rows);
int time_mean(ws_engine* e, const float* x, int R, int T, int C, float* mean2);

// ---- the pieces of a forward that the entry points share (engine.cc) ----
int check_engine(const ws_engine* e, const char* who);
// the separator's demands on a rectangle of R rows of T samples (the architecture's own message); ptrs: no NULL argument
int check_rows(ws_engine* e, bool ptrs, int R, int T);
// enrollment kind and lengths against the container; Te / te_row: the frames of the rectangle / of every row
int check_enroll(ws_engine* e, int R, int enroll_kind, int enroll_len, const int* enroll_lengths, int* Te, std::vector<int>* te_row);
struct ForwardTurn {     // hipSetDevice + the opt-in one-forward-at-a-time lock (WS_ENGINE_SERIALIZE), held while it lives
  std::unique_lock<std::mutex> turn;
  int rc = WS_OK;
  int nested = -1;       // the device whose per-thread depth this turn counts in: a turn taken while the calling thread holds
                         // one for the same device (ws_engine_separate_rate around ws_engine_separate) does not lock again
  explicit ForwardTurn(ws_engine* e);
  ~ForwardTurn();
  ForwardTurn(const ForwardTurn&) = delete;
  ForwardTurn& operator=(const ForwardTurn&) = delete;
};
int speaker_stage(ws_engine* e, const void* enroll, int enroll_kind, int R, int enroll_len, int Te, const int* enroll_lengths,
                  const int* te_row, float* d_emb);
int note_cluster_status(ws_engine* e);
// TF-GridNet's (unbiased) standard deviation of x[0..n) and, if wanted, x / std
void row_std_scale(const float* x, int n, float* std_out, float* scaled);
int separate_impl(ws_engine* e, const float* mix, int R, int T, const int* lengths, const void* enroll, int enroll_kind,
                  int enroll_len, const int* enroll_lengths, float* est);
int separate_long(ws_engine* e, const float* mix, int n, int K, const void* enroll, int enroll_kind, int enroll_len,
                  const int* enroll_lengths, int window, int overlap, int max_rows, float* est);
int long_check_window(ws_engine* e, int window, int overlap, int max_rows);
int long_check_group(ws_engine* e, int G, int L, int K, int enroll_kind, int enroll_len, const int* enroll_lengths, int* Te,
                     std::vector<int>* te_row);

// ---- speaker stage (speaker.cc) ----
int read_speaker_meta(ws_engine* e);
int prep_spk_transform(ws_engine* e);
int prep_speaker(ws_engine* e);
// enroll_lengths / te_row (host, [R]; both or neither): the rows' own samples or frames and their frame counts -- one
// encoder pass over the rectangle with masked epilogues and length-aware reductions (ragged_speaker_covered encoders only)
int speaker_embed(ws_engine* e, const void* enroll, int enroll_kind, int R, int enroll_len, int Te, float* emb,
                  const int* enroll_lengths = nullptr, const int* te_row = nullptr);
bool ragged_speaker_covered(const ws_engine* e);
int spk_transform(ws_engine* e, const float* emb, int R, const float** out);

// ---- launch plans ----
int prepare_bsrnn(ws_engine* e);
int pack_rnn(ws_engine* e, int C, const float* wih_f, const float* wih_r, const float* const bias[4], const float* proj_w,
             RnnPrep* r);
int separate_device(ws_engine* e, const float* wav, int R, int T, const float* emb_in, float* est,
                    const int* d_len = nullptr, const int* d_tf = nullptr);
int prepare_tasnet(ws_engine* e);
int tasnet_separate(ws_engine* e, const float* mix, int R, int T, const void* enroll, int enroll_kind, int enroll_len,
                    float* est);
int tasnet_check_rows(ws_engine* e, bool ptrs, int R, int T);
int tasnet_check_enroll(ws_engine* e, int enroll_kind, int enroll_len);
int tasnet_speaker(ws_engine* e, const float* enroll_wave, int R, int Te, float* emb);
int tasnet_device(ws_engine* e, const float* wav, int R, int T, const float* emb_in, const float* enroll_wave, int Te,
                  float* est);
int tas_row_stats(ws_engine* e, const float* x, long long M, int C, float* st);
struct TasGemm {
  const float* A = nullptr;
  long long lda = 0;
  long long M = 0;
  int K = 0;
  const float* W = nullptr;
  int ldw = 0, N = 0;
  const float* bias = nullptr;
  int act = 0;
  float* C = nullptr;
  long long ldc = 0;
  const float* R = nullptr;                                       // residual, addressed like C
  const float *stats = nullptr, *gamma = nullptr, *beta = nullptr; // norm-on-load
  int st_div1 = 1;                                                 // rows per statistics pair (gLN: T', cLN: 1)
  bool f32 = false;                                                // exact-fp32 products (the SpEx+ speaker encoder)
  int a_div = kBig;                                                // frames view: row m -> (m / a_div) * a_s1 + (m % a_div) * lda
  long long a_s1 = 0;
};
int tas_gemm(ws_engine* e, const TasGemm& t);
inline bool tas_streamable(const ws_engine* e) { return e->arch == 1 && e->tas.causal && e->tas.norm == 1; }
// ---- what the streaming front ends (stream.cc, stream_pool.cc, rate.cc, rate_pool.cc) share ----
struct StreamBlock {         // one causal cLN block: its weights, and where its carried state lives
  const float *w1, *b1, *a1, *g1, *be1, *wd, *bd, *a2, *g2, *be2, *w3, *b3;
  int ldw, dil, cap;
  float* ring;               // [rows][cap][H]
  const float* rb;           // [rows][H] = W_e e + b for the stack's first block, else NULL
};
struct StreamWeights {       // every weight pointer of a group of frames, resolved once
  const float *enc_w[3], *enc_b[3], *ln_g, *ln_b, *proj_w, *proj_b, *mask_w, *mask_b, *dec_b;
  std::vector<StreamBlock> blocks;
};
int refuse_not_streamable(const ws_engine* e, const char* who);      // WS_ERR_INVALID with the reason, by name
int tas_flat_stats(ws_engine* e, const float* x, int R, long long n, float* st);
// The state block of a solo stream or a pool: ONE allocation made at open.  rows: the rows of a stream, the slots of a pool.
struct StreamCore : StreamWeights {
  ws_engine* e = nullptr;
  int rows = 0, G = 0;
  char* state = nullptr;
  size_t state_bytes = 0;
  std::vector<float*> rb;               // per stack [rows][H]
  float *carry = nullptr, *carry0 = nullptr, *emb = nullptr;     // [rows][L - s], the carry's reset image, [rows][E]
  bool block_kernel = false;            // WS_STREAM_BLOCK_KERNEL: one call per block
};
// rows x max_chunk_frames against 2^31 elements in one buffer; noun: "rows" or "slots"
int stream_core_check(const ws_engine* e, const char* who, const char* noun, int rows, int G);
// Lays out and allocates the state -- the rings per block, `parts` (floats each, the owner's), the row biases per stack,
// `extra_floats` if any; 256-byte aligned, in that order -- fills it with NaN under WS_ENGINE_POISON, resolves the weights and
// wires cap / ring / rb into the blocks.  at: the addresses of `parts`, then of the extra part.
int stream_core_open(StreamCore* c, const char* who, ws_engine* e, int rows, int G, unsigned flags, const std::vector<size_t>& parts,
                     size_t extra_floats, std::vector<float*>* at);
void stream_core_free(StreamCore* c);
// The speaker stage for rows [row0, row0 + n): embedding, SpeakerTransform, copy into emb, the stacks' row biases W_e e + b
int stream_enroll(StreamCore* c, const char* who, const void* enroll, int enroll_kind, int enroll_len, int row0, int n);
struct ChainRows {           // how the two time-crossing kernels address their rows
  int rows = 0, Tc = 0;
  long long t0 = 0;          // solo form: every row at frame t0, state row = rectangle row
  int nslots = 0;            // rows form (d_slot != nullptr): per-row (slot, t0, tc) device tables
  const int *d_slot = nullptr, *d_tc = nullptr;
  const long long* d_t0 = nullptr;
};
// The launch chain of one group of frames over the rectangle x0 [rows][pitch]: 3 framing GEMMs, row statistics, projection; per
// block GEMM, the fused middle, GEMM (or the block kernel); mask GEMM, mask product, synthesis GEMM, overlap-add.  Its
// activations and *est [rows][Tc s] come from the work arena: the caller holds an ArenaScope.
int stream_chain(ws_engine* e, const StreamWeights& w, bool block_kernel, const float* x0, long long pitch, const ChainRows& r,
                 float* carry, float** est);

// ---- the emission rule ----
constexpr int kEncLmax = 160;    // the longest window of the MultiEncoder (encoder.py:66-114)
struct Geom {                    // one direction of the resampler (ws_resample_geom)
  int U = 1, D = 1, w = 0, K = 1;
};
inline long long rs_len(const Geom& g, long long n) { return ((long long)g.U * n + g.D - 1) / g.D; }                   // whole signal
inline long long rs_emitted(const Geom& g, long long n) { return n > g.w ? (long long)g.U * ((n - g.w) / g.D) : 0; }    // streamed so far
// frames of a stream that n samples complete: while it runs (the longest window must fit), and at its flush (zero-extended)
inline long long plain_frames(long long n, int L, bool flush = false) {
  return flush ? (n - L) / (L / 2) + 1 : (n >= kEncLmax ? (n - kEncLmax) / (L / 2) + 1 : 0);
}
inline long long plain_emitted(long long n, int L) { return plain_frames(n, L) * (L / 2); }
inline long long plain_total(long long n, int L) { return ((n - L) / (L / 2)) * (L / 2) + L; }
struct Step {
  int lead = 0, n_valid = 0, n_out = 0, hist_from = 0, hist_len = 0;
  long long g_new = 0;
};
// the arguments of one streaming resampler step from the counters: n_new samples behind a history of h; a final step keeps none
inline Step plan_step(const Geom& g, long long n_in, long long groups, int h, int n_new, bool final) {
  Step s;
  const long long N = n_in + n_new;
  const long long a0 = std::max<long long>(0, groups * g.D - g.w);
  s.lead = static_cast<int>(std::max<long long>(0, g.w - groups * g.D));
  s.n_valid = h + n_new;
  s.g_new = groups;
  if (final) {
    s.n_out = static_cast<int>(rs_len(g, N) - groups * g.U);
  } else {
    s.g_new = N > g.w ? (N - g.w) / g.D : 0;
    s.n_out = static_cast<int>((s.g_new - groups) * g.U);
    s.hist_from = static_cast<int>(std::max<long long>(0, s.g_new * g.D - g.w) - a0);
    s.hist_len = s.n_valid - s.hist_from;
  }
  return s;
}
// what a push of n >= 1 samples at the caller's rate returns at most (n = 0: the flush), through a (in) and b (back)
inline int rate_push_cap(const Geom& a, const Geom& b, int L, int n) {
  const int hop = L / 2;
  if (n == 0) {      // the flush: what A still owes (its history is below K), the inner stream's rest, what B still owes
    const long long ma = ((long long)a.K / a.D + 1) * a.U;
    const long long mm = (ma / hop + 1) * hop + WS_STREAM_FLUSH_CAP;
    return static_cast<int>(std::min<long long>(0x7fffffff, ((mm + b.K) / b.D + 2) * b.U));
  }
  // A returns whole groups: at most n / D + 1 of them; the inner stream whole frames; B whole groups again
  const long long ma = ((long long)n / a.D + 1) * a.U;
  const long long mm = (ma / hop + 1) * hop;
  return static_cast<int>(std::min<long long>(0x7fffffff, (mm / b.D + 1) * b.U));
}

// ---- the emission rule of the live front ends (live.cc, live_pool.cc; include/wesep_engine.h "live windows") ----
// windows run after N samples: window w starts at w H and runs once w H + S samples exist
inline long long live_windows_run(long long N, int S, int H) { return N < S ? 0 : 1 + (N - S) / H; }
// samples emitted once Wr windows have run: those before the start of the newest window
inline long long live_emitted(long long Wr, int H) { return std::max<long long>(Wr - 1, 0) * H; }
// the next group of a recording that has run Wr of Wr_new windows: at most g_max windows, cut where the ring of cap slots wraps
inline int live_cut(long long Wr, long long Wr_new, int g_max, int cap) {
  return static_cast<int>(std::min<long long>({Wr_new - Wr, (long long)g_max, cap - Wr % cap}));
}

// ---- copies and the synchronisation of a streaming call, on the engine's stream; who / what: the message of a failure.
// Dry run: nothing was computed, so a caller's buffer (device to host) stays untouched; every other copy is a memcpy (dry
// "device" memory is malloc'd).  height == 1 with both pitches 0: a 1-D copy
inline int copy_async(ws_engine* e, const char* who, const char* what, void* dst, size_t dpitch, const void* src, size_t spitch,
                      size_t width, size_t height, hipMemcpyKind kind) {
  if (width == 0 || height == 0) return WS_OK;
  const bool flat = height == 1 && dpitch == 0 && spitch == 0;
  if (e->dry) {
    for (size_t r = 0; kind != hipMemcpyDeviceToHost && r < height; ++r)
      memcpy(static_cast<char*>(dst) + r * dpitch, static_cast<const char*>(src) + r * spitch, width);
    return WS_OK;
  }
  if ((flat ? hipMemcpyAsync(dst, src, width, kind, e->stream)
            : hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, e->stream)) != hipSuccess) {
    set_err("%s: %s failed", who, what);
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}
inline int copy_async(ws_engine* e, const char* who, const char* what, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  return copy_async(e, who, what, dst, 0, src, 0, bytes, 1, kind);
}
inline int sync_stream(ws_engine* e, const char* who) {
  if (!e->dry && hipStreamSynchronize(e->stream) != hipSuccess) {
    set_err("%s: the device reported an error", who);
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

// ---- what a rate stream (rate.cc) needs of the solo stream (stream.cc) ----
// extra_floats > 0: one more slot in the stream's state allocation (*extra), and chunks / estimates are DEVICE buffers
int stream_open_impl(ws_engine* e, int rows, const void* enroll, int enroll_kind, int enroll_len, int max_chunk_frames,
                     unsigned flags, size_t extra_floats, ws_stream** out, float** extra);
// pitches in floats; est_pitch < 0: the emitted count (the plain stream).  A device-buffer stream takes no turn, does not reset
// the launch counter and does not synchronise: its caller does, once
int stream_push_impl(ws_stream* st, const float* chunk, long long chunk_pitch, int n, float* est, long long est_pitch, int est_cap,
                     int* n_out);
int stream_flush_impl(ws_stream* st, float* est, long long est_pitch, int est_cap, int* n_out);
// ---- the stream pool's state (stream_pool.cc), and what a rate pool (rate_pool.cc) needs of it ----
struct PoolSlot {
  enum State { kFree, kAttached, kDone } state = kFree;
  bool failed = false;         // a push or flush that named this slot ended half way
  long long n = 0, k = 0;      // samples pushed, frames run
  std::vector<float> pend;     // the samples from frame k's first one on (a rate pool keeps them on the device)
};
struct PoolGroup {             // host memory of one group, alive until the call's synchronisation
  std::vector<float> stage, est;
  std::vector<int> slot, tc, col;      // col: where the row's samples go in its caller's buffer
  std::vector<long long> t0;
  int Tc = 0;
  // a group on DEVICE buffers (a rate pool): row i's pending samples are src_have[i] floats at state float src_off[i], its
  // estimates go to state float dst_off[i]; the two ws_rows_copy_fwd tables stay alive here
  std::vector<long long> src_off, dst_off;
  std::vector<int> src_have;
  std::vector<ws_rows_copy_row> gather, scatter;
};
}  // namespace wsrt

struct ws_pool : wsrt::StreamCore {     // rows: the slots; carry0 is one row [L - s]
  std::vector<wsrt::PoolSlot> slots;
  std::vector<wsrt::PoolGroup> groups;  // of the call in hand
  bool device_io = false;               // a rate pool's: groups gather from and scatter to the state allocation
};

namespace wsrt {
// who: the entry point's name in messages; extra_floats > 0: one more part of the ONE state allocation (*extra), and groups
// run on device buffers (PoolGroup src_off / dst_off).  The caller holds no turn; attach takes the lowest free slot.
int pool_open_impl(ws_engine* e, const char* who, int slots, int max_chunk_frames, unsigned flags, size_t extra_floats, ws_pool** out,
                   float** extra);
int pool_attach_impl(ws_pool* p, const char* who, const void* enroll, int enroll_kind, int enroll_len, int* slot);
int pool_run_group(ws_pool* p, PoolGroup& g);
int pool_check(const ws_pool* p, const char* who);
void pool_free(ws_pool* p);
// the slot checks of a push, a flush and a detach, for both pools: the argument arrays; entry i (slot id, n samples at chunk:
// attached, not flushed, named once -- seen [slots] -- a packet); the slot of a flush or a detach
int pool_check_push_args(const char* who, int n_active, const void* slots, const void* chunks, const void* n, const void* est,
                         const void* est_cap, const void* n_out);
int pool_check_entry(const ws_pool* p, const char* who, std::vector<char>& seen, int i, int id, int n, const float* chunk);
int pool_check_slot(const ws_pool* p, const char* who, int slot, bool flush);
int pool_detach_impl(ws_pool* p, const char* who, int slot);   // p NULL: refused as a null pool
// ---- what a rate pool needs of rate.cc: x [R][n] (host) at rate_in -> y [R][*n_out] (host) at rate_out, the kernel's limits and
// the sizes refused by name as `who`; the caller holds the turn
int resample_host_rows(ws_engine* e, const char* who, const float* x, int R, int n, int rate_in, int rate_out, std::vector<float>* y,
                       int* n_out);
int prepare_dpccn(ws_engine* e);
int dpccn_device(ws_engine* e, const float* wav, int R, int T, const float* emb_in, float* est);
int dp_conv_view(ws_engine* e, const float* x, int R, int H, int W, int Cin, int mode, int Wo, int sw, const float* Wm, int Cout,
                 const float* bias, float* y, long long ldy);
int dp_gemm(ws_engine* e, const float* A, long long M, int K, const float* Wm, int N, const float* bias, const float* Rm, float* C,
            long long ldc);
int dp_io_convs(ws_engine* e, const std::string& conv, int cin, const std::string& deconv, int cout, float** w_in, float** w_out,
                float** b_out);
int dft_bases(ws_engine* e, int n, float** ana4, float** syn4);
int dft_istft(ws_engine* e, const float* est4, const float* syn4, int R, int Tf, int n, int hop, int T, float* est);
int prepare_gridnet(ws_engine* e);
// h_tf (host), d_len / d_tf (device), [R], all or none: the rows' own frame counts 1 + lengths[r] / hop, samples and frame
// counts -- one forward over the rectangle, the length where the model reduces over time (gridnet_plan.cc)
int gridnet_device(ws_engine* e, const float* wav, int R, int T, const float* emb_in, float* est, const int* h_tf = nullptr,
                   const int* d_len = nullptr, const int* d_tf = nullptr);

}  // namespace wsrt

#endif  // WESEP_ENGINE_INTERNAL_H_
