// libwesep_engine.so -- native inference runtime of wesep_amd (include/wesep_engine.h).
//
// MI355X counterpart of the reference's C++ runtime (runtime/separate/separate_engine.{h,cc}: a TorchScript module on
// LibTorch-CPU plus a host kaldi fbank).  Each model's forward is a fixed launch plan over the device library's C ABI
// (include/wesep_hip.h), one file per plan (engine_internal.h lists them):
//   * load: the weight container is read, uploaded once, and everything that the Python training path re-derives
//     per step is derived once -- [W_ih_f | W_ih_r] concatenation, MFMA-fragment packs of W_ih / W_hh / proj for the
//     blocked-layout GEMMs and recurrences, BatchNorm folded to (running mean, rstd), conv kernels permuted to the
//     im2col column order, the folded kaldi fbank basis (see wesep_amd/utils/funcs.py);
//   * forward: activations come from one grow-only device arena with stack discipline (per-layer scratch is released
//     when the layer ends, so the peak is one ResRNN's working set, not the sum); the per-band grouped GEMMs get their
//     descriptor tables rebuilt only when the frame count changes.
// This file: the weight container, the helpers every plan uses, the load dispatch by meta "arch" and the C ABI.
#include <stdarg.h>

#include <mutex>

#include "engine_internal.h"

namespace wsrt {

namespace {
thread_local char g_err[768] = "";
}  // namespace

void set_err(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

bool passes(ws_engine* e, int rc, const char* what) {
  ++e->n_launches;
  if (rc == WS_OK) return true;
  if (e->dry && rc != WS_ERR_INVALID) return true;
  set_err("engine: %s failed (rc=%d): %s", what, rc, ws_last_error());
  return false;
}

int to_device(ws_engine* e, void* dst, const void* src, size_t bytes) {
  if (e->dry) {
    memcpy(dst, src, bytes);
    return WS_OK;
  }
  if (hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
      hipStreamSynchronize(e->stream) != hipSuccess) {
    set_err("engine: host-to-device copy of %zu bytes failed", bytes);
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

int to_host(ws_engine* e, void* dst, const void* src, size_t bytes) {
  if (e->dry) return WS_OK;    // nothing was computed: leave the caller's buffer untouched
  if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
      hipStreamSynchronize(e->stream) != hipSuccess) {
    set_err("engine: device-to-host copy of %zu bytes failed", bytes);
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

int zero_device(ws_engine* e, void* p, size_t bytes) {
  if (e->dry) {
    memset(p, 0, bytes);
    return WS_OK;
  }
  if (hipMemsetAsync(p, 0, bytes, e->stream) != hipSuccess) {
    set_err("engine: memset failed");
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

float* upload(ws_engine* e, Arena& a, const float* src, size_t n) {
  float* d = a.alloc(n);
  if (!d) return nullptr;
  if (to_device(e, d, src, n * 4) != WS_OK) return nullptr;
  return d;
}

int* upload_ints(ws_engine* e, Arena& a, const std::vector<int>& v) {
  return reinterpret_cast<int*>(upload(e, a, reinterpret_cast<const float*>(v.data()), v.size()));
}

// ---- weight container (written by wesep_amd/bin/export_engine.py) ---------------------------------------------
//   char magic[8] = "WSEPW001"
//   u32 n_meta;    n_meta    x { char key[32]; i64 value }
//   u32 n_tensors; n_tensors x { u32 name_len; char name[name_len]; u32 ndim; i64 dims[ndim]; u64 offset_floats }
//   u64 n_floats;  float data[n_floats]
bool read_exact(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int load_container(ws_engine* e, const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    set_err("engine: cannot open %s", path);
    return WS_ERR_INVALID;
  }
  char magic[8];
  uint32_t n_meta = 0, n_tensors = 0;
  bool ok = read_exact(f, magic, 8) && memcmp(magic, "WSEPW001", 8) == 0 && read_exact(f, &n_meta, 4) &&
            n_meta < 4096;
  for (uint32_t i = 0; ok && i < n_meta; ++i) {
    char key[33] = {0};
    int64_t v = 0;
    ok = read_exact(f, key, 32) && read_exact(f, &v, 8);
    if (ok) e->meta[key] = v;
  }
  ok = ok && read_exact(f, &n_tensors, 4) && n_tensors < (1u << 20);
  for (uint32_t i = 0; ok && i < n_tensors; ++i) {
    uint32_t name_len = 0, ndim = 0;
    ok = read_exact(f, &name_len, 4) && name_len < 1024;
    std::string name(name_len, '\0');
    ok = ok && read_exact(f, &name[0], name_len) && read_exact(f, &ndim, 4) && ndim <= 8;
    Tensor t;
    t.n = 1;
    for (uint32_t d = 0; ok && d < ndim; ++d) {
      int64_t v = 0;
      ok = read_exact(f, &v, 8) && v >= 0;
      t.dims.push_back(v);
      // overflow-checked product: a crafted container must not wrap n (and pass the bounds check below)
      if (ok && v != 0 && t.n > (uint64_t(1) << 40) / static_cast<uint64_t>(v)) ok = false;
      t.n *= static_cast<size_t>(v);
    }
    uint64_t off = 0;
    ok = ok && read_exact(f, &off, 8);
    t.off = off;
    if (ok) e->tensors[name] = t;
  }
  uint64_t n_floats = 0;
  ok = ok && read_exact(f, &n_floats, 8) && n_floats < (uint64_t(1) << 34);
  if (ok) {
    e->hw.resize(n_floats);
    ok = read_exact(f, e->hw.data(), n_floats * 4);
  }
  fclose(f);
  if (!ok) {
    set_err("engine: %s is not a valid wesep_amd weight container", path);
    return WS_ERR_INVALID;
  }
  for (auto& kv : e->tensors) {
    if (kv.second.n > e->hw.size() || kv.second.off > e->hw.size() - kv.second.n) {   // no wrap-around
      set_err("engine: tensor %s exceeds the data section", kv.first.c_str());
      return WS_ERR_INVALID;
    }
  }
  return WS_OK;
}

int64_t meta_or(const ws_engine* e, const char* key, int64_t dflt) {
  auto it = e->meta.find(key);
  return it == e->meta.end() ? dflt : it->second;
}

bool require(ws_engine* e, const std::string& name, std::initializer_list<int64_t> dims) {
  const Tensor* t = e->find(name);
  if (!t) {
    set_err("engine: tensor %s is missing from the container", name.c_str());
    return false;
  }
  std::vector<int64_t> want(dims);
  size_t n = 1;
  for (auto d : want) n *= static_cast<size_t>(d);
  if (t->n != n) {
    set_err("engine: tensor %s has %zu elements, expected %zu", name.c_str(), t->n, n);
    return false;
  }
  return true;
}

float* bn_eval_stats(ws_engine* e, const std::string& bn, int c) {
  const float* rm = e->host(bn + ".running_mean");
  const float* rv = e->host(bn + ".running_var");
  std::vector<float> st(2 * size_t(c));
  for (int o = 0; o < c; ++o) {
    st[o] = rm[o];
    st[c + o] = 1.0f / sqrtf(rv[o] + kBnEps);
  }
  return upload(e, e->persist, st.data(), st.size());
}

// ---- forward pieces shared by the plans -------------------------------------------------------------------------
int vec_bits(std::initializer_list<long long> dims, int base) {
  for (long long d : dims)
    if (d % 4) return 4;                 // scalar loads, split-bf16 bit kept (falls back to the fp32 kernels)
  return base | 4;
}

// y[M][nout] = act(x[M][k] W[nout][k]^T + bias)      (functional._lin_fwd)
int linear(ws_engine* e, const float* x, int M, int k, const float* W, long long ldw, int nout, const float* bias,
           int act, float* y) {
  ws_gemm_nt_args a = {};
  a.A = x;
  a.W = W;
  a.bias = bias;
  a.C = y;
  a.a_div = kBig;
  a.a_s2 = k;
  a.c_div = kBig;
  a.c_s2 = nout;
  a.st_div1 = 1;
  a.st_div2 = 1;
  a.M = M;
  a.N = nout;
  a.K = k;
  a.ldw = static_cast<int>(ldw);
  a.act = act;
  a.vec = vec_bits({k, ldw});
  WS_RUN(e, ws_gemm_nt(&a, e->stream));
  return WS_OK;
}

// dst[m][0:width] = src[m][0:width] for `rows` rows with row strides ldd / lds (floats): channel slices of
// channels-last activations (torch.split / torch.cat of the Res2Net branches and the layer aggregation)
int copy_cols(ws_engine* e, float* dst, long long ldd, const float* src, long long lds, int width, long long rows) {
  ++e->n_launches;
  if (e->dry) return WS_OK;
  if (hipMemcpy2DAsync(dst, size_t(ldd) * 4, src, size_t(lds) * 4, size_t(width) * 4, size_t(rows), hipMemcpyDeviceToDevice,
                       e->stream) != hipSuccess) {
    set_err("engine: strided device copy failed");
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

// mean over the T frames of each utterance, [R*T][C] -> sums [R][2][C] scaled by 1/T (the first C of each row)
int time_mean(ws_engine* e, const float* x, int R, int T, int C, float* mean2) {
  void* s = e->stream;
  Arena& a = e->work;
  int nsplit = T / 32;
  const int cap = 1024 / R > 1 ? 1024 / R : 1;
  if (nsplit > cap) nsplit = cap;
  if (nsplit < 1) nsplit = 1;
  float* slab = a.alloc(size_t(nsplit) * R * 2 * C);
  float* sums = a.alloc(size_t(R) * 2 * C);
  WS_PTR(slab && sums);
  WS_RUN(e, ws_chan_sums(x, nullptr, nullptr, 1, T, R, nsplit, C, slab, s));
  WS_RUN(e, ws_reduce_slabs(slab, nsplit, (long long)R * 2 * C, (long long)R * 2 * C, sums, 0, 0, s));
  WS_RUN(e, ws_bcast_rows(sums, 1.0f / T, 1, R, 2 * C, mean2, s));
  return WS_OK;
}

int prepare(ws_engine* e) {
  e->arch = static_cast<int>(meta_or(e, "arch", 0));
  e->sr = static_cast<int>(meta_or(e, "sample_rate", 16000));
  int rc;
  switch (e->arch) {
    case 0: rc = prepare_bsrnn(e); break;
    case 1: rc = prepare_tasnet(e); break;
    case 2: rc = prepare_dpccn(e); break;
    case 3: rc = prepare_gridnet(e); break;
    default:
      set_err("engine: architecture %d has no launch plan (0 pBSRNN, 1 Conv-TasNet, 2 DPCCN, 3 TF-GridNet)", e->arch);
      return WS_ERR_INVALID;
  }
  if (rc != WS_OK) return rc;
  if (!e->dry && hipStreamSynchronize(e->stream) != hipSuccess) {
    set_err("engine: weight preparation failed on the device");
    return WS_ERR_LAUNCH;
  }
  return WS_OK;
}

int check_engine(const ws_engine* e, const char* who) {
  if (!e) {
    set_err("%s: null engine", who);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

}  // namespace wsrt

using namespace wsrt;

// ---- C ABI ----------------------------------------------------------------------------------------------------
WS_ENGINE_API int ws_engine_abi_version(void) { return WS_ENGINE_ABI_VERSION; }
WS_ENGINE_API const char* ws_engine_last_error(void) { return g_err; }

WS_ENGINE_API void ws_engine_destroy(ws_engine* e) {
  if (!e) return;
  e->work.free_all();
  e->persist.free_all();
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

WS_ENGINE_API int ws_engine_create(const char* weights_path, int device, int flags, ws_engine** out) {
  if (!weights_path || !out) {
    set_err("ws_engine_create: null argument");
    return WS_ERR_INVALID;
  }
  *out = nullptr;
  if (ws_abi_version() != WS_ABI_VERSION) {
    set_err("ws_engine_create: libwesep_hip.so ABI %d, engine built for %d", ws_abi_version(), WS_ABI_VERSION);
    return WS_ERR_INVALID;
  }
  ws_engine* e = new ws_engine();
  e->dry = (flags & WS_ENGINE_DRY_RUN) != 0;
  e->device = device;
  e->persist.dry = e->work.dry = e->dry;
  int rc = load_container(e, weights_path);
  if (rc == WS_OK && e->dry) {
    // with a device present the launches of a dry run would really execute -- on host pointers
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
      set_err("ws_engine_create: WS_ENGINE_DRY_RUN is for machines without a GPU (%d HIP device(s) visible)", ndev);
      rc = WS_ERR_INVALID;
    }
  }
  if (rc == WS_OK && !e->dry) {
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess ||
        hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
      set_err("ws_engine_create: no usable HIP device %d (use WS_ENGINE_DRY_RUN to validate without a GPU)", device);
      rc = WS_ERR_LAUNCH;
    } else {
      e->cu_count = prop.multiProcessorCount;
    }
  }
  if (rc == WS_OK) rc = prepare(e);
  if (rc != WS_OK) {
    ws_engine_destroy(e);
    return rc;
  }
  *out = e;
  return WS_OK;
}

// WS_ENGINE_RAGGED_SPK=0: the speaker stage of a ragged call runs one enrollment at a time, as it did before the batched
// pass existed (an escape hatch and a measurement arm, like WS_ENGINE_SERIALIZE)
static bool ragged_speaker_enabled() {
  static const bool on = !(getenv("WS_ENGINE_RAGGED_SPK") != nullptr && atoi(getenv("WS_ENGINE_RAGGED_SPK")) == 0);
  return on;
}

WS_ENGINE_API long long ws_engine_info(const ws_engine* e, const char* key) {
  if (!e || !key) return -1;
  const std::string k(key);
  if (k == "n_tensors") return static_cast<long long>(e->tensors.size());
  if (k == "n_launches") return e->n_launches;
  if (k == "arena_bytes") return static_cast<long long>(e->work.peak_bytes);
  if (k == "cluster_fallbacks") return e->cluster_fallbacks;
  if (k == "nband") return e->bs.K;
  if (k == "arch") return e->arch;
  if (k == "spk_pool" && (e->arch == 0 || e->arch == 2)) return e->spk.pool;   // meta, or the encoder's default
  // 1: enroll_lengths of ws_engine_separate_ragged run the speaker encoder once over all rows; 0: one row at a time
  if (k == "ragged_speaker") return (e->arch == 0 || e->arch == 3) && ragged_speaker_covered(e) && ragged_speaker_enabled() ? 1 : 0;
  // 1: lengths of ws_engine_separate_ragged are taken (pBSRNN, TF-GridNet); 0: this separator refuses them
  if (k == "ragged_separator") return e->arch == 0 || e->arch == 3 ? 1 : 0;
  // windows per target speaker and separator forwards of the last ws_engine_separate_long (0 after any other call)
  if (k == "long_windows") return e->long_windows;
  if (k == "long_forwards") return e->long_forwards;
  // 1: ws_engine_stream_open takes this container (causal cLN Conv-TasNet / SpEx+); the state bytes of the stream opened last
  if (k == "streaming") return tas_streamable(e) ? 1 : 0;
  if (k == "stream_state_bytes") return e->stream_state_bytes;
  // the live handle opened last: its one device allocation; the handle that ran last: windows since its open / reset, groups of
  // its last call
  if (k == "live_state_bytes") return e->live_state_bytes;
  if (k == "live_windows") return e->live_windows;
  if (k == "live_groups") return e->live_groups;
  // the live pool opened last: its one device allocation; the pool that ran last: rounds and forwards of its last push or flush
  if (k == "live_pool_state_bytes") return e->live_pool_state_bytes;
  if (k == "live_pool_rounds") return e->live_pool_rounds;
  if (k == "live_pool_forwards") return e->live_pool_forwards;
  // the tail pool opened last: its one device allocation; the pool that ran last: forwards and rows of its last tick or flush
  if (k == "tail_pool_state_bytes") return e->tail_pool_state_bytes;
  if (k == "tail_pool_forwards") return e->tail_pool_forwards;
  if (k == "tail_pool_rows") return e->tail_pool_rows;
  // the same three of the rate tail pool
  if (k == "rate_tail_pool_state_bytes") return e->rate_tail_pool_state_bytes;
  if (k == "rate_tail_pool_forwards") return e->rate_tail_pool_forwards;
  if (k == "rate_tail_pool_rows") return e->rate_tail_pool_rows;
  auto it = e->meta.find(k);
  return it == e->meta.end() ? -1 : it->second;
}

namespace wsrt {

// frames of an enrollment of `enroll_len` samples / frames for this model's front-end, or WS_ERR_INVALID (message set)
static int enroll_frames(const ws_engine* e, int enroll_kind, int enroll_len, int* frames) {
  int Te = enroll_len;
  if (enroll_kind == WS_ENROLL_WAVE && e->spk.feat) {          // kaldi fbank, snip-edges framing
    if (enroll_len < e->spk.fb_win) {
      set_err("ws_engine_separate: enrollment shorter than one %d-sample frame", e->spk.fb_win);
      return WS_ERR_INVALID;
    }
    Te = 1 + (enroll_len - e->spk.fb_win) / e->spk.fb_shift;
  } else if (enroll_kind == WS_ENROLL_WAVE) {                  // in-model MelSpectrogram, centred framing
    if (enroll_len <= 256) {
      set_err("ws_engine_separate: enrollment must be longer than the 256-sample reflect padding");
      return WS_ERR_INVALID;
    }
    Te = 1 + enroll_len / kHop;
  } else if (enroll_kind == WS_ENROLL_FBANK && !e->spk.feat) {
    set_err("ws_engine_separate: this model computes its own features (spk_feat = False): pass the waveform");
    return WS_ERR_INVALID;
  }
  if (enroll_kind != WS_ENROLL_EMBEDDING && enroll_kind != WS_ENROLL_SPEAKER && Te < 8) {
    set_err("ws_engine_separate: enrollment of %d frames is too short for the speaker encoder", Te);
    return WS_ERR_INVALID;
  }
  *frames = Te;
  return WS_OK;
}

int check_rows(ws_engine* e, bool ptrs, int R, int T) {
  if (e->arch == 1) return tasnet_check_rows(e, ptrs, R, T);
  // (TF-GridNet's own lower bound is 2 * n_fft, checked below: a ragged row of that length is compared with this call)
  const int t_min = e->arch == 3 && T >= 2 * e->grid.n_fft ? 2 * e->grid.n_fft : 512;
  if (!ptrs || R < 1 || T < t_min || (long long)R * (1 + T / kHop) * 4 * kNBin > 0x7fffffffLL) {
    set_err("ws_engine_separate: bad arguments (R=%d, T=%d; T >= 512)", R, T);
    return WS_ERR_INVALID;
  }
  if (e->arch == 3) {
    const GridNet& gn = e->grid;
    // (any sample count: the standard-deviation scaling that ties the Python path to multiples of 4 samples runs on the host here)
    if (T < 2 * gn.n_fft || (long long)R * (1 + T / gn.hop) * gn.Q * (2 * gn.nh * gn.E + gn.C) > 0x7fffffffLL) {
      set_err("ws_engine_separate: a TF-GridNet engine needs T >= %d and R * frames * bins * %d below 2^31 (R=%d, T=%d)",
              2 * gn.n_fft, 2 * gn.nh * gn.E + gn.C, R, T);
      return WS_ERR_INVALID;
    }
  }
  if (e->arch == 2 && (T < 31 * kHop || (long long)R * (1 + T / kHop) * kDpBins * 160 > 0x7fffffffLL)) {
    set_err("ws_engine_separate: a DPCCN engine needs T >= %d samples (32 frames for the AvgPool2d(32) branch) and "
            "R * frames * 257 * 160 below 2^31 (R=%d, T=%d)", 31 * kHop, R, T);
    return WS_ERR_INVALID;
  }
  return WS_OK;
}

int check_enroll(ws_engine* e, int R, int enroll_kind, int enroll_len, const int* enroll_lengths, int* Te,
                 std::vector<int>* te_row) {
  int rc;
  if (e->arch == 1) {
    if (enroll_lengths) {
      set_err("ws_engine_separate_ragged: per-row lengths are built for pBSRNN (arch 0) and TF-GridNet (arch 3) only; this "
              "container holds arch %d", e->arch);
      return WS_ERR_INVALID;
    }
    *Te = enroll_len;
    return tasnet_check_enroll(e, enroll_kind, enroll_len);
  }
  const bool fits = enroll_kind == WS_ENROLL_SPEAKER ? e->joint != 0 : (enroll_kind == WS_ENROLL_EMBEDDING) != (e->joint != 0);
  if (!fits || enroll_kind < 0 || enroll_kind > WS_ENROLL_SPEAKER) {
    set_err("ws_engine_separate: enrollment kind %d does not fit this model (joint_training = %d)", enroll_kind, e->joint);
    return WS_ERR_INVALID;
  }
  if ((rc = enroll_frames(e, enroll_kind, enroll_len, Te)) != WS_OK) return rc;
  if (enroll_lengths) {
    if (enroll_kind == WS_ENROLL_EMBEDDING || enroll_kind == WS_ENROLL_SPEAKER) {
      set_err("ws_engine_separate_ragged: enroll_lengths given with fixed embeddings (they have no length)");
      return WS_ERR_INVALID;
    }
    te_row->resize(R);
    for (int r = 0; r < R; ++r) {
      if (enroll_lengths[r] > enroll_len) {
        set_err("ws_engine_separate_ragged: enroll_lengths[%d] = %d exceeds the row pitch enroll_len = %d", r,
                enroll_lengths[r], enroll_len);
        return WS_ERR_INVALID;
      }
      if ((rc = enroll_frames(e, enroll_kind, enroll_lengths[r], &(*te_row)[r])) != WS_OK) return rc;
    }
  }
  return WS_OK;
}

static std::mutex g_device_mutex[16];   // see ForwardTurn
static thread_local int g_turn_depth[16];   // turns this thread holds per device: only the outermost one locks

// Engines that share a GPU overlap on the device.  Round 2 serialised them here (one forward at a time per GPU)
// because ws_gemm_b2p / the grouped ws_gemm_nt / ws_gemm_tn disturbed this plan's STFT / iSTFT kernels on another
// stream.  Round 3 named the victim class -- packed FP32 instructions with an operand selection -- and the library is
// built without them (profiles/r03_kernel_race.md; tests/test_cross_stream_gpu.py), so the lock is opt-in:
// WS_ENGINE_SERIALIZE=1 restores one forward at a time (e.g. beside third-party kernels on the same GPU).
ForwardTurn::ForwardTurn(ws_engine* e) : turn(g_device_mutex[e->device & 15], std::defer_lock) {
  static const bool serialize = getenv("WS_ENGINE_SERIALIZE") != nullptr && atoi(getenv("WS_ENGINE_SERIALIZE")) != 0;
  if (!e->dry && hipSetDevice(e->device) != hipSuccess) {
    set_err("ws_engine_separate: hipSetDevice(%d) failed", e->device);
    rc = WS_ERR_LAUNCH;
    return;
  }
  if (serialize) {
    nested = e->device & 15;
    if (g_turn_depth[nested]++ == 0) turn.lock();
  }
}

ForwardTurn::~ForwardTurn() {
  if (nested >= 0) --g_turn_depth[nested];      // (the outermost turn of the thread owns the lock and releases it last)
}

// the speaker stage of every forward: host enrollment -> device emb [R][E], the encoder's embedding before SpeakerTransform
// (what the plans receive as emb_in).  Fixed embeddings and WS_ENROLL_SPEAKER are uploaded where the encoder would write.
int speaker_stage(ws_engine* e, const void* enroll, int enroll_kind, int R, int enroll_len, int Te, const int* enroll_lengths,
                  const int* te_row, float* d_emb) {
  int rc;
  if (enroll_kind == WS_ENROLL_EMBEDDING || enroll_kind == WS_ENROLL_SPEAKER) {
    if ((rc = to_device(e, d_emb, enroll, size_t(R) * e->E * 4)) != WS_OK) return rc;
  } else if (e->arch == 1) {
    // SpEx+: the enrollment waveform through the separator's own encoder (convtasnet.py:179-187)
    if ((rc = tasnet_speaker(e, static_cast<const float*>(enroll), R, enroll_len, d_emb)) != WS_OK) return rc;
  } else if (enroll_lengths && ragged_speaker_covered(e) && ragged_speaker_enabled()) {
    // one encoder pass over all rows: masked epilogues keep every row zero behind its own frames, the reductions over
    // time take the row's length (speaker.cc)
    if ((rc = speaker_embed(e, enroll, enroll_kind, R, enroll_len, Te, d_emb, enroll_lengths, te_row)) != WS_OK) return rc;
  } else if (enroll_lengths) {
    // CAM++, the attentive multi-head pools, WS_ENGINE_RAGGED_SPK=0: one enrollment at a time into the [R][E] buffer
    // (its convolutions then pad with zeros at the row's true end and its pooling sees the row's own frames), then the
    // separator once over all rows
    const size_t pitch = size_t(enroll_len) * (enroll_kind == WS_ENROLL_FBANK ? e->spk.feat_dim : 1);
    for (int r = 0; r < R; ++r)
      if ((rc = speaker_embed(e, static_cast<const float*>(enroll) + r * pitch, enroll_kind, 1, enroll_lengths[r], te_row[r],
                              d_emb + size_t(r) * e->E)) != WS_OK)
        return rc;
  } else if ((rc = speaker_embed(e, enroll, enroll_kind, R, enroll_len, Te, d_emb)) != WS_OK) {
    return rc;
  }
  return WS_OK;
}

int note_cluster_status(ws_engine* e) {
  if (e->cl_status && !e->dry) {   // did a cluster recurrence time out (and the predicated streaming pair repair it)?
    unsigned st = 0;
    int rc;
    if ((rc = to_host(e, &st, e->cl_status, 4)) != WS_OK) return rc;
    if (st) {
      ++e->cluster_fallbacks;
      if ((rc = zero_device(e, e->cl_status, 4)) != WS_OK) return rc;
    }
  }
  return WS_OK;
}

void row_std_scale(const float* x, int n, float* std_out, float* scaled) {
  double m = 0.0, v = 0.0;
  for (int i = 0; i < n; ++i) m += x[i];
  m /= n;
  for (int i = 0; i < n; ++i) v += (x[i] - m) * (x[i] - m);
  *std_out = static_cast<float>(sqrt(v / (n - 1.0)));
  if (!scaled) return;
  const float inv = 1.0f / *std_out;
  for (int i = 0; i < n; ++i) scaled[i] = x[i] * inv;
}

// ws_engine_separate and ws_engine_separate_ragged: lengths / enroll_lengths = nullptr is the rectangular call
int separate_impl(ws_engine* e, const float* mix, int R, int T, const int* lengths, const void* enroll, int enroll_kind,
                  int enroll_len, const int* enroll_lengths, float* est) {
  int rc = check_engine(e, lengths || enroll_lengths ? "ws_engine_separate_ragged" : "ws_engine_separate");
  if (rc != WS_OK) return rc;
  if ((lengths || enroll_lengths) && e->arch != 0 && e->arch != 3) {
    set_err("ws_engine_separate_ragged: per-row lengths are built for pBSRNN (arch 0) and TF-GridNet (arch 3) only; this "
            "container holds arch %d", e->arch);
    return WS_ERR_INVALID;
  }
  e->long_windows = e->long_forwards = 0;
  if (e->arch == 1) return tasnet_separate(e, mix, R, T, enroll, enroll_kind, enroll_len, est);
  if ((rc = check_rows(e, mix && enroll && est, R, T)) != WS_OK) return rc;
  int Te = enroll_len;
  std::vector<int> tf, te_row;
  if ((rc = check_enroll(e, R, enroll_kind, enroll_len, nullptr, &Te, &te_row)) != WS_OK) return rc;
  if (lengths) {
    // a row's own T: what this surface demands of T, and no more than the row pitch; frames with the model's own hop
    const int lo = e->arch == 3 ? 2 * e->grid.n_fft : 512, hop = e->arch == 3 ? e->grid.hop : kHop;
    for (int r = 0; r < R; ++r) {
      if (lengths[r] < lo || lengths[r] > T) {
        set_err("ws_engine_separate_ragged: lengths[%d] = %d outside [%d, T = %d]", r, lengths[r], lo, T);
        return WS_ERR_INVALID;
      }
      tf.push_back(1 + lengths[r] / hop);
    }
  }
  if (enroll_lengths && (rc = check_enroll(e, R, enroll_kind, enroll_len, enroll_lengths, &Te, &te_row)) != WS_OK) return rc;
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->n_launches = 0;
  Arena& a = e->work;
  a.reset();
  float* d_mix = a.alloc(size_t(R) * T);
  float* d_est = a.alloc(size_t(R) * T);
  float* d_emb = a.alloc(size_t(R) * e->E);
  WS_PTR(d_mix && d_est && d_emb);
  // TF-GridNet scales the mixture by its (unbiased) standard deviation and the estimate back (tfgridnet.py:222-226,292);
  // a ragged row over its own samples (the tail of the scaled copy is zeros: nothing behind a length is read)
  std::vector<float> mixn, stds;
  if (e->arch == 3) {
    mixn.assign(size_t(R) * T, 0.f);
    stds.resize(R);
    for (int r = 0; r < R; ++r) row_std_scale(mix + size_t(r) * T, lengths ? lengths[r] : T, &stds[r], mixn.data() + size_t(r) * T);
    mix = mixn.data();
  }
  if ((rc = to_device(e, d_mix, mix, size_t(R) * T * 4)) != WS_OK) return rc;
  int *d_len = nullptr, *d_tf = nullptr;
  if (lengths) {
    d_len = reinterpret_cast<int*>(a.alloc(R));
    d_tf = reinterpret_cast<int*>(a.alloc(R));
    WS_PTR(d_len && d_tf);
    if ((rc = to_device(e, d_len, lengths, size_t(R) * 4)) != WS_OK || (rc = to_device(e, d_tf, tf.data(), size_t(R) * 4)) != WS_OK)
      return rc;
  }
  if ((rc = speaker_stage(e, enroll, enroll_kind, R, enroll_len, Te, enroll_lengths, te_row.data(), d_emb)) != WS_OK) return rc;
  rc = e->arch == 2 ? dpccn_device(e, d_mix, R, T, d_emb, d_est)
                    : e->arch == 3 ? gridnet_device(e, d_mix, R, T, d_emb, d_est, lengths ? tf.data() : nullptr, d_len, d_tf)
                                   : separate_device(e, d_mix, R, T, d_emb, d_est, d_len, d_tf);
  if (rc != WS_OK) return rc;
  if ((rc = to_host(e, est, d_est, size_t(R) * T * 4)) != WS_OK) return rc;
  if (e->arch == 3 && !e->dry)
    for (int r = 0; r < R; ++r)
      for (int i = 0, n = lengths ? lengths[r] : T; i < n; ++i) est[size_t(r) * T + i] *= stds[r];
  if ((rc = note_cluster_status(e)) != WS_OK) return rc;
  a.reset();
  a.consolidate();
  return WS_OK;
}

}  // namespace wsrt

WS_ENGINE_API int ws_engine_separate(ws_engine* e, const float* mix, int R, int T, const void* enroll, int enroll_kind,
                                  int enroll_len, float* est) {
  return separate_impl(e, mix, R, T, nullptr, enroll, enroll_kind, enroll_len, nullptr, est);
}

WS_ENGINE_API int ws_engine_separate_ragged(ws_engine* e, const float* mix, int R, int T, const int* lengths, const void* enroll,
                                         int enroll_kind, int enroll_len, const int* enroll_lengths, float* est) {
  return separate_impl(e, mix, R, T, lengths, enroll, enroll_kind, enroll_len, enroll_lengths, est);
}

// the speaker stage alone: what a service with one enrolled user runs once, to pass the result as WS_ENROLL_SPEAKER
WS_ENGINE_API int ws_engine_embed(ws_engine* e, const void* enroll, int enroll_kind, int R, int enroll_len, const int* enroll_lengths,
                               float* emb) {
  int rc = check_engine(e, "ws_engine_embed");
  if (rc != WS_OK) return rc;
  if (!e->joint) {
    set_err("ws_engine_embed: this container takes fixed embeddings (joint_training = 0): it holds no speaker encoder");
    return WS_ERR_INVALID;
  }
  if (!enroll || !emb || R < 1 || (enroll_kind != WS_ENROLL_FBANK && enroll_kind != WS_ENROLL_WAVE)) {
    set_err("ws_engine_embed: bad arguments (R=%d, enrollment kind %d; WS_ENROLL_FBANK or WS_ENROLL_WAVE)", R, enroll_kind);
    return WS_ERR_INVALID;
  }
  if (enroll_lengths && e->arch != 0 && e->arch != 3) {
    set_err("ws_engine_embed: per-row lengths are built for pBSRNN (arch 0) and TF-GridNet (arch 3) only; this container "
            "holds arch %d", e->arch);
    return WS_ERR_INVALID;
  }
  int Te = enroll_len;
  std::vector<int> te_row;
  if ((rc = check_enroll(e, R, enroll_kind, enroll_len, enroll_lengths, &Te, &te_row)) != WS_OK) return rc;
  ForwardTurn turn(e);
  if (turn.rc != WS_OK) return turn.rc;
  e->long_windows = e->long_forwards = 0;
  e->n_launches = 0;
  Arena& a = e->work;
  a.reset();
  float* d_emb = a.alloc(size_t(R) * e->E);
  WS_PTR(d_emb);
  if ((rc = speaker_stage(e, enroll, enroll_kind, R, enroll_len, Te, enroll_lengths, te_row.data(), d_emb)) != WS_OK) return rc;
  if ((rc = to_host(e, emb, d_emb, size_t(R) * e->E * 4)) != WS_OK) return rc;
  a.reset();
  a.consolidate();
  return WS_OK;
}

WS_ENGINE_API int ws_engine_separate_long(ws_engine* e, const float* mix, int n, int K, const void* enroll, int enroll_kind,
                                       int enroll_len, const int* enroll_lengths, int window, int overlap, int max_rows,
                                       float* est) {
  return separate_long(e, mix, n, K, enroll, enroll_kind, enroll_len, enroll_lengths, window, overlap, max_rows, est);
}

WS_ENGINE_API int ws_engine_forward_pcm16(ws_engine* e, const int16_t* mix, int n, const int16_t* spk1, const int16_t* spk2,
                                       int n_enroll, float* out) {
  int rc = check_engine(e, "ws_engine_forward_pcm16");
  if (rc != WS_OK) return rc;
  if (!mix || !spk1 || !spk2 || !out || n < 512 || n_enroll < 1) {
    set_err("ws_engine_forward_pcm16: bad arguments");
    return WS_ERR_INVALID;
  }
  // separate_engine.cc:78-98: the mixture twice (one row per enrollment), scaled to [-1, 1]; the enrollment fbank is
  // computed on int16-valued samples, which the folded basis' 2^15 factor reproduces from the [-1, 1] rows
  std::vector<float> m(size_t(2) * n), enr(size_t(2) * n_enroll);
  for (int i = 0; i < n; ++i) m[i] = m[size_t(n) + i] = static_cast<float>(mix[i]) / 32768.0f;
  for (int i = 0; i < n_enroll; ++i) {
    enr[i] = static_cast<float>(spk1[i]) / 32768.0f;
    enr[size_t(n_enroll) + i] = static_cast<float>(spk2[i]) / 32768.0f;
  }
  return ws_engine_separate(e, m.data(), 2, n, enr.data(), WS_ENROLL_WAVE, n_enroll, out);
}
