/* wesep_engine.h -- C ABI of libwesep_engine.so, the native (C++) inference runtime of wesep_amd for MI355X.
 *
 * MI355X counterpart of the reference's C++ runtime:
 *   runtime/separate/separate_engine.h:31-57  class SeparateEngine {ctor(model_path, feat_dim, sample_rate),
 *                                              ExtractFeature, ApplyMean, ForwardFunc(mix, spk1, spk2, output)}
 *   runtime/separate/separate_engine.cc:37-123 (TorchScript module on LibTorch-CPU, kaldi fbank + CMN on the host)
 * and of the whole-utterance forward of wesep/bin/infer.py:94-118.
 *
 * The reference loads a TorchScript archive; this engine loads a flat weight container written by
 * `python -m wesep_amd.bin.export_engine` (the `state_dict` under the reference's own key names, see INTEGRATION.md;
 * meta key "arch": 0 pBSRNN, 1 Conv-TasNet / SpEx+, 2 DPCCN, 3 TF-GridNet -- ws_engine_info(e, "arch")) and runs the forward as a
 * fixed launch plan over include/wesep_hip.h: weights are uploaded and
 * packed into MFMA fragment order ONCE at load, activations live in one grow-only device arena with stack
 * discipline, the enrollment front-end (kaldi fbank + CMN as two GEMMs, include/wesep_hip.h) and the jointly
 * trained ResNet speaker encoder (eval mode: BatchNorm folded to its running statistics) run on the device too.
 * Host buffers in, host buffers out; the engine owns its HIP stream and device memory.  One engine per GPU and
 * thread.  Return value: 0 or a negative WS_ERR_* code of wesep_hip.h, message via ws_engine_last_error().
 */
#ifndef WESEP_ENGINE_H_
#define WESEP_ENGINE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WS_ENGINE_ABI_VERSION 2

typedef struct ws_engine ws_engine;

/* flags of ws_engine_create */
#define WS_ENGINE_DRY_RUN 1 /* no GPU needed: host memory stands in for device memory and every launch is allowed to
                               fail with WS_ERR_LAUNCH, but every entry point's ARGUMENT validation must pass
                               (WS_ERR_INVALID still aborts).  Validates a weight container and the launch plan of a
                               given geometry on a machine without a GPU (refused when a HIP device is visible, where
                               the launches would execute); computes nothing (outputs are left untouched). */

int ws_engine_abi_version(void);
const char* ws_engine_last_error(void);

/* Loads the container, uploads and packs the weights on HIP device `device`.
 * Replaces SeparateEngine::SeparateEngine (separate_engine.cc:37-51: torch::jit::load + feature pipeline setup). */
int ws_engine_create(const char* weights_path, int device, int flags, ws_engine** out);
void ws_engine_destroy(ws_engine* e);

/* Model facts read from the container: key in {"sample_rate", "num_repeat", "spk_emb_dim", "joint_training",
 * "feat_dim", "n_tensors", "n_launches" (entry-point calls issued by the last forward), "arena_bytes",
 * "cluster_fallbacks" (forwards so far in which a weight-stationary cluster recurrence timed out -- its workgroups were
 * not co-resident, e.g. several engines on one GPU -- and the predicated streaming kernels recomputed the layer;
 * wesep_hip.h, ws_lstm_fwd_cluster), "ragged_speaker" (1: enroll_lengths of ws_engine_separate_ragged run the speaker
 * encoder once over all rows, 0: one row at a time), "ragged_separator" (1: the separator takes the lengths of
 * ws_engine_separate_ragged -- pBSRNN and TF-GridNet; 0: it refuses them), "long_windows" / "long_forwards" (windows per
 * target speaker and separator forwards of the last ws_engine_separate_long; 0 after any other call), "causal" / "norm"
 * (Conv-TasNet containers: 1 / 1 for causal blocks with cLN; absent, i.e. -1, in containers written before these keys, which
 * load as non-causal gLN), "streaming" (1: ws_engine_stream_open takes this container), "stream_state_bytes" (device state
 * of the stream or stream pool opened last)}; unknown key -> -1. */
long long ws_engine_info(const ws_engine* e, const char* key);

/* enrollment kinds */
#define WS_ENROLL_EMBEDDING 0 /* float [R][spk_emb_dim]: fixed speaker embeddings (joint_training = False models) */
#define WS_ENROLL_FBANK 1     /* float [R][enroll_len][feat_dim]: mean-normalised fbank (joint models, spk_feat True) */
#define WS_ENROLL_WAVE 2      /* float [R][enroll_len] in [-1, 1].  spk_feat = True models: kaldi fbank (dither 0) + CMN
                                 computed on the device (what SeparateEngine::ExtractFeature does on the host,
                                 separate_engine.cc:53-74); spk_feat = False models: their in-model PreEmphasis +
                                 MelSpectrogram + log + CMN front-end (bsrnn.py:343-350) */
#define WS_ENROLL_SPEAKER 3   /* float [R][spk_emb_dim]: what ws_engine_embed returned (joint containers) */

/* est[r][0..T) = target-speaker estimate for mix[r][0..T) given enrollment r.  All pointers are HOST pointers.
 * Replaces `model(features, enroll)[0]` of infer.py:101-103 (whole utterance, any T >= 512; ws_engine_separate_long
 * below cuts a long recording into windows). */
int ws_engine_separate(ws_engine* e, const float* mix, int R, int T, const void* enroll, int enroll_kind,
                       int enroll_len, float* est);

/* Ragged batches (engine ABI 2; pBSRNN and TF-GridNet containers, arch 0 and 3): utterances of different lengths in ONE
 * forward.  mix / est keep the row pitch T; lengths[r] in [512, T] (TF-GridNet: [2 n_fft, T]) is the number of valid samples
 * of row r.  est[r][0..lengths[r]) is what
 * ws_engine_separate returns for mix[r][0..lengths[r]) as a batch of one (reflect padding, GroupNorm statistics, the
 * reverse recurrence over time and the iSTFT envelope all end at the row's own end); est[r][lengths[r]..T) = 0; what the
 * caller left in mix[r][lengths[r]..T) is never read into a valid output (NaN included).
 * enroll_lengths (HOST int [R], or NULL = every row has enroll_len): valid samples (WS_ENROLL_WAVE) / frames
 * (WS_ENROLL_FBANK) of each enrollment row of pitch enroll_len.  The speaker stage is ragged too: the ResNets and
 * ECAPA-TDNN (TSTP / TAP / TSDP / ASTP pooling) run ONCE over all R enrollment rows -- every layer's input is exactly
 * zero behind the row's own width, which follows the convolutions' geometry, and the reductions over time (pooling, the
 * SE mean, CMN) take the row's length; each row gets the embedding it gets as a batch of one, and what the caller left
 * behind enroll_lengths[r] never reaches it (NaN included).  ws_engine_info(e, "ragged_speaker") is 1 for such a
 * container.  CAM++ and the MHASTP / MQMHASTP pools report 0 and run one enrollment at a time, as does every container
 * with WS_ENGINE_RAGGED_SPK=0 in the environment; the separator runs once over all rows either way.
 * lengths = enroll_lengths = NULL is ws_engine_separate (any architecture); with either given, a Conv-TasNet or DPCCN
 * container is refused (WS_ERR_INVALID).  The recurrences over time of a ragged call (pBSRNN's time view, TF-GridNet's
 * inter-frame path) run over precomputed gates (the rows' tails are zeroed there); the number of launches depends on
 * (R, T) only, not on the lengths.  TF-GridNet: the row's standard deviation, its scaling and the scale-back run over its
 * own samples; the frames follow the model's hop; the keys behind a row's last frame are masked out of the attention. */
int ws_engine_separate_ragged(ws_engine* e, const float* mix, int R, int T, const int* lengths, const void* enroll,
                              int enroll_kind, int enroll_len, const int* enroll_lengths, float* est);

/* The speaker stage alone (joint containers): emb[r] = the speaker encoder's embedding of enrollment r, BEFORE the model's
 * SpeakerTransform -- what the separator receives from the speaker stage of ws_engine_separate.  enroll / enroll_kind
 * (WS_ENROLL_FBANK or WS_ENROLL_WAVE) / enroll_len / enroll_lengths (or NULL; pBSRNN and TF-GridNet containers) as in
 * ws_engine_separate_ragged, and the same passes run: once over all rows where "ragged_speaker" is 1, one row at a time
 * otherwise (WS_ENGINE_RAGGED_SPK=0 included); a SpEx+ container runs its encoder on the waveform.  emb: HOST
 * [R][spk_emb_dim].  Passing it back as WS_ENROLL_SPEAKER (ws_engine_separate, _ragged, _long) uploads it where the speaker
 * stage would have written: with the same R the estimates are bit for bit those of the call with the raw enrollment, and
 * the encoder does not run.  A container that takes fixed embeddings has no speaker stage and is refused. */
int ws_engine_embed(ws_engine* e, const void* enroll, int enroll_kind, int R, int enroll_len, const int* enroll_lengths,
                    float* emb);

/* Long recordings: ONE mixture mix [n], K >= 1 target speakers (enroll: K rows, any kind the container takes), est HOST
 * [K][n].  The mixture is cut into W windows of `window` samples that overlap by `overlap` (0 <= overlap <= window / 2;
 * hop = window - overlap): W = 1 + ceil((n - window) / hop), window w starts at min(w hop, n - window) -- the last one is
 * aligned to the end, so every window has full length and the architecture's rectangular plan runs on it.  The K W rows
 * go through the separator in groups of at most max_rows rows (the arena holds one group's working set); a row is what
 * ws_engine_separate makes of it as a mixture of its own (TF-GridNet: the window's own standard deviation and scale-back;
 * a window of constant samples has none, as in the whole-utterance call).  The estimates are cross-faded on the device:
 * linear ramps over the overlapping samples, normalised by the sum of the weights that cover a sample (wesep_hip.h,
 * ws_xfade_ola), in a fixed order.  The enrollment fixes which speaker comes out, so windows need no permutation alignment.
 * The speaker stage runs ONCE over the K enrollments, or not at all (WS_ENROLL_EMBEDDING / WS_ENROLL_SPEAKER).
 * n <= window with K <= max_rows is ws_engine_separate on [K][n], bit for bit.  Refused before any launch: a window below
 * the architecture's minimum T (its own message), overlap outside [0, window / 2], max_rows < 1, a group of
 * min(max_rows, K W) rows of `window` samples over the architecture's 2^31 guard, and a Conv-TasNet window that is not
 * L + k L / 2 samples (its last samples would be the plan's zero extension, not model output).  Memory and time grow
 * linearly in n; "long_windows" / "long_forwards" of ws_engine_info report W and the number of groups. */
int ws_engine_separate_long(ws_engine* e, const float* mix, int n, int K, const void* enroll, int enroll_kind, int enroll_len,
                            const int* enroll_lengths, int window, int overlap, int max_rows, float* est);

/* Streaming (new symbols, engine ABI 2 unchanged): a causal cLN Conv-TasNet / SpEx+ container (meta "causal" = 1, "norm" = 1;
 * ws_engine_info(e, "streaming") == 1) fed audio as it arrives, in chunks of any size.  The concatenation of what the pushes
 * and the flush return is the model-output part of ws_engine_separate's row on the concatenated input: its first
 * (T' - 1) s + L samples, T' = (N - L) / s + 1, s = L / 2, to the rounding of a forward over another number of frames.  Every
 * encoder frame, block frame and output sample is computed once.  All pointers are HOST pointers.
 *
 * Emission rule, with N samples pushed so far: frame k runs once k s + 160 <= N (160: the longest encoder window); after K
 * frames, K s samples a row have been returned.  ws_engine_stream_push(chunk [rows][n], n >= 1) writes the samples that
 * became final to est [rows][*n_out] (row pitch *n_out, possibly 0); est must hold est_cap >= *n_out samples a row --
 * WS_STREAM_PUSH_CAP(n, L) always suffices.  ws_engine_stream_flush zero-extends the pending samples as the whole-utterance
 * encoder does, runs the frames up to T' and returns the rest ((T' - 1) s + L samples in all; at most WS_STREAM_FLUSH_CAP a
 * row in this call).  ws_engine_stream_reset returns to sample 0 and keeps the enrollment.
 *
 * ws_engine_stream_open runs the speaker stage once -- enrollment kinds as for ws_engine_separate on this container:
 * WS_ENROLL_EMBEDDING for fixed embeddings, WS_ENROLL_WAVE or WS_ENROLL_SPEAKER for SpEx+ --, then SpeakerTransform and the
 * row biases W_e e + b of the stacks' first blocks, and keeps the results.  A container that is not arch 1 with causal blocks
 * and cLN is refused by name.  Carried state is ONE device allocation owned by the stream, made at open and freed at close:
 * per block a ring [rows][(P - 1) dil + max_chunk_frames][H] of normalised frames, the overlap-add carry [rows][L - s]
 * (reset: the decoder bias), two pending-sample buffers [rows][max_chunk_frames s + 160] used in turn, the embedding and
 * the row biases.  It does not grow with n: frames run in groups of at most max_chunk_frames, and a long chunk is taken in
 * pieces.  Transient activations come from the engine's arena and are returned before the call ends, so any other engine
 * call between two pushes leaves the stream as it was, and several streams may be open on one engine (callers serialise, as
 * for every engine call).  Close every stream before ws_engine_destroy.
 *
 * Launches: a group of frames is WS_STREAM_GROUP_LAUNCHES(R, X) = 3 R X + 10 entry-point calls -- 3 framing GEMMs, row
 * statistics, projection; per block GEMM, ws_tcn_mid_stream_fwd, GEMM; mask GEMM, ws_maskmul_fwd, synthesis GEMM,
 * ws_ola_stream_fwd; the copy of the unconsumed pending samples to the other buffer.  ws_engine_info(e, "n_launches") after
 * a push or flush is that figure times the groups the call ran (0 when no frame became complete); it does not depend on n
 * for a push that runs one group.  The copies to and from the host are not counted.  One host synchronisation per push, on
 * the engine's own stream, after the device-to-host copy.
 * WS_ERR_INVALID with a message and nothing launched: est_cap below what the call emits, flush with N < L, push or flush after
 * a flush, n < 1, a NULL pointer. */
#define WS_STREAM_PUSH_CAP(n, L) (((n) / ((L) / 2) + 1) * ((L) / 2))
#define WS_STREAM_FLUSH_CAP 160
#define WS_STREAM_GROUP_LAUNCHES(R, X) (3 * (R) * (X) + 10)
typedef struct ws_stream ws_stream;
int ws_engine_stream_open(ws_engine* e, int rows, const void* enroll, int enroll_kind, int enroll_len, int max_chunk_frames,
                          ws_stream** out);
int ws_engine_stream_push(ws_stream* s, const float* chunk, int n, float* est, int est_cap, int* n_out);
int ws_engine_stream_flush(ws_stream* s, float* est, int est_cap, int* n_out);
int ws_engine_stream_reset(ws_stream* s);
void ws_engine_stream_close(ws_stream* s);

/* Stream pool (new symbols, engine ABI 2 unchanged): MANY independent streams on one engine -- calls that start at different
 * times and deliver packets of different sizes -- through ONE launch chain per round.  A ws_stream's rows all sit at the same
 * sample position; N of them pushed one after another cost N launch chains.  In a causal cLN model every frame depends on
 * earlier frames of its own row only, and the two kernels that look across time take a per-row position, frame count and
 * state slot (wesep_hip.h: ws_tcn_mid_stream_rows_fwd, ws_ola_stream_rows_fwd), so any set of streams shares one rectangle.
 * Each slot is one stream with the emission rule, the outputs and the error bound of a ws_stream with rows = 1.
 *
 *   ws_engine_pool_open(e, slots, max_chunk_frames, &pool)  makes the state: ONE device allocation, freed at close, that no
 *     push, attach or detach grows ("stream_state_bytes").  Per slot: per block a ring [(P - 1) dil + max_chunk_frames][H],
 *     the overlap-add carry [L - s], the embedding after SpeakerTransform, the stacks' row biases; and one carry reset image.
 *     The samples that have not completed a frame (fewer than 160 + s after a push) are kept on the HOST, per slot.
 *   ws_engine_pool_attach(pool, enroll, enroll_kind, enroll_len, &slot)  takes the lowest free slot, runs the speaker stage
 *     for this ONE enrollment (kinds as for ws_engine_stream_open with rows = 1), writes the slot's embedding and row biases
 *     and puts it at sample 0 (carry = the decoder bias; the rings need no clearing).  A full pool is refused by name.
 *   ws_engine_pool_push(pool, n_active, slots, chunks, n, est, est_cap, n_out)  one packet for each of n_active DISTINCT
 *     attached slots: chunks[i] is n[i] >= 1 samples for slots[i]; the samples of that slot that became final go to est[i]
 *     (est_cap[i] >= n_out[i]; WS_STREAM_PUSH_CAP(n[i], L) always suffices), their count to n_out[i] -- per slot the
 *     emission rule of ws_engine_stream_push.  The work is cut into groups: a slot that still owes frames joins a group with
 *     tc_i = min(frames owed, max_chunk_frames) of them, the group is the rectangle [A][Tc], A the slots in it, Tc = max tc_i,
 *     staged zero-filled on the host and uploaded once with its three tables.  Frames t >= tc_i of a row are computed on
 *     zeros by the GEMMs and consumed by nothing: the price of one rectangle, largest when one slot delivers a long packet
 *     beside short ones.  A group is WS_POOL_GROUP_LAUNCHES(R, X) = 3 R X + 9 entry-point calls whatever A is (a ws_stream's
 *     group without the pending-sample copy); "n_launches" after a push is that figure times its groups; a round in which
 *     every slot owes at most max_chunk_frames frames is one group.  One host synchronisation per push.
 *   ws_engine_pool_flush(pool, slot, est, est_cap, &n_out)  the end of ONE slot's stream, as ws_engine_stream_flush: the
 *     remaining frames on the zero-extended pending samples (groups with A = 1), then the carry; at most
 *     WS_STREAM_FLUSH_CAP samples.  The slot then takes no push or flush until it is detached.
 *   ws_engine_pool_detach(pool, slot)  frees the slot for the next attach.    ws_engine_pool_close(pool)  before
 *     ws_engine_destroy.
 * What one slot returns does not depend on what the other slots of a push carry (NaN and inf included): no launch mixes
 * rows.  All pointers are HOST pointers; callers serialise, as for every engine call.
 * WS_ERR_INVALID with a message and nothing launched: a container that cannot stream (the text of ws_engine_stream_open),
 * slots < 1, max_chunk_frames outside [1, 65536], slots x max_chunk_frames over the 2^31 guards of ws_engine_stream_open, a
 * full pool, a slot of a push or flush that is not attached, was flushed, or is named twice, n[i] < 1, est_cap[i] below what
 * the slot emits, a flush with fewer than L samples, a NULL pointer, and any call but detach and close after a push or flush
 * that failed half way, until the slots that call named are detached. */
#define WS_POOL_GROUP_LAUNCHES(R, X) (3 * (R) * (X) + 9)
typedef struct ws_pool ws_pool;
int ws_engine_pool_open(ws_engine* e, int slots, int max_chunk_frames, ws_pool** out);
/* The whole block as one call (new symbols, engine ABI 2 unchanged).  ws_engine_stream_open_ex / ws_engine_pool_open_ex are
 * the two opens above with a `flags` word; flags = 0 IS the plain open (which calls the _ex form with 0), an unknown bit is
 * WS_ERR_INVALID by name.  WS_STREAM_BLOCK_KERNEL: every block of a group is ONE entry-point call, ws_tcn_block_stream_fwd
 * (stream) or ws_tcn_block_stream_rows_fwd (pool), in place of GEMM, fused middle, GEMM: a group is framing GEMMs, row
 * statistics, projection, one call per block, mask GEMM, mask product, synthesis GEMM, overlap-add (and the pending copy of
 * the solo stream) -- WS_STREAM_BLOCK_GROUP_LAUNCHES(R, X) = R X + 10 and WS_POOL_BLOCK_GROUP_LAUNCHES(R, X) = R X + 9
 * entry-point calls.  The block kernel reduces every frame's products in one fixed order wherever the frame sits, so the
 * separator's part of a flagged stream does not depend on the packet sizes, nor a flagged pool slot's on its neighbours.
 * State layout, "stream_state_bytes", push, flush, reset, attach, detach, the one synchronisation per push, the dry run and
 * every refusal are those of the plain opens.  Containers with B above WS_TCN_BLOCK_MAXB or H above WS_TCN_BLOCK_MAXH
 * (wesep_hip.h) are refused by the kernel at the first push. */
#define WS_STREAM_BLOCK_KERNEL 1
#define WS_STREAM_BLOCK_GROUP_LAUNCHES(R, X) ((R) * (X) + 10)
#define WS_POOL_BLOCK_GROUP_LAUNCHES(R, X) ((R) * (X) + 9)
int ws_engine_stream_open_ex(ws_engine* e, int rows, const void* enroll, int enroll_kind, int enroll_len, int max_chunk_frames,
                             unsigned flags, ws_stream** out);
int ws_engine_pool_open_ex(ws_engine* e, int slots, int max_chunk_frames, unsigned flags, ws_pool** out);
int ws_engine_pool_attach(ws_pool* p, const void* enroll, int enroll_kind, int enroll_len, int* slot);
int ws_engine_pool_push(ws_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n, float* const* est,
                        const int* est_cap, int* n_out);
int ws_engine_pool_flush(ws_pool* p, int slot, float* est, int est_cap, int* n_out);
int ws_engine_pool_detach(ws_pool* p, int slot);
void ws_engine_pool_close(ws_pool* p);

/* Sample rates (new symbols, engine ABI 2 unchanged): audio at the caller's rate.  Every call above takes audio at the
 * container's "sample_rate" only; these put the device resampler of wesep_hip.h ("sample rates": the sinc_interp_hann design
 * with lowpass_filter_width 6, rolloff 0.99; D = rate_in / gcd, U = rate_out / gcd, w = ceil(6 D / (0.99 min(D, U))),
 * K = 2 w + D taps per output sample) in front of and behind them.  The tap tables come from ws_resample_taps and are kept on
 * the device per (rate_in, rate_out).  All pointers are HOST pointers.  Refused by name before any launch: rates <= 0, U or D
 * above 1024, K above 4096 (the kernel's limits and its own texts).
 *
 *   ws_engine_resample(e, x, R, n, rate_in, rate_out, y, y_cap, &n_out)  x [R][n] -> y [R][*n_out], *n_out = ceil(U n / D) <=
 *     y_cap: one upload, one launch, one download; any container.  Dry run supported.
 *   ws_engine_separate_rate(e, mix, R, T, sample_rate, enroll, enroll_kind, enroll_len, enroll_rate, est)  mix and est are
 *     [R][T] at sample_rate; ALL four architectures.  (1) the mixture is resampled to the container's rate, T' = ceil(U T / D)
 *     samples; (2) a WS_ENROLL_WAVE enrollment is resampled from enroll_rate; (3) ws_engine_separate runs as it is on [R][T'];
 *     (4) the estimate is resampled back and cropped to T.  A step whose rates are equal does not run: "n_launches" is
 *     ws_engine_separate's figure plus WS_SEPARATE_RATE_LAUNCHES(mixture resampled, enrollment resampled), and with sample_rate
 *     and enroll_rate equal to the container's rate (or enroll_rate == 0: "the container's") the call IS ws_engine_separate:
 *     same launches, same bits.  The estimate is bit for bit ws_engine_resample -> ws_engine_separate -> ws_engine_resample,
 *     cropped.  Refused by name before any launch: an enroll_rate other than 0 or the container's with a kind that is not a
 *     waveform, a T' below the architecture's minimum (its own message), rates outside the kernel's limits.
 *
 * Rate stream: a causal cLN Conv-TasNet stream (ws_engine_stream_*) whose pushes carry and return samples at sample_rate.
 *   ws_engine_rate_stream_open(e, rows, enroll, enroll_kind, enroll_len, enroll_rate, max_chunk_frames, flags, sample_rate,
 *     max_push, &s)  flags is the word of ws_engine_stream_open_ex, passed through; a waveform enrollment is resampled from
 *     enroll_rate first.  Per push, all on the device: chunk H2D -> resampler A (sample_rate -> container) -> the solo
 *     stream's pending buffer and group loop -> its estimates, written behind resampler B's history -> resampler B (container ->
 *     sample_rate) -> one D2H; ONE host synchronisation.  A resampler's state is the last < K samples it took, kept in one
 *     of two buffers used in turn (the launch that computes a step's outputs also moves the new history to the other one).
 *     The four buffers and the two staging buffers (A's output, B's output) are one more slot of the stream's ONE state
 *     allocation, sized at open from max_push; "stream_state_bytes" reports the sum and no push changes it.  A push above
 *     max_push is taken in pieces.
 *   Emission.  A resampler that has taken N samples has returned U max(0, floor((N - w) / D)) (its flush: the rest up to
 *     ceil(U N / D)); the solo stream after M samples floor((M - 160) / s + 1) s.  A push returns B's emission on the solo
 *     stream's emission on A's emission; the count is known before anything runs.  ws_engine_rate_stream_flush is A's flush,
 *     the solo stream's rest and flush, then B's flush, cropped so that the total is at most the number of samples pushed:
 *     min(N, ceil(U_B ((T' - 1) s + L) / D_B)), T' the frames of ceil(U_A N / D_A) samples.  The whole output is bit for bit
 *     ws_engine_resample -> the plain stream with the same flags -> ws_engine_resample, cropped, in the separator's part to
 *     what that stream guarantees (WS_STREAM_BLOCK_KERNEL: bit for bit under any packet sizes).  Added delay: A holds back
 *     up to w_A + D_A - 1 input samples, B up to w_B + D_B - 1 of the container's, on top of the solo stream's 160 + s - 1.
 *   ws_engine_rate_stream_push_cap(s, n)  samples a row that a push of n >= 1 samples can return at most, from any state;
 *     n = 0: what the flush can return at most.
 *   Launches: a push's piece is the solo stream's groups plus WS_RATE_STREAM_PIECE_LAUNCHES = 2, one call of
 *     ws_resample_stream_fwd per resampler (a resampler that received nothing in the piece -- B before the first frame is
 *     complete -- does not run).  The copies to and from the host are not counted.
 *   With sample_rate equal to the container's rate a rate stream IS the plain stream: the calls forward to ws_engine_stream_*
 *     (same launches, same bits, its caps and refusals).  Otherwise, WS_ERR_INVALID with a message and nothing launched: a
 *     container that cannot stream, an unknown flag bit (the texts of ws_engine_stream_open_ex), rows < 1, max_push outside
 *     [1, 2^24], an enroll_rate with a kind that is not a waveform, est_cap below what the call emits, a flush before L samples
 *     at the container's rate, push or flush after a flush, n < 1, a NULL pointer.
 * The stream pool is NOT rate-aware: its pending samples live on the host, and per-slot rates need rows forms of the
 * resampler (per-row geometry, position and history slot): that pool is the rate pool below. */
#define WS_SEPARATE_RATE_LAUNCHES(mix_resampled, enroll_resampled) (2 * ((mix_resampled) != 0) + ((enroll_resampled) != 0))
#define WS_RATE_STREAM_PIECE_LAUNCHES 2
typedef struct ws_rate_stream ws_rate_stream;
int ws_engine_resample(ws_engine* e, const float* x, int R, int n, int rate_in, int rate_out, float* y, int y_cap, int* n_out);
int ws_engine_separate_rate(ws_engine* e, const float* mix, int R, int T, int sample_rate, const void* enroll, int enroll_kind,
                            int enroll_len, int enroll_rate, float* est);
int ws_engine_rate_stream_open(ws_engine* e, int rows, const void* enroll, int enroll_kind, int enroll_len, int enroll_rate,
                               int max_chunk_frames, unsigned flags, int sample_rate, int max_push, ws_rate_stream** out);
int ws_engine_rate_stream_push(ws_rate_stream* s, const float* chunk, int n, float* est, int est_cap, int* n_out);
int ws_engine_rate_stream_flush(ws_rate_stream* s, float* est, int est_cap, int* n_out);
int ws_engine_rate_stream_reset(ws_rate_stream* s);
void ws_engine_rate_stream_close(ws_rate_stream* s);
int ws_engine_rate_stream_push_cap(const ws_rate_stream* s, int n);

/* Rate pool (new symbols, engine ABI 2 unchanged): the stream pool with a sample rate per slot -- calls at 8, 16 and 48 kHz in
 * one push.  A slot is a rate stream of one row; one round carries one packet for any set of slots at any mix of rates, and the
 * number of entry-point calls does not depend on how many slots or how many distinct rates the round holds.
 *   ws_engine_rate_pool_open(e, slots, max_chunk_frames, flags, rates, n_rates, max_push, &pool)  rates [n_rates]: the sample
 *     rates the pool will accept; the container's own is always accepted.  Every listed rate is validated in both directions
 *     with the kernel's limits, by name, and every tap table is made and uploaded here.  max_push in [1, 2^24]: caller-rate
 *     samples per slot per piece.  The state -- the pool's, two pending buffers and resampler B's two buffers per slot, the
 *     output block, the tables -- is ONE device allocation sized from max_push and the worst listed geometry; it never grows
 *     (ws_engine_info "stream_state_bytes", constant over attach, push, flush and detach).  flags: the word of
 *     ws_engine_pool_open_ex.
 *   ws_engine_rate_pool_attach(pool, enroll, enroll_kind, enroll_len, enroll_rate, sample_rate, &slot)  as ws_engine_pool_attach;
 *     sample_rate must be one of the accepted rates (refused by name, the message lists them); a waveform enrollment at
 *     enroll_rate != 0 is resampled first, as ws_engine_rate_stream_open does.
 *   ws_engine_rate_pool_push(pool, n_active, slots, chunks, n, est, est_cap, n_out)  as ws_engine_pool_push with chunks and
 *     estimates at each slot's own rate.  Entry i emits B's emission on the pool's emission on A's emission (known before
 *     anything runs; est_cap[i] is checked before any launch; ws_engine_rate_pool_push_cap(pool, slot, n) always suffices).
 *     A packet above max_push is taken in pieces, piece j of every slot that has one in round j: each slot sees the inner
 *     pushes of a solo rate stream opened with the same max_push.  Per piece, all on the device: resampler A over all slots
 *     (its history is caller samples and stays on the host; one staging block and the table are uploaded) -> the pool's
 *     groups, each gathered from the slots' pending samples and scattered behind the slots' B histories by ws_rows_copy_fwd
 *     -> one compaction copy of the pending samples -> resampler B over all slots -> one device-to-host copy of B's compact
 *     block.  ONE host synchronisation per push.  A group is WS_RATE_POOL_GROUP_LAUNCHES(R, X) = WS_POOL_GROUP_LAUNCHES + 2
 *     entry-point calls, a piece adds WS_RATE_POOL_PIECE_LAUNCHES = 3 (A, compaction, B; a step that has nothing to do in a
 *     piece -- no frame complete yet -- does not run); with WS_STREAM_BLOCK_KERNEL the _BLOCK_ forms.
 *   ws_engine_rate_pool_flush(pool, slot, est, est_cap, &n_out)  the end of ONE slot's stream: A's flush, the remaining frames,
 *     the inner flush group and the overlap-add carry, B's steps, B's flush; the total is cropped to the samples pushed.
 *   ws_engine_rate_pool_detach / _close  as the pool's.
 * A slot at the container's rate runs the identity table (U = D = K = 1, the tap 1.0) through both resamplers: no delay, no
 * filter; its samples are the plain pool's.  WS_ERR_INVALID with a message and nothing launched: the refusals of
 * ws_engine_pool_* and ws_engine_rate_stream_* under this family's names (a container that cannot stream, an unknown flag
 * bit, an enroll_rate with a kind that is not a waveform, a slot that is free, flushed or named twice, est_cap below the
 * emission, a flush before L samples at the container's rate, a slot of a call that failed half way), slots outside
 * [1, 65535], a rate outside the kernel's limits, an attach at a rate that was not listed. */
#define WS_RATE_POOL_GROUP_LAUNCHES(R, X) (WS_POOL_GROUP_LAUNCHES(R, X) + 2)
#define WS_RATE_POOL_BLOCK_GROUP_LAUNCHES(R, X) (WS_POOL_BLOCK_GROUP_LAUNCHES(R, X) + 2)
#define WS_RATE_POOL_PIECE_LAUNCHES 3
#define WS_RATE_POOL_BLOCK_PIECE_LAUNCHES 3
typedef struct ws_rate_pool ws_rate_pool;
int ws_engine_rate_pool_open(ws_engine* e, int slots, int max_chunk_frames, unsigned flags, const int* rates, int n_rates,
                             int max_push, ws_rate_pool** out);
int ws_engine_rate_pool_attach(ws_rate_pool* p, const void* enroll, int enroll_kind, int enroll_len, int enroll_rate,
                               int sample_rate, int* slot);
int ws_engine_rate_pool_push(ws_rate_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n,
                             float* const* est, const int* est_cap, int* n_out);
int ws_engine_rate_pool_push_cap(const ws_rate_pool* p, int slot, int n);
int ws_engine_rate_pool_flush(ws_rate_pool* p, int slot, float* est, int est_cap, int* n_out);
int ws_engine_rate_pool_detach(ws_rate_pool* p, int slot);
void ws_engine_rate_pool_close(ws_rate_pool* p);

/* ---- live windows (runtime/live.cc; DESIGN sections 7 and 11b) -- new symbols, WS_ENGINE_ABI_VERSION 2 unchanged ----------
 * ws_engine_separate_long for audio that arrives: ANY container (pBSRNN, Conv-TasNet, DPCCN, TF-GridNet; nothing here needs a
 * causal model), one mixture, K target speakers, pushes of any size.  S = window, O = overlap, H = S - O, N = samples pushed.
 *   windows run      Wr(N) = N < S ? 0 : 1 + (N - S) / H: window w starts at w H and runs once w H + S samples exist
 *   samples emitted  E(N) = max(Wr - 1, 0) H: the samples before the start of the newest window run.  Every later window,
 *                    regular or end-aligned, starts behind it, so every window covering an emitted sample has run, with its
 *                    tail ramp.  LATENCY: a sample comes out S .. S + H samples after it went in -- the price of not knowing
 *                    where the recording ends (the end-aligned last window may reach back to the newest window's start)
 *   flush            n = N is final: if (n - S) % H != 0 one more window runs at n - S (no tail ramp); n < S is the one short
 *                    row of ws_engine_separate_long's W == 1 branch, with the architecture's own lower bound on T -- a refusal
 *                    launches nothing and leaves the state as it was, so a later push goes on.  Then [E, n) comes out.
 * open makes exactly the checks of ws_engine_separate_long (its messages), runs the speaker stage ONCE over the K enrollments
 * (or copies fixed embeddings / WS_ENROLL_SPEAKER) and makes ONE device allocation, ws_engine_info "live_state_bytes", a
 * function of (K, S, O, max_rows): a ring [K][cap][S] of window estimates, cap = g_max + 3, g_max = max(1, max_rows / K); the
 * ring of TF-GridNet's per-window factors; a group's samples, rows and embeddings.  Pending samples (fewer than S + H between
 * pushes) stay on the host.  K > max_rows: a window's K rows go in several forwards, as in ws_engine_separate_long.
 * push: est [K][est_cap], *n_out samples a target.  If no window became complete: *n_out = 0, NO launch, NO synchronisation.
 * Otherwise per group of at most g_max new windows (cut where the ring wraps): one upload of its span, ws_window_rows, the
 * rectangular plan on its rows in forwards of at most max_rows rows, the estimates into the ring, ws_xfade_stream_fwd on what
 * became final; then one device-to-host copy and one synchronisation.  ws_engine_info "n_launches" after a push or flush:
 *     sum over its groups of (the forwards' rectangular counts + WS_LIVE_GROUP_LAUNCHES(K, max_rows)) + 1
 * -- per group ws_window_rows, the copy into the ring where a forward's rows span several targets (K > 1 and max_rows > 1;
 * otherwise the plan writes into the ring itself) and ws_xfade_stream_fwd; + 1: the copy to the host.  A flush runs at most
 * one group.  Nothing of it depends on N.  "live_windows": windows run since open / reset; "live_groups": groups of the last
 * push or flush.  The engine's work arena is used under a scope and never reset; other calls on the engine between two
 * pushes do not disturb the handle.  A push or flush after a flush is refused until ws_engine_live_reset (back to sample 0,
 * enrollments kept).  Dry-run engines take every call.
 * PARITY: the concatenated output equals ws_engine_separate_long(mix, n, K, ..., window, overlap, max_rows)
 *   - to the rounding of forwards over other row counts (groups form differently);
 *   - bit for bit when both run one row per forward (max_rows = 1), whatever the packet sizes;
 *   - a flush alone with n <= window, K <= max_rows is ws_engine_separate on [K][n], bit for bit. */
typedef struct ws_live ws_live;
#define WS_LIVE_PUSH_CAP(n, H) (((n) / (H) + 1) * (H))
#define WS_LIVE_FLUSH_CAP(S, O) (2 * (S) - (O))
#define WS_LIVE_GROUP_LAUNCHES(K, max_rows) (2 + ((K) > 1 && (max_rows) > 1))
int ws_engine_live_open(ws_engine* e, int K, const void* enroll, int enroll_kind, int enroll_len, const int* enroll_lengths,
                        int window, int overlap, int max_rows, ws_live** out);
int ws_engine_live_push(ws_live* s, const float* chunk, int n, float* est, int est_cap, int* n_out);
int ws_engine_live_flush(ws_live* s, float* est, int est_cap, int* n_out);
int ws_engine_live_reset(ws_live* s);
void ws_engine_live_close(ws_live* s);

/* ---- live pool (runtime/live_pool.cc; DESIGN sections 7 "Live pool" and 11b) -- new symbols, WS_ENGINE_ABI_VERSION 2 unchanged
 * MANY independent live recordings on one engine: each slot is a ws_live's bookkeeping -- its own position, its own packet
 * sizes, its own K enrollments -- and every window that one push completes, in whatever slot, goes through the separator in
 * the same forwards.  N solo handles run N half-empty forwards one after another, each with its own upload, synchronisation
 * and download; the pool runs one chain.  S = window, O = overlap, H = S - O, g_max = max(1, max_rows / K), cap = g_max + 3.
 *   ws_engine_live_pool_open(e, slots, K, window, overlap, max_rows, &pool)  the window checks of ws_engine_separate_long (its
 *     messages) and the plan's guards on a forward of max_rows rows; slots in [1, 65535], slots K g_max + slots <= 65535 (the
 *     tables of a launch).  Makes ONE device allocation, ws_engine_info "live_pool_state_bytes", a function of (slots, K, S,
 *     O, max_rows) only, that no attach, push, flush or detach grows.  Per slot: the ring [K][cap][S] of window estimates, the
 *     ring [cap] of TF-GridNet's per-window factors, the K embeddings.  Per round: the staging block (the slots' spans of
 *     (g - 1) H + S samples, the factors, the embedding rows, the three tables), the rows rectangle and the estimates
 *     rectangle, slots K g_max rows of S samples each.  Pending samples (fewer than S + H a slot between pushes) stay on the host.
 *   ws_engine_live_pool_attach(pool, enroll, enroll_kind, enroll_len, enroll_lengths, &slot)  takes the lowest free slot, checks
 *     the K enrollments as ws_engine_separate_long does (every kind ws_engine_live_open takes, WS_ENROLL_SPEAKER included),
 *     runs the speaker stage ONCE for them and puts the slot at sample 0.  A full pool is refused by name.
 *   ws_engine_live_pool_push(pool, n_active, slots, chunks, n, est, est_cap, n_out)  one packet for each of n_active DISTINCT
 *     attached slots: chunks[i] is n[i] >= 1 samples for slots[i]; est[i] is [K][est_cap[i]], n_out[i] samples a target -- per
 *     slot the emission rule of ws_engine_live_push (WS_LIVE_PUSH_CAP(n[i], H) always suffices).  All packets are appended
 *     first.  If no slot completed a window: every n_out[i] = 0, NO launch, NO synchronisation.  Otherwise the work runs in
 *     ROUNDS: in ascending slot order every slot that still owes windows gives min(owed, g_max, cap - Wr % cap) consecutive
 *     windows (the solo handle's cut).  A round's rows are ordered (slot, target, window); per round ONE upload of the staging
 *     block, ONE ws_window_slots_fwd for all of its rows, the architecture's rectangular plan in forwards of at most max_rows
 *     rows whichever slots they came from, ONE ws_rows_copy_fwd of the estimates (and TF-GridNet's factors, computed on the
 *     host) into the rings, ONE ws_xfade_stream_rows_fwd for everything the round made final.  After the last round one copy
 *     to the host and ONE synchronisation.  ws_engine_info "n_launches" after a push:
 *         sum over its rounds of (the forwards' rectangular counts + WS_LIVE_POOL_ROUND_LAUNCHES) + 1
 *     -- it depends on the number of participating slots only through the forwards' own counts.  "live_pool_rounds" and
 *     "live_pool_forwards" report the last push or flush.
 *   ws_engine_live_pool_flush(pool, slot, est, est_cap, &n_out)  the end of ONE slot's recording by the rule of
 *     ws_engine_live_flush: the short window n < S (the architecture's lower bound on T is checked before anything runs; a
 *     refusal leaves the slot as it was) or the end-aligned last window, as a round of this one slot whose cross-fade is the
 *     final one; WS_LIVE_FLUSH_CAP(S, O) always suffices.  A flush that has no window to run is the cross-fade and the copy:
 *     2 entry-point calls.  The slot then takes nothing until it is detached.
 *   ws_engine_live_pool_detach(pool, slot)  frees the slot for the next attach.    ws_engine_live_pool_close(pool)  before
 *     ws_engine_destroy.
 * STORE, RUN, DUE -- the windows run on the CALLER's clock.  A push runs what it completes at once, so recordings that did not
 * start together never share a forward.  Every slot completes exactly one window per H samples: a caller that holds complete
 * windows back for up to H samples lets every slot in flight ride in the same forwards however the calls are staggered.
 * LATENCY: a sample then comes out S .. S + H samples after it went in, plus whatever the caller holds.
 *   ws_engine_live_pool_store(pool, n_active, slots, chunks, n)  push's packets (its argument checks, under this name) appended
 *     to the slots' pending samples on the host: NO launch, NO synchronisation, "n_launches" 0 after it.  The backlog is
 *     bounded: a store that would leave a slot with WS_LIVE_POOL_STORE_LIMIT(S, H) = 2 S + H or more pending samples is refused
 *     ("run first") before anything of the call is appended.
 *   ws_engine_live_pool_run(pool, n_active, slots, final, est, est_cap, n_out)  for every named slot ALL windows that are complete
 *     and not yet run, through the rounds of a push: ascending slot order, the solo cut per slot and round, one upload, one
 *     ws_window_slots_fwd, forwards of at most max_rows rows whichever slots they came from, one ws_rows_copy_fwd and one
 *     ws_xfade_stream_rows_fwd per round, one download and one synchronisation per call; the emission rule of a push.  final
 *     may be NULL; final[i] != 0 ends slot i's recording by the rule of ws_engine_live_pool_flush once its regular windows have
 *     run: with n >= S the end-aligned last window is a row of S samples like any other and shares the round's forwards with
 *     the other slots' windows (in the round after the slot's last regular one, if the call ran any); a short recording
 *     (n < S) gets forwards of its own rows in that round, behind the rows of S samples (the rectangular plans take one length
 *     a forward), its lower bound on T checked before anything runs.  The slot then takes nothing until it is detached.  No
 *     named slot has work: every n_out[i] = 0, NO launch, NO synchronisation.  WS_LIVE_POOL_RUN_CAP(S, H) = 2 S + H always
 *     suffices as est_cap; est_cap is checked for every entry before any launch.  "n_launches", "live_pool_rounds" and
 *     "live_pool_forwards" report the last run by the formula of a push.
 *   ws_engine_live_pool_due(pool, &rows_ready, &oldest_age)  a query for a scheduler, no launch, no change of state: rows_ready
 *     = K x the complete windows not yet run over all slots a run would take; oldest_age = the largest number of samples a slot
 *     has received since its oldest such window w became complete, N - (w H + S), 0 if none is ready.  Either pointer may be NULL.
 *   push and flush on a slot with stored audio are store + run and run(final) of their slots: one code path serves all.
 * The engine's work arena is used under a scope and nothing of it is held between two calls: other calls on the engine between
 * two pushes do not disturb the pool.  Dry-run engines take every call.  All pointers are HOST pointers; callers serialise.
 * FAILURE: the slots named by a push, run or flush that failed half way are refused by name until they are detached; the other
 * slots go on.
 * PARITY, per slot: the concatenation of what its pushes and its flush return equals ws_engine_separate_long on that slot's
 * concatenated audio -- whatever the packet sizes were, whenever the slot was attached, whatever the other slots were doing
 *   - bit for bit with max_rows = 1: every forward then holds one row, so these are also the solo live handle's bits;
 *   - otherwise to the rounding of forwards over other row counts (which rows share a forward depends on the other slots).
 * No launch mixes rows: with the row composition of the forwards held fixed, a slot's bits do not depend on the other slots'
 * sample values, NaN and inf included -- as far as the architecture's rectangular plan keeps its rows apart.
 * NOT built: a sample rate per slot; a different K per slot; a clock inside the pool (the caller's due + run is the policy).
 * WS_ERR_INVALID with a message and nothing launched: every refusal of ws_engine_live_* under this family's names; slots
 * outside [1, 65535]; a full pool; a slot of a push, store, run or flush that is free, flushed, named twice or part of a failed
 * call; n[i] < 1; est_cap below the emission, checked for every entry before any launch; a store past its limit; a final entry
 * of a run whose slot was never fed; a NULL pointer. */
typedef struct ws_live_pool ws_live_pool;
#define WS_LIVE_POOL_ROUND_LAUNCHES 3
#define WS_LIVE_POOL_STORE_LIMIT(S, H) (2 * (S) + (H))   /* pending samples a slot: a store must stay below */
#define WS_LIVE_POOL_RUN_CAP(S, H) (2 * (S) + (H))       /* est_cap that always suffices for a run, per target */
int ws_engine_live_pool_open(ws_engine* e, int slots, int K, int window, int overlap, int max_rows, ws_live_pool** out);
int ws_engine_live_pool_attach(ws_live_pool* p, const void* enroll, int enroll_kind, int enroll_len, const int* enroll_lengths,
                               int* slot);
int ws_engine_live_pool_push(ws_live_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n,
                             float* const* est, const int* est_cap, int* n_out);
int ws_engine_live_pool_flush(ws_live_pool* p, int slot, float* est, int est_cap, int* n_out);
int ws_engine_live_pool_store(ws_live_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n);
int ws_engine_live_pool_run(ws_live_pool* p, int n_active, const int* slots, const int* final, float* const* est, const int* est_cap,
                            int* n_out);
int ws_engine_live_pool_due(ws_live_pool* p, long long* rows_ready, long long* oldest_age);
int ws_engine_live_pool_detach(ws_live_pool* p, int slot);
void ws_engine_live_pool_close(ws_live_pool* p);

/* ---- tail pool (runtime/tail_pool.cc; DESIGN sections 7 "Tail pool" and 11b) -- new symbols, WS_ENGINE_ABI_VERSION 2 unchanged
 * LOW-LATENCY live separation on TRAILING windows, any container, many recordings.  The live families above emit a sample once
 * every window of ws_engine_separate_long that covers it has run: S .. S + H samples late, and a live pool's slots complete
 * windows together only when their recordings are aligned.  Here the clock is the caller's: a TICK runs, for every named slot
 * with enough new audio, the window of its NEWEST S samples and emits the newest part of it.  Latency: the tick period plus the
 * fade.  Every slot with new audio fires on the same tick, so the forwards fill up however the calls are staggered.  PRICE: one
 * full window a slot a tick, the caller's to choose through the tick period.  The output is a rule of its own, NOT
 * ws_engine_separate_long, and nothing is claimed about separation quality: the backward direction of a BLSTM sees no future at
 * a window's end; callers trade that through S, the tick period and the fade.
 * THE RULE, per slot.  Fixed at open: window S, fade C in [0, S / 2], warm in [max(C, 1, the architecture's lower bound on T), S],
 * K targets.  N: samples pushed.  F: N at the last firing.  hold [K][C]: the last window's estimate of the newest C samples, kept
 * back.  E: samples emitted, 0 before the first firing and F - C after it.
 *   push   appends to the slot's pending samples on the host: NO launch, NO synchronisation.  A push that would make N - E > S is
 *          refused ("tick first") before anything of the call is appended: what has not come out must fit one window.
 *   tick   a named slot FIRES if N >= warm and it never fired or N - F >= max(C, 1); one that does not gets n_out = 0.  A firing
 *          slot runs the window [a, N), a = max(0, N - S), L = N - a, one row per target, and emits [E, N - C): m = N - C - E
 *          samples.  With h = C after a first firing, else 0, the first h of them are the held ones cross-faded into the new
 *          window's estimate of the same positions, the rest come from the new window alone; the window's last C samples become
 *          the new hold; then F = N.
 *   flush  ends one recording.  N > F, or never fired: one last window [max(0, N - S), N) emits [E, N), no new hold; its L only
 *          has to meet the architecture's own lower bound on T -- a refusal launches nothing and leaves the slot as it was.
 *          N == F: the hold comes out as it is, a copy with no forward.  The slot then takes nothing until it is detached.
 *   blend  with y the window's estimate: v = fl(y scale), scale the window's standard deviation for TF-GridNet (computed on the
 *          host over the window's own L samples, 1 / std folded into the gather) and exactly 1 otherwise; for j < h
 *          out = fma(ramp[j], fl(v - hold[j]), hold[j]), ramp[j] = float(j + 1) / float(C + 1); for j >= h out = v; the new hold
 *          stores v.  hold is double-buffered per slot and target and flipped at every firing.
 *   ws_engine_tail_pool_open(e, slots, K, window, fade, warm, max_rows, &pool)  the window checks of ws_engine_separate_long (its
 *     messages), the plan's guards on a forward of max_rows rows of S samples, the bounds on fade and warm above; slots in
 *     [1, 65535], slots K <= 65535 (the tables of a launch).  Makes ONE device allocation, ws_engine_info
 *     "tail_pool_state_bytes", a function of (slots, K, S, C, max_rows) only, that no later call grows: per slot the two hold
 *     buffers [2][K][C] and the K embeddings; per tick the staging block (the slots' spans of at most S samples, the embedding
 *     rows, the two tables), the rows, estimates and output rectangles, slots K rows of pitch S each; the ramp.  Pending samples
 *     (at most S a slot) stay on the host.
 *   ws_engine_tail_pool_attach(pool, enroll, enroll_kind, enroll_len, enroll_lengths, &slot)  takes the lowest free slot, runs the
 *     speaker stage ONCE for its K enrollments (every kind ws_engine_live_pool_attach takes, WS_ENROLL_SPEAKER included) and
 *     puts the slot at sample 0.  A full pool is refused by name.
 *   ws_engine_tail_pool_push(pool, n_active, slots, chunks, n)  chunks[i] is n[i] >= 1 samples for slots[i], DISTINCT slots.
 *   ws_engine_tail_pool_tick(pool, n_active, slots, est, est_cap, n_out)  est[i] is [K][est_cap[i]], n_out[i] samples a target
 *     (WS_TAIL_CAP(S) always suffices).  If no named slot fires: NO launch, NO synchronisation.  Otherwise, in order: one upload
 *     of the staging block, ONE ws_window_slots_fwd for all rows, the forwards, ONE ws_tail_emit_rows_fwd, one copy to the
 *     host, ONE synchronisation.  Forwards: the rows of full windows (L = S), ordered (slot, target), in forwards of at most
 *     max_rows rows whichever slots they came from; the rows of a slot still in warm-up (L < S) in forwards of that slot's own
 *     rows (the rectangular plans take one length a forward).  ws_engine_info "n_launches" after a tick:
 *         the forwards' rectangular counts + WS_TAIL_TICK_LAUNCHES + 1
 *     "tail_pool_forwards" and "tail_pool_rows" report the last tick or flush.
 *   ws_engine_tail_pool_flush(pool, slot, est, est_cap, &n_out)  a tick of this one slot with the final rule; with N == F it is
 *     ws_rows_copy_fwd of the hold and the copy to the host: 2 entry-point calls (nothing at all when the fade is 0).
 *   ws_engine_tail_pool_detach(pool, slot)  frees the slot.    ws_engine_tail_pool_close(pool)  before ws_engine_destroy.
 * The engine's work arena is used under a scope and nothing of it is held between two calls.  Dry-run engines take every call.
 * All pointers are HOST pointers; callers serialise.
 * FAILURE: the slots named by a tick or flush that failed half way are refused by name until they are detached; the other
 * slots go on.
 * No launch mixes rows: with the row composition of the forwards held fixed, a slot's bits do not depend on the other slots'
 * sample values -- as far as the architecture's rectangular plan keeps its rows apart.  With one row per forward
 * (max_rows = 1) every window is bit for bit ws_engine_separate on that window alone.
 * A sample rate per slot: the rate tail pool below (ws_engine_rate_tail_pool_*).
 * NOT built: a different K per slot; backlog handling beyond one window (a caller that falls behind has to tick, or drop audio
 * itself).
 * WS_ERR_INVALID with a message and nothing launched: a slot of a push, tick or flush that is free, flushed, named twice or
 * part of a failed call; n[i] < 1; est_cap below the emission, checked for every entry before any launch; a NULL pointer; the
 * push overflow above; a full pool; the bounds of open. */
typedef struct ws_tail_pool ws_tail_pool;
#define WS_TAIL_TICK_LAUNCHES 2          /* ws_window_slots_fwd + ws_tail_emit_rows_fwd */
#define WS_TAIL_CAP(S) (S)               /* est_cap that always suffices, per target */
int ws_engine_tail_pool_open(ws_engine* e, int slots, int K, int window, int fade, int warm, int max_rows, ws_tail_pool** out);
int ws_engine_tail_pool_attach(ws_tail_pool* p, const void* enroll, int enroll_kind, int enroll_len, const int* enroll_lengths,
                               int* slot);
int ws_engine_tail_pool_push(ws_tail_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n);
int ws_engine_tail_pool_tick(ws_tail_pool* p, int n_active, const int* slots, float* const* est, const int* est_cap, int* n_out);
int ws_engine_tail_pool_flush(ws_tail_pool* p, int slot, float* est, int est_cap, int* n_out);
int ws_engine_tail_pool_detach(ws_tail_pool* p, int slot);
void ws_engine_tail_pool_close(ws_tail_pool* p);

/* ---- rate tail pool (runtime/rate_tail_pool.cc; DESIGN sections 7 "Rate tail pool" and 11b) -- new symbols,
 * WS_ENGINE_ABI_VERSION 2 unchanged.  The tail pool above with a SAMPLE RATE PER SLOT: a telephony call at 8 kHz and a WebRTC
 * call at 48 kHz get the low-latency path to pBSRNN, DPCCN and (non-causal) Conv-TasNet containers in the same ticks.  A slot
 * carries and returns audio at its caller's rate r; the separator runs at the container's rate r0.
 * THE RULE, per slot.  A is the r -> r0 filter (U_A, D_A, w_A, K_A), B the r0 -> r filter (ws_resample_geom).  Window S, fade C and
 * warm are samples at the CONTAINER's rate, exactly as in the tail pool.  N_c: caller-rate samples pushed.
 *   N      the container-rate samples the recording HAS: the streaming emission count of wesep_hip.h,
 *          U_A max(0, floor((N_c - w_A) / D_A)), known on the host before anything runs.
 *   push   appends caller-rate samples on the host: NO launch, NO synchronisation.  Refused ("tick first") when
 *          ceil(U_A (N_c + n) / D_A) - E > S, before anything of the call is appended: what a flush right after the push would
 *          have to emit must fit one window.
 *   tick   the tail pool's rule on N, unchanged: firing condition, window [max(0, N - S), N), emission [E, N - C), hold, blend,
 *          ramp, F.  The window's samples are kept NOWHERE at the container's rate: the gather (ws_window_resample_rows_fwd)
 *          computes them from the caller-rate span that their taps cover, so the pool carries no input-resampler state and a
 *          window's bits are those of ws_resample_fwd on the whole recording.  The emitted samples of every (slot, target) are
 *          a stream: they go through B as a streaming resampler whose history is held per slot and target in the pool's state,
 *          double-buffered.  The tick returns B's emission, at the caller's rate; n_out[i] is known before anything runs.
 *   flush  N becomes ceil(U_A N_c / D_A); the last window runs with A's final rule (taps behind the end are skipped); the tail
 *          flush rule emits [E, N); B takes them and ends its stream in the same launch (final = 1 on `history | new`: the bits
 *          of B's step followed by B's flush).  The total is cropped so that a slot returns exactly N_c samples a target over
 *          its life (B's uncropped total is never below N_c).
 *   a slot at the container's rate runs the identity table (U = D = K = 1, tap 1.0) through both filters: its samples are the
 *          plain tail pool's.
 * PARITY, per slot: bit for bit what the existing public pieces give when chained -- a streaming resampler r -> r0 fed the same
 * packets; a tail pool at the container's rate fed its emissions and ticked at the same moments (its flush after the
 * resampler's); one streaming resampler r0 -> r per target fed the pool's emissions and flushed, cropped to N_c -- with
 * max_rows = 1, and whenever the two pools form the same forwards (the same slots attached in the same order and firing on the
 * same ticks).
 *   ws_engine_rate_tail_pool_open(e, slots, K, window, fade, warm, max_rows, rates, n_rates, &pool)  the checks of
 *     ws_engine_tail_pool_open under this name; every listed rate validated in both directions and every tap table uploaded, as
 *     ws_engine_rate_pool_open does (the container's own rate is always accepted).  A TF-GridNet container is refused by name:
 *     its per-window standard deviation is taken on the host from container-rate samples, which this pool never has there.
 *     Makes ONE device allocation, ws_engine_info "rate_tail_pool_state_bytes", that no later call grows, a function of
 *     (slots, K, S, C, max_rows) and the worst listed geometry only: the tail pool's parts (the spans at the caller's rate, the
 *     three tables), B's two buffers [K_B - 1 + S] per slot and target, B's compact output block, the ramp, the tables.
 *   ws_engine_rate_tail_pool_attach(pool, enroll, enroll_kind, enroll_len, enroll_lengths, enroll_rate, sample_rate, &slot)  as
 *     ws_engine_tail_pool_attach; sample_rate must be a listed rate (the message lists the accepted ones); a WS_ENROLL_WAVE
 *     enrollment at enroll_rate != 0 is resampled first, every row over its own length (other kinds: enroll_rate 0).
 *     A rate whose slots could never fire is refused: before the first firing a push is taken while ceil(U_A N_c / D_A) <= S, and
 *     the filter's look-ahead keeps N below that; warm must not exceed U_A floor((floor(D_A S / U_A) - w_A) / D_A).
 *   ws_engine_rate_tail_pool_push(pool, n_active, slots, chunks, n)  chunks[i]: n[i] >= 1 samples at slots[i]'s rate.
 *     ws_engine_rate_tail_pool_room(pool, slot): the largest n the slot takes now (0: tick first; -1: not an attached, unflushed
 *     slot) -- what a caller cuts a packet to.
 *   ws_engine_rate_tail_pool_tick(pool, n_active, slots, est, est_cap, n_out)  est[i] is [K][est_cap[i]], n_out[i] samples a
 *     target at the slot's rate; ws_engine_rate_tail_pool_cap(pool, slot) always suffices; est_cap is checked for every entry
 *     before any launch.  If no named slot fires: NO launch, NO synchronisation.  Otherwise, in order: one upload of the staging
 *     block (spans, embedding rows, tables), ONE ws_window_resample_rows_fwd, the forwards grouped exactly as the tail pool
 *     groups them, ONE ws_tail_emit_rows_fwd writing straight behind B's histories, ONE ws_resample_stream_rows_fwd for B over
 *     all (slot, target) rows, one copy to the host, ONE synchronisation.  ws_engine_info "n_launches" after a tick:
 *         the forwards' rectangular counts + WS_RATE_TAIL_TICK_LAUNCHES + 1
 *     whatever the number of firing slots and of distinct rates among them (one less in the one case that nothing reaches B: only
 *     first firings with warm == fade).  "rate_tail_pool_forwards" and "rate_tail_pool_rows" report the last tick or flush.
 *   ws_engine_rate_tail_pool_flush(pool, slot, est, est_cap, &n_out)  a tick of this one slot with the final rule: the same
 *     count.  Only a slot at the container's rate can have N == F: ws_rows_copy_fwd of the hold behind B's history in place of
 *     the gather, the forwards and the emission (nothing at all when the fade is 0).
 *   ws_engine_rate_tail_pool_detach(pool, slot)    ws_engine_rate_tail_pool_close(pool)  before ws_engine_destroy.
 * Dry-run engines take every call and return the right counts.  All pointers are HOST pointers; callers serialise.
 * FAILURE: the slots named by a tick or flush that failed half way are refused by name until they are detached.
 * No launch mixes rows: with the row composition of the forwards held fixed, a slot's bits do not depend on the other slots'
 * sample values, NaN and inf included.
 * NOT built: TF-GridNet containers; a different K per slot; backlog handling beyond one window.
 * WS_ERR_INVALID with a message and nothing launched: the refusals of ws_engine_tail_pool_* and ws_engine_rate_pool_* under this
 * family's names; an unlisted rate; the push overflow above. */
typedef struct ws_rate_tail_pool ws_rate_tail_pool;
#define WS_RATE_TAIL_TICK_LAUNCHES 3     /* ws_window_resample_rows_fwd + ws_tail_emit_rows_fwd + ws_resample_stream_rows_fwd */
int ws_engine_rate_tail_pool_open(ws_engine* e, int slots, int K, int window, int fade, int warm, int max_rows, const int* rates,
                                  int n_rates, ws_rate_tail_pool** out);
int ws_engine_rate_tail_pool_attach(ws_rate_tail_pool* p, const void* enroll, int enroll_kind, int enroll_len, const int* enroll_lengths,
                                    int enroll_rate, int sample_rate, int* slot);
int ws_engine_rate_tail_pool_cap(const ws_rate_tail_pool* p, int slot);
int ws_engine_rate_tail_pool_room(const ws_rate_tail_pool* p, int slot);
int ws_engine_rate_tail_pool_push(ws_rate_tail_pool* p, int n_active, const int* slots, const float* const* chunks, const int* n);
int ws_engine_rate_tail_pool_tick(ws_rate_tail_pool* p, int n_active, const int* slots, float* const* est, const int* est_cap, int* n_out);
int ws_engine_rate_tail_pool_flush(ws_rate_tail_pool* p, int slot, float* est, int est_cap, int* n_out);
int ws_engine_rate_tail_pool_detach(ws_rate_tail_pool* p, int slot);
void ws_engine_rate_tail_pool_close(ws_rate_tail_pool* p);

/* The reference runtime's call: one mixture, two enrollment utterances (int16 PCM), two estimates.
 * mix [n] int16; spk1 / spk2 [n_enroll] int16; out [2][n] float in [-1, 1] like the reference (it scales the mixture by
 * 2^-15 before the model, separate_engine.cc:81-84, and its wav writer scales back, frontend/wav.h:245-253).
 * Replaces SeparateEngine::ForwardFunc (separate_engine.cc:76-123). */
int ws_engine_forward_pcm16(ws_engine* e, const int16_t* mix, int n, const int16_t* spk1, const int16_t* spk2,
                            int n_enroll, float* out);

#ifdef __cplusplus
}
#endif
#endif /* WESEP_ENGINE_H_ */
