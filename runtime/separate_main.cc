// separate_main -- command-line front end of the native runtime, with the interface of the reference's
// runtime/bin/separate_main.cc:24-115:
//
//   separate_main --wav_scp scp --model model.wsw --output_dir out [--sample_rate 16000] [--devices 0,1] [--jobs 4]
//                 [--batch 8] [--sort_by_length] [--chunk_seconds 4 [--overlap_seconds 1] [--chunk_rows 8]] [--dry_run]
//                 [--stream_ms 10 [--stream_pool 4 | --rate_pool 4] [--stream_block]] [--resample]
//                 [--live_ms 100 --chunk_seconds 4 [--live_pool 4 [--live_hold_ms 3000]]]
//                 [--tail_ms 100 --chunk_seconds 4 [--tail_fade_ms 10] [--tail_warm_seconds 4] [--tail_pool 4]]
//                 [--tail_ms 40 --chunk_seconds 4 --tail_rate_pool 4 [--tail_fade_ms 10] [--tail_warm_seconds 3]]
//   separate_main --wav_path mix.wav --spk1_emb e1.wav --spk2_emb e2.wav --model model.wsw --output_dir out
//
// wav_scp lines: "<key> <mixture.wav> <enroll_spk1.wav> <enroll_spk2.wav>".  For every line the mixture and the two
// enrollment utterances go through ws_engine_forward_pcm16 (enrollments cut to the shorter one, as the reference does)
// and <key>-spk1.wav / <key>-spk2.wav are written; the real-time factor is printed per utterance and in total.
// Utterances are independent: --jobs J worker threads, each with its own engine (own HIP stream, arena and weight
// copy -- 0.3 GB of 288), spread round-robin over --devices.  Engines that share a GPU overlap on the device (round 2
// serialised them; round 3 removed the cause -- profiles/r03_kernel_race.md -- and WS_ENGINE_SERIALIZE=1 restores one
// forward at a time per GPU).  The reference tool is single-threaded on CPU cores.
// --batch N (default 1 = the path above; pBSRNN and TF-GridNet models): N consecutive lines of the scp go through ONE forward of 2 N rows
// (ws_engine_separate_ragged: every row keeps its own length, every enrollment its own -- each cut to the shorter of its
// pair as above -- so the estimates are those of --batch 1); same output names and formats; works with --jobs (a worker
// takes the next N lines) and --dry_run.  The rectangle is as long as the longest of the N.
// --sort_by_length (off by default; with --batch N): the scp lines are ordered by the mixture's sample count, longest
// first (stable), before they are grouped N at a time, so a rectangle holds rows of similar length.  The counts come from
// the wav headers (no file is loaded for it).  Outputs are still named by key and the total is unchanged; the "process:"
// lines appear in processing order.  Without --batch the flag is accepted and changes nothing.
// --chunk_seconds S [--overlap_seconds O, default S / 4] [--chunk_rows N, default 8] (long recordings; any model): every
// line goes through ws_engine_separate_long with its two enrollments -- the mixture as windows of S seconds that overlap by
// O, N window rows per forward, the estimates cross-faded on the device, the speaker encoder run once per line.  Memory
// grows with N, not with the recording.  Scaling, output names and formats as above; works with --jobs and --dry_run; not
// together with --batch N > 1 (a rectangle of whole utterances).  A mixture no longer than S is the whole-utterance forward.
// --live_ms M (with --chunk_seconds S; any model): the same windows, run as their samples arrive -- every line is fed to a
// live handle (ws_engine_live_open / push / flush) in packets of M milliseconds at the model's rate, as a capture device would
// deliver it; --overlap_seconds and --chunk_rows apply.  A sample comes out S .. S + (S - O) seconds of audio after it went in.
// Names, scaling and formats are those of the --chunk_seconds run, and with --chunk_rows 1 so are the samples, bit for bit.
// Works with --jobs, --dry_run and --resample (the files are brought to the model's rate around the handle, as for
// --chunk_seconds).  Refused without --chunk_seconds, and together with --batch N > 1, --stream_ms and the pools.
// --live_ms M --live_pool N (with --chunk_seconds S; any model): N lines of the scp are in flight at once on one live pool
// (ws_engine_live_pool_*, K = 2, one slot per line): every round feeds each line in flight its next M ms packet in ONE push, so
// the windows that complete in the same round share their forwards (--chunk_rows rows each); a line that ends is flushed, its
// slot detached and re-attached to the next line.  Names and formats are those of --live_ms; with N = 1 and --chunk_rows 1 so
// are the samples, bit for bit.  Works with --jobs, --dry_run and --resample (files go through ws_engine_resample around the
// pool, as for --live_ms).  Refused without --live_ms, and together with --batch N > 1, --stream_ms and the other pools.
// --live_hold_ms W (with --live_pool N): the windows run on the tool's clock, not the packets'.  Every round of packets is a
// ws_engine_live_pool_store (no launch); then ws_engine_live_pool_due is read and ONE ws_engine_live_pool_run takes every line
// with a complete window once --chunk_rows rows wait or the oldest complete window has waited W ms of audio (and before a
// store that would pass the pool's backlog limit).  Lines that did not start together then share their forwards: a hold of
// the hop S - O lets every line in flight ride in the same ones.  A line that ends is passed as final in the next run, its
// last window beside the others', not flushed alone.  The files are those of --live_pool (bit for bit with --chunk_rows 1);
// a sample comes out up to W ms later.  Refused without --live_pool.
// --tail_ms M [--tail_fade_ms F, default 10] [--tail_warm_seconds W, default S] [--tail_pool N, default 1] (with --chunk_seconds S;
// any model): low-latency separation on trailing windows -- N lines in flight on one tail pool (ws_engine_tail_pool_*, K = 2):
// every round pushes each line its next M ms packet and ticks, so every line runs the window of its newest S seconds and what
// is new comes out M ms plus the fade after it went in; a line that ends is flushed and its slot re-attached.  The samples
// follow the tail rule (include/wesep_engine.h), NOT the --chunk_seconds run.  A packet is cut where more than one window of
// samples would be waiting.  Works with --jobs, --dry_run and --resample; refused together with every other mode.
// --tail_ms M --tail_rate_pool N (with --chunk_seconds S; any model but TF-GridNet): the same rounds on one rate tail pool
// (ws_engine_rate_tail_pool_*, K = 2): every line is fed at its own file's sample rate, in packets of M ms at that rate cut to
// what ws_engine_rate_tail_pool_room still takes, and returned at that rate -- nothing is resampled around the pool, so
// --resample is refused with it, and so is --tail_pool.  --tail_warm_seconds defaults to 3/4 S here (the filters' look-ahead
// keeps a resampled line below a whole window before its first firing).  Outputs have the mixture's rate and length; a
// --dry_run with an --output_dir writes the (all-zero) files.
// --stream_ms M (causal cLN Conv-TasNet / SpEx+ models, ws_engine_info "streaming"): every line is fed to a stream
// (ws_engine_stream_open / push / flush) in chunks of M milliseconds, as a live source would deliver it; the speaker encoder
// runs once per line, at open.  Same files as the plain run: the streamed samples, then zeros where the plain run has its
// zero tail.  Refused on a model that cannot stream, and together with --batch N > 1 or --chunk_seconds.
// --stream_ms M --stream_pool N: N consecutive lines of the scp run CONCURRENTLY through one stream pool (ws_engine_pool_*, two
// slots per line): every round feeds each live line its next M ms packet in ONE push -- one launch chain for all of them --
// and a line that ends is flushed, its slots detached and re-attached to the next line, while the others are in mid-stream.
// Output names and formats are those of --stream_ms alone.  --stream_pool without --stream_ms, or together with --batch N > 1
// or --chunk_seconds, is refused.
// --stream_block (with --stream_ms, alone or with --stream_pool): the streams are opened with WS_STREAM_BLOCK_KERNEL -- every
// block of the separator is one call, and a line's samples do not depend on the packet size or on the lines beside it.
// Refused without --stream_ms.
// --resample (off by default: without it a file at another rate than the model's fails with "sample rate is not ..."): the
// mixture and the two enrollments may each have any sample rate within the resampler's limits (wesep_hip.h, "sample rates").
// Plain, --batch and --chunk_seconds runs bring every file to the model's rate with ws_engine_resample, run as above (seconds
// are seconds of audio) and bring the estimates back; --stream_ms feeds a rate stream (ws_engine_rate_stream_*) packets of M
// ms at the mixture's own rate.  Outputs are written at the mixture's rate with the mixture's length.  Refused together
// with --stream_pool (the pool is not rate-aware; --rate_pool N is: N lines at a time through ws_engine_rate_pool_*, every line
// at its own file's rate, packets of M ms at that rate, outputs at the mixture's rate and length; refused with --stream_pool,
// --batch N > 1 and --chunk_seconds).  A --dry_run with --resample and an --output_dir writes the files too, all
// zeros: their rate and length can be checked without a GPU.
// --dry_run validates the model file and the launch plan of every utterance without a GPU and writes nothing.
// --raw_out additionally writes the unquantised estimates as <key>-spk{1,2}.f32 (float32, for parity checks).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <fstream>
#include <functional>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../include/wesep_engine.h"
#include "wav_io.h"

namespace {

struct Args {
  std::map<std::string, std::string> kv;
  const std::string& get(const std::string& k, const std::string& dflt) const {
    auto it = kv.find(k);
    return it == kv.end() ? dflt : it->second;
  }
  bool has(const std::string& k) const { return kv.count(k) != 0; }
};

// gflags-style: --name=value, --name value, --flag
Args parse(int argc, char** argv) {
  Args a;
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    if (s.rfind("--", 0) != 0) continue;
    s = s.substr(2);
    const size_t eq = s.find('=');
    if (eq != std::string::npos) {
      a.kv[s.substr(0, eq)] = s.substr(eq + 1);
    } else if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0) {
      a.kv[s] = argv[++i];
    } else {
      a.kv[s] = "true";
    }
  }
  return a;
}

int die(const std::string& msg) {
  fprintf(stderr, "separate_main: %s\n", msg.c_str());
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  const Args args = parse(argc, argv);
  const std::string model = args.get("model", ""), out_dir = args.get("output_dir", "");
  const int sample_rate = atoi(args.get("sample_rate", "16000").c_str());
  const bool dry = args.has("dry_run"), raw_out = args.has("raw_out");
  if (model.empty()) return die("--model is required");
  if (out_dir.empty() && !dry) return die("Invalid output path.");

  std::vector<std::vector<std::string>> waves;
  if (args.has("wav_path") && args.has("spk1_emb") && args.has("spk2_emb")) {
    waves.push_back({"test", args.get("wav_path", ""), args.get("spk1_emb", ""), args.get("spk2_emb", "")});
  } else {
    std::ifstream scp(args.get("wav_scp", ""));
    std::string line;
    while (std::getline(scp, line)) {
      std::istringstream is(line);
      std::vector<std::string> f;
      std::string tok;
      while (is >> tok) f.push_back(tok);
      if (f.empty()) continue;
      if (f.size() != 4) return die("wav_scp line needs 4 fields: key mix spk1 spk2 -- got: " + line);
      waves.push_back(f);
    }
    if (waves.empty()) return die("Please provide non-empty wav scp.");
  }

  std::vector<int> devices;
  {
    std::istringstream ds(args.get("devices", args.get("device", "0")));
    std::string tok;
    while (std::getline(ds, tok, ',')) devices.push_back(atoi(tok.c_str()));
    if (devices.empty()) devices.push_back(0);
  }
  int jobs = atoi(args.get("jobs", "1").c_str());
  if (jobs < 1) jobs = 1;
  const int batch = atoi(args.get("batch", "1").c_str());
  if (batch < 1) return die("--batch needs a positive count");
  const bool chunked = args.has("chunk_seconds");
  const double chunk_s = atof(args.get("chunk_seconds", "0").c_str());
  const double overlap_s = args.has("overlap_seconds") ? atof(args.get("overlap_seconds", "0").c_str()) : chunk_s / 4;
  const int chunk_rows = atoi(args.get("chunk_rows", "8").c_str());
  const int window = static_cast<int>(chunk_s * sample_rate + 0.5), overlap = static_cast<int>(overlap_s * sample_rate + 0.5);
  const bool streamed = args.has("stream_ms");
  const double stream_ms = atof(args.get("stream_ms", "0").c_str());
  const int stream_n = static_cast<int>(stream_ms * sample_rate / 1000.0 + 0.5);
  const bool pooled = args.has("stream_pool");
  const int pool_n = atoi(args.get("stream_pool", "0").c_str());
  const bool stream_block = args.has("stream_block");
  const unsigned stream_flags = stream_block ? WS_STREAM_BLOCK_KERNEL : 0u;
  const bool resample = args.has("resample");
  const bool live = args.has("live_ms");
  const double live_ms = atof(args.get("live_ms", "0").c_str());
  const int live_n = static_cast<int>(live_ms * sample_rate / 1000.0 + 0.5);
  const bool live_pooled = args.has("live_pool");
  const int live_pool_n = atoi(args.get("live_pool", "0").c_str());
  const bool live_hold = args.has("live_hold_ms");
  const double live_hold_ms = atof(args.get("live_hold_ms", "0").c_str());
  const long long live_hold_n = static_cast<long long>(live_hold_ms * sample_rate / 1000.0 + 0.5);
  const bool tail = args.has("tail_ms");
  const double tail_ms = atof(args.get("tail_ms", "0").c_str());
  const int tail_n = static_cast<int>(tail_ms * sample_rate / 1000.0 + 0.5);
  const int tail_fade = static_cast<int>(atof(args.get("tail_fade_ms", "10").c_str()) * sample_rate / 1000.0 + 0.5);
  const int tail_warm = args.has("tail_warm_seconds") ? static_cast<int>(atof(args.get("tail_warm_seconds", "0").c_str()) * sample_rate + 0.5) : window;
  const int tail_pool_n = atoi(args.get("tail_pool", "1").c_str());
  const bool tail_rate = args.has("tail_rate_pool");
  const int tail_rate_n = atoi(args.get("tail_rate_pool", "0").c_str());
  const bool rate_pooled = args.has("rate_pool");
  const int rate_pool_n = atoi(args.get("rate_pool", "0").c_str());
  // a dry run writes nothing -- except with --resample and an --output_dir: the (all-zero) files then show the rate and the
  // length an output will have
  const bool write_out = !dry || ((resample || rate_pooled || tail_rate) && !out_dir.empty());
  if (args.has("help")) {
    printf("usage: separate_main --wav_scp scp --model model.wsw --output_dir out [--sample_rate 16000] [--devices 0,1]\n"
           "                     [--jobs J] [--batch N] [--sort_by_length] [--raw_out] [--dry_run]\n"
           "                     [--chunk_seconds S [--overlap_seconds O] [--chunk_rows N]]\n"
           "                     [--stream_ms M [--stream_pool N | --rate_pool N] [--stream_block]] [--resample]\n"
           "                     [--live_ms M --chunk_seconds S [--live_pool N [--live_hold_ms W]]]\n"
           "                     [--tail_ms M --chunk_seconds S [--tail_fade_ms F] [--tail_warm_seconds W] [--tail_pool N]]\n"
           "                     [--tail_ms M --chunk_seconds S --tail_rate_pool N [--tail_fade_ms F] [--tail_warm_seconds W]]\n"
           "  --batch N          N scp lines per forward (pBSRNN and TF-GridNet models), every row at its own length\n"
           "  --sort_by_length   with --batch N: order the lines by mixture length (longest first, stable) before grouping;\n"
           "                     outputs keep their names, the log follows the processing order.  Without --batch the flag\n"
           "                     is accepted and changes nothing\n"
           "  --chunk_seconds S  long recordings: windows of S seconds through the separator, cross-faded; the speaker\n"
           "                     encoder runs once per line.  Not together with --batch N > 1\n"
           "  --overlap_seconds O  overlap of neighbouring windows, 0 <= O <= S / 2 (default S / 4)\n"
           "  --chunk_rows N     window rows per forward (default 8): memory grows with N, not with the recording\n"
           "  --live_ms M        with --chunk_seconds S, any model: feed every line to a live handle in packets of M ms; the\n"
           "                     windows run as their samples arrive (latency S .. 2 S - O seconds); same files as the\n"
           "                     --chunk_seconds run.  Not together with --batch N > 1, --stream_ms or a pool\n"
           "  --live_pool N      with --live_ms M: N lines in flight at once on one live pool, one push per round of M ms\n"
           "                     packets; windows that complete in the same round share their forwards; same files as --live_ms\n"
           "  --live_hold_ms W   with --live_pool N: store every packet round and run all lines with a complete window at once, when\n"
           "                     --chunk_rows rows wait or the oldest window has waited W ms of audio; lines that end ride in the\n"
           "                     next run.  Lines that started apart share forwards; output up to W ms later; same files\n"
           "  --tail_ms M        with --chunk_seconds S, any model: low-latency separation on trailing windows (a tail pool): every\n"
           "                     line is fed in packets of M ms with a tick after every packet round and a flush at the end; a\n"
           "                     sample comes out M ms plus the fade after it went in, each tick costs one window of S seconds a\n"
           "                     line.  A rule of its own: NOT the files of the --chunk_seconds run\n"
           "  --tail_fade_ms F   the cross-fade between consecutive trailing windows (default 10, not a tuned value), at most S / 2\n"
           "  --tail_warm_seconds W  the audio a line needs before its first window (default S)\n"
           "  --tail_pool N      N lines in flight at once on one tail pool (default 1); every line with new audio fires on the\n"
           "                     same tick and shares the forwards; a lane takes the next line when its own ends\n"
           "  --tail_rate_pool N with --tail_ms M: N lines in flight at once on one rate tail pool, every line at its own file's\n"
           "                     sample rate (packets of M ms at that rate, no --resample); --tail_warm_seconds defaults to 3/4 S;\n"
           "                     outputs have the mixture's rate and length.  Not a TF-GridNet model, not with --tail_pool\n"
           "  --stream_ms M      causal cLN Conv-TasNet / SpEx+ models: feed every line to a stream in chunks of M ms; same\n"
           "                     files as the plain run.  Not together with --batch N > 1 or --chunk_seconds\n"
           "  --stream_pool N    with --stream_ms M: N consecutive lines at a time through one stream pool, one push per round\n"
           "                     of M ms packets; same files as --stream_ms alone\n"
           "  --stream_block     with --stream_ms M: every block of the separator as one call (WS_STREAM_BLOCK_KERNEL); the\n"
           "                     samples of a line then do not depend on the packet size or on the other lines of a pool\n"
           "  --resample         take files at any sample rate: resample to the model's rate on the device and back; outputs\n"
           "                     have the mixture's rate and length.  Not together with --stream_pool\n"
           "  --rate_pool N      with --stream_ms M: N consecutive lines at a time through one rate pool, every line at its own\n"
           "                     file's sample rate (packets of M ms at that rate); outputs have the mixture's rate and length\n");
    return 0;
  }
  if ((args.has("tail_fade_ms") || args.has("tail_warm_seconds") || args.has("tail_pool")) && !tail)
    return die("--tail_fade_ms, --tail_warm_seconds and --tail_pool need --tail_ms M: the tail pool is fed packets of M milliseconds");
  if (tail_rate && !tail) return die("--tail_rate_pool needs --tail_ms M: the rate tail pool is fed packets of M milliseconds at every line's own rate");
  if (tail_rate && args.has("tail_pool")) return die("--tail_rate_pool conflicts with --tail_pool: one pool per run; --tail_rate_pool takes lines at any rate");
  if (tail_rate && resample)
    return die("--tail_rate_pool conflicts with --resample: the rate tail pool takes every line at its own file's rate, nothing is resampled "
               "around it");
  if (tail_rate && tail_rate_n < 1) return die("--tail_rate_pool needs a positive number of lines");
  if (tail && !chunked) return die("--tail_ms needs --chunk_seconds S: a tail pool runs the trailing window of S seconds at every tick");
  if (tail && (batch > 1 || streamed || live || live_pooled || pooled || rate_pooled))
    return die("--tail_ms conflicts with --batch N > 1, --stream_ms, --live_ms, --live_pool, --stream_pool and --rate_pool: one mode per "
               "run, and a tail pool takes recordings as they arrive through the trailing windows of --chunk_seconds");
  if (tail && tail_n < 1) return die("--tail_ms needs a positive packet length");
  if (tail && tail_pool_n < 1) return die("--tail_pool needs a positive number of lines");
  if (live_hold && !live_pooled)
    return die("--live_hold_ms needs --live_pool N: only a live pool can hold complete windows back until the lines in flight share a run");
  if (live_hold && live_hold_ms < 0) return die("--live_hold_ms needs a hold of 0 ms or more");
  if (live_pooled && !live) return die("--live_pool needs --live_ms M: the pool is fed packets of M milliseconds");
  if (live_pooled && (batch > 1 || streamed || pooled || rate_pooled))
    return die("--live_pool conflicts with --batch N > 1, --stream_ms, --stream_pool and --rate_pool: one pool per run, and a live pool "
               "takes recordings as they arrive through the windows of --chunk_seconds");
  if (live_pooled && live_pool_n < 1) return die("--live_pool needs a positive number of lines");
  if (live && !chunked) return die("--live_ms needs --chunk_seconds S: a live handle runs the windows of S seconds as their samples arrive");
  if (live && (batch > 1 || streamed || pooled || rate_pooled))
    return die("--live_ms conflicts with --batch N > 1, --stream_ms, --stream_pool and --rate_pool: a live handle takes one recording as "
               "it arrives, on any model, through the windows of --chunk_seconds");
  if (live && live_n < 1) return die("--live_ms needs a positive packet length");
  if (chunked && batch > 1) return die("--chunk_seconds and --batch " + std::to_string(batch) + " conflict: a batch is a rectangle of "
                                       "whole utterances, --chunk_seconds cuts one recording into windows (use --jobs for more lines at a time)");
  if (pooled && !streamed) return die("--stream_pool needs --stream_ms M: the pool is fed packets of M milliseconds");
  if (pooled && (batch > 1 || chunked))
    return die("--stream_pool conflicts with --batch N > 1 and --chunk_seconds: the pool's lines are streams, each fed as it arrives");
  if (pooled && resample)
    return die("--resample conflicts with --stream_pool: the stream pool is not rate-aware (its pending samples live on the host); use "
               "--stream_ms alone, or --rate_pool N for lines at their own rates through one pool");
  if (rate_pooled && !streamed) return die("--rate_pool needs --stream_ms M: the pool is fed packets of M milliseconds");
  if (rate_pooled && pooled) return die("--rate_pool conflicts with --stream_pool: one pool per run; --rate_pool takes lines at any rate");
  if (rate_pooled && (batch > 1 || chunked))
    return die("--rate_pool conflicts with --batch N > 1 and --chunk_seconds: the pool's lines are streams, each fed as it arrives");
  if (rate_pooled && rate_pool_n < 1) return die("--rate_pool needs a positive number of lines");
  if (pooled && pool_n < 1) return die("--stream_pool needs a positive number of lines");
  if (stream_block && !streamed) return die("--stream_block needs --stream_ms M: it selects the block kernel of a stream or a stream pool");
  if (streamed && (batch > 1 || chunked))
    return die("--stream_ms conflicts with --batch N > 1 and --chunk_seconds: a stream takes one recording as it arrives");
  if (streamed && stream_n < 1) return die("--stream_ms needs a positive chunk length");
  if (chunked && (chunk_s <= 0 || overlap_s < 0)) return die("--chunk_seconds needs a positive length and --overlap_seconds none below 0");
  if (args.has("sort_by_length") && batch > 1) {
    std::vector<size_t> count(waves.size()), order(waves.size());
    for (size_t i = 0; i < waves.size(); ++i) {
      std::string err;
      if (!wesep_rt::peek_wav_frames(waves[i][1], &count[i], &err)) return die(err);
      order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return count[a] > count[b]; });
    std::vector<std::vector<std::string>> sorted;
    for (size_t i : order) sorted.push_back(waves[i]);
    waves.swap(sorted);
  }
  const size_t ngroups = (waves.size() + batch - 1) / batch;
  if (jobs > static_cast<int>(ngroups)) jobs = static_cast<int>(ngroups);

  std::mutex io_mu;                 // stdout / first error
  std::string first_error;
  std::atomic<size_t> next{0};
  std::atomic<bool> failed{false};
  double total_audio_ms = 0.0, total_busy_ms = 0.0;
  auto fail = [&](const std::string& msg) {
    std::lock_guard<std::mutex> l(io_mu);
    if (first_error.empty()) first_error = msg;
    failed = true;
  };
  auto worker = [&](int job) {
    ws_engine* engine = nullptr;
    long long fallbacks_seen = 0;
    if (ws_engine_create(model.c_str(), devices[job % devices.size()], dry ? WS_ENGINE_DRY_RUN : 0, &engine) != 0)
      return fail(ws_engine_last_error());
    if (ws_engine_info(engine, "sample_rate") != sample_rate) {
      ws_engine_destroy(engine);
      return fail("model sample rate differs from --sample_rate");
    }
    if (streamed && ws_engine_info(engine, "streaming") != 1) {
      ws_engine_destroy(engine);
      return fail("--stream_ms: this model cannot stream (ws_engine_info \"streaming\" is not 1): streaming needs a causal cLN "
                  "Conv-TasNet / SpEx+ container");
    }
    // --live_ms: mix [n] at the model's rate through a live handle in packets of live_n samples -> est [2][n]
    long long live_pushes = 0, live_launches = 0, live_windows = 0, live_groups = 0;
    auto run_live = [&](const float* mix, int n, const float* enr, int n_enroll, float* est) -> int {
      live_pushes = live_launches = live_windows = live_groups = 0;
      ws_live* lv = nullptr;
      int rc = ws_engine_live_open(engine, 2, enr, WS_ENROLL_WAVE, n_enroll, nullptr, window, overlap, chunk_rows, &lv);
      if (rc != 0) return rc;
      const int cap = std::max(WS_LIVE_PUSH_CAP(live_n, window - overlap), WS_LIVE_FLUSH_CAP(window, overlap));
      std::vector<float> got(size_t(2) * cap);
      int done = 0;
      auto take = [&](int m) {                                          // est [2][cap], m samples each, behind what came before
        for (int k = 0; k < 2; ++k) memcpy(est + size_t(k) * n + done, got.data() + size_t(k) * cap, size_t(m) * 4);
        done += m;
        live_launches += ws_engine_info(engine, "n_launches"), live_groups += ws_engine_info(engine, "live_groups");
      };
      for (int pos = 0; rc == 0 && pos < n; pos += live_n, ++live_pushes) {
        int m = 0;
        if ((rc = ws_engine_live_push(lv, mix + pos, std::min(live_n, n - pos), got.data(), cap, &m)) == 0) take(m);
      }
      if (rc == 0) {
        int m = 0;
        if ((rc = ws_engine_live_flush(lv, got.data(), cap, &m)) == 0) take(m);
      }
      live_windows = ws_engine_info(engine, "live_windows");
      ws_engine_live_close(lv);
      return rc;
    };
    // --resample: PCM at `rate` as floats in [-1, 1] at the model's rate, and estimates [R][n_m] back as [R][n] at `rate`
    auto to_model = [&](const std::vector<int16_t>& x, int rate, std::vector<float>* y) -> bool {
      std::vector<float> f(x.size());
      for (size_t i = 0; i < x.size(); ++i) f[i] = static_cast<float>(x[i]) / 32768.0f;
      if (rate == sample_rate) {
        y->swap(f);
        return true;
      }
      const long long cap = rate > 0 ? (static_cast<long long>(f.size()) * sample_rate + rate - 1) / rate : 0;   // ceil(U n / D)
      y->assign(static_cast<size_t>(std::max<long long>(cap, 1)), 0.f);
      int m = 0;
      if (ws_engine_resample(engine, f.data(), 1, static_cast<int>(f.size()), rate, sample_rate, y->data(), static_cast<int>(cap), &m) != 0)
        return false;
      y->resize(m);
      return true;
    };
    auto from_model = [&](const float* rows, int R, int n_m, int rate, int n, float* out) -> bool {
      if (rate == sample_rate) {
        for (int r = 0; r < R; ++r) memcpy(out + size_t(r) * n, rows + size_t(r) * n_m, size_t(std::min(n, n_m)) * 4);
        return true;
      }
      const long long cap = (static_cast<long long>(n_m) * rate + sample_rate - 1) / sample_rate;
      std::vector<float> back(size_t(R) * cap);
      int m = 0;
      if (ws_engine_resample(engine, rows, R, n_m, sample_rate, rate, back.data(), static_cast<int>(cap), &m) != 0) return false;
      for (int r = 0; r < R; ++r) memcpy(out + size_t(r) * n, back.data() + size_t(r) * m, size_t(std::min(n, m)) * 4);
      return true;
    };
    // --tail_ms M --tail_rate_pool N: up to N lines in flight on one rate tail pool (ws_engine_rate_tail_pool_*, K = 2), every line at
    // its own file's rate: a round pushes every lane its next packet of M ms at that rate -- cut to what the slot still takes -- and
    // ticks all of them; the accepted rates are those of the scp's mixtures, read before the pool is opened; outputs have the
    // mixture's rate and length.  An enrollment pair at one rate goes to the attach at that rate, another pair through
    // ws_engine_resample first.
    if (tail_rate) {
      struct Lane {
        bool live = false;
        size_t line = 0;
        std::vector<float> mix, out, got;      // at the file's rate: the mixture [n], the estimates [2][n]; a call's [2][cap]
        int n = 0, pos = 0, done = 0, slot = -1, rate = 0, packet = 0, cap = 0;
        long long pushes = 0;
        std::chrono::steady_clock::time_point t0;
      };
      std::vector<int> rates;
      for (const auto& w : waves) {
        wesep_rt::Wav hdr;
        std::string err;
        if (!wesep_rt::read_wav(w[1], &hdr, &err)) {
          fail(err);
          ws_engine_destroy(engine);
          return;
        }
        if (std::find(rates.begin(), rates.end(), hdr.sample_rate) == rates.end()) rates.push_back(hdr.sample_rate);
      }
      const int warm = args.has("tail_warm_seconds") ? tail_warm : 3 * window / 4;
      ws_rate_tail_pool* rt = nullptr;
      if (ws_engine_rate_tail_pool_open(engine, tail_rate_n, 2, window, tail_fade, warm, chunk_rows, rates.data(), static_cast<int>(rates.size()),
                                        &rt) != 0) {
        fail(std::string("--tail_rate_pool: ") + ws_engine_last_error());
        ws_engine_destroy(engine);
        return;
      }
      std::vector<Lane> lanes(tail_rate_n);
      bool ok = true;
      long long rounds = 0, launches = 0, forwards = 0, rows = 0;
      double audio_ms = 0.0;
      const auto pool_t0 = std::chrono::steady_clock::now();
      auto start = [&](Lane& ln) {                // the next line of the scp into this lane: read it, attach its two enrollments
        const size_t i = next++;
        if (i >= waves.size() || failed) return;
        const auto& w = waves[i];
        wesep_rt::Wav mix, s1, s2;
        std::string err;
        if (!wesep_rt::read_wav(w[1], &mix, &err) || !wesep_rt::read_wav(w[2], &s1, &err) || !wesep_rt::read_wav(w[3], &s2, &err)) {
          fail(err);
          ok = false;
          return;
        }
        std::vector<float> e[2];
        int enroll_rate = 0;
        if (s1.sample_rate == s2.sample_rate) {   // the attach resamples the pair
          enroll_rate = s1.sample_rate;
          for (int k = 0; k < 2; ++k)
            for (int16_t v : (k ? s2 : s1).samples) e[k].push_back(static_cast<float>(v) / 32768.0f);
        } else if (!to_model(s1.samples, s1.sample_rate, &e[0]) || !to_model(s2.samples, s2.sample_rate, &e[1])) {
          fail(w[0] + ": " + ws_engine_last_error());
          ok = false;
          return;
        }
        const int n_enroll = static_cast<int>(std::min(e[0].size(), e[1].size()));
        std::vector<float> enr(size_t(2) * n_enroll);
        memcpy(enr.data(), e[0].data(), size_t(n_enroll) * 4);
        memcpy(enr.data() + n_enroll, e[1].data(), size_t(n_enroll) * 4);
        ln.line = i, ln.n = static_cast<int>(mix.samples.size()), ln.pos = ln.done = 0, ln.pushes = 0, ln.rate = mix.sample_rate;
        ln.packet = std::max(1, static_cast<int>(tail_ms * ln.rate / 1000.0 + 0.5));
        ln.mix.resize(ln.n);
        for (int j = 0; j < ln.n; ++j) ln.mix[j] = static_cast<float>(mix.samples[j]) / 32768.0f;
        ln.out.assign(size_t(2) * ln.n, 0.f);
        ln.t0 = std::chrono::steady_clock::now();
        if (ws_engine_rate_tail_pool_attach(rt, enr.data(), WS_ENROLL_WAVE, n_enroll, nullptr, enroll_rate, ln.rate, &ln.slot) != 0) {
          fail(w[0] + ": " + ws_engine_last_error());
          ok = false;
          return;
        }
        ln.cap = ws_engine_rate_tail_pool_cap(rt, ln.slot);
        ln.got.assign(size_t(2) * ln.cap, 0.f);
        ln.live = true;
      };
      auto take = [&](Lane& ln, int m) {          // got [2][cap], m samples each, behind what came before
        for (int k = 0; k < 2; ++k) memcpy(ln.out.data() + size_t(k) * ln.n + ln.done, ln.got.data() + size_t(k) * ln.cap, size_t(m) * 4);
        ln.done += m;
      };
      auto finish = [&](Lane& ln) {               // flush the slot, free it, write the line's files at the mixture's rate
        const auto& w = waves[ln.line];
        int m = 0;
        if (ws_engine_rate_tail_pool_flush(rt, ln.slot, ln.got.data(), ln.cap, &m) != 0 || ws_engine_rate_tail_pool_detach(rt, ln.slot) != 0) {
          fail(w[0] + ": " + ws_engine_last_error());
          ok = false;
          return;
        }
        launches += ws_engine_info(engine, "n_launches"), forwards += ws_engine_info(engine, "rate_tail_pool_forwards");
        take(ln, m);
        ln.live = false;
        std::string err;
        if (ln.done != ln.n) {
          fail(w[0] + ": the rate tail pool returned " + std::to_string(ln.done) + " samples for " + std::to_string(ln.n));
          ok = false;
          return;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ln.t0).count();
        if (write_out && (!wesep_rt::write_wav(out_dir + "/" + w[0] + "-spk1.wav", ln.out.data(), ln.n, ln.rate, &err) ||
                          !wesep_rt::write_wav(out_dir + "/" + w[0] + "-spk2.wav", ln.out.data() + ln.n, ln.n, ln.rate, &err))) {
          fail(err);
          ok = false;
          return;
        }
        if (!dry && raw_out) {
          for (int k = 0; k < 2; ++k) {
            FILE* f = fopen((out_dir + "/" + w[0] + "-spk" + std::to_string(k + 1) + ".f32").c_str(), "wb");
            if (!f || fwrite(ln.out.data() + size_t(k) * ln.n, 4, ln.n, f) != size_t(ln.n)) fail("cannot write raw output");
            if (f) fclose(f);
          }
        }
        std::lock_guard<std::mutex> l(io_mu);
        printf("process: %s RTF: %.4f (rate tail pool of %d lines: %d Hz, %lld ticks, packets of %d samples, fade %d, %lld bytes of rate tail "
               "pool state)%s\n", w[0].c_str(), ms / (1000.0 * ln.n / ln.rate), tail_rate_n, ln.rate, ln.pushes, ln.packet, tail_fade,
               ws_engine_info(engine, "rate_tail_pool_state_bytes"), dry ? " [dry run]" : "");
        audio_ms += 1000.0 * ln.n / ln.rate;
      };
      for (int a = 0; a < tail_rate_n; ++a)
        if (ok) start(lanes[a]);
      while (ok && !failed) {
        std::vector<int> slots, ns, caps, n_out, who;
        std::vector<const float*> chunks;
        std::vector<float*> ests;
        for (int a = 0; a < tail_rate_n && ok; ++a) {
          Lane& ln = lanes[a];
          if (!ln.live) continue;
          const int room = ws_engine_rate_tail_pool_room(rt, ln.slot);
          if (room < 1) {                         // the last tick did not fire the line and it takes no more
            fail(waves[ln.line][0] + ": a window of audio is waiting and the line does not fire: lower --tail_warm_seconds");
            ok = false;
            break;
          }
          slots.push_back(ln.slot), ns.push_back(std::min({ln.packet, ln.n - ln.pos, room})), caps.push_back(ln.cap), who.push_back(a);
          chunks.push_back(ln.mix.data() + ln.pos), ests.push_back(ln.got.data());
        }
        if (slots.empty() || !ok) break;
        n_out.assign(slots.size(), 0);
        const int A = static_cast<int>(slots.size());
        if (ws_engine_rate_tail_pool_push(rt, A, slots.data(), chunks.data(), ns.data()) != 0 ||
            ws_engine_rate_tail_pool_tick(rt, A, slots.data(), ests.data(), caps.data(), n_out.data()) != 0) {
          fail(std::string("--tail_rate_pool: ") + ws_engine_last_error());
          ok = false;
          break;
        }
        launches += ws_engine_info(engine, "n_launches"), forwards += ws_engine_info(engine, "rate_tail_pool_forwards");
        rows += ws_engine_info(engine, "rate_tail_pool_rows"), ++rounds;
        for (size_t r = 0; r < who.size() && ok; ++r) {
          Lane& ln = lanes[who[r]];
          take(ln, n_out[r]);
          ln.pos += ns[r], ++ln.pushes;
          if (ln.pos >= ln.n) {
            finish(ln);
            if (ok) start(ln);
          }
        }
      }
      ws_engine_rate_tail_pool_close(rt);
      if (ok) {
        std::lock_guard<std::mutex> l(io_mu);
        printf("rate tail pool: %lld ticks, %lld rows, %lld forwards, %lld launches\n", rounds, rows, forwards, launches);
        total_audio_ms += audio_ms;
        total_busy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pool_t0).count();
      }
      ws_engine_destroy(engine);
      return;
    }
    // --live_pool N: up to N lines in flight on one live pool of N slots (K = 2), each fed its next packet of live_n samples at the
    // model's rate in one push per round; a lane takes the next line when its own ends.  With --resample a line's files are
    // brought to the model's rate before and its estimates back after, as for --live_ms.
    // --tail_ms M [--tail_pool N]: the same lanes on one tail pool (ws_engine_tail_pool_*): a round pushes every lane its next packet
    // -- cut so that what has not come out still fits one window -- and ticks all of them; outputs follow the tail rule.
    if (live_pooled || tail) {
      const int lanes_n = tail ? tail_pool_n : live_pool_n;
      struct Lane {
        bool live = false;
        size_t line = 0;
        std::vector<float> mix, out, got;      // at the model's rate: the mixture [n], the estimates [2][n]; a call's [2][cap]
        int n = 0, pos = 0, done = 0, slot = -1, n_file = 0, rate = 0;
        bool ending = false;                   // --live_hold_ms: every packet is stored, the next run is the line's last
        long long pushes = 0;
        std::chrono::steady_clock::time_point t0;
      };
      ws_live_pool* lp = nullptr;
      ws_tail_pool* tp = nullptr;
      const char* flag = tail ? "--tail_ms: " : "--live_pool: ";
      if ((tail ? ws_engine_tail_pool_open(engine, lanes_n, 2, window, tail_fade, tail_warm, chunk_rows, &tp)
                : ws_engine_live_pool_open(engine, lanes_n, 2, window, overlap, chunk_rows, &lp)) != 0) {
        fail(std::string(flag) + ws_engine_last_error());
        ws_engine_destroy(engine);
        return;
      }
      const int packet = tail ? tail_n : live_n;
      const int cap = tail        ? WS_TAIL_CAP(window)
                      : live_hold ? WS_LIVE_POOL_RUN_CAP(window, window - overlap)
                                  : std::max(WS_LIVE_PUSH_CAP(live_n, window - overlap), WS_LIVE_FLUSH_CAP(window, overlap));
      const char* forwards_key = tail ? "tail_pool_forwards" : "live_pool_forwards";
      std::vector<Lane> lanes(lanes_n);
      bool ok = true;
      long long rounds = 0, launches = 0, forwards = 0, pool_rounds = 0;
      double audio_ms = 0.0;
      const auto pool_t0 = std::chrono::steady_clock::now();
      auto start = [&](Lane& ln) {                // the next line of the scp into this lane: read it, attach its two enrollments
        const size_t i = next++;
        if (i >= waves.size() || failed) return;
        const auto& w = waves[i];
        wesep_rt::Wav mix, s1, s2;
        std::string err;
        if (!wesep_rt::read_wav(w[1], &mix, &err) || !wesep_rt::read_wav(w[2], &s1, &err) || !wesep_rt::read_wav(w[3], &s2, &err)) {
          fail(err);
          ok = false;
          return;
        }
        if (!resample && (mix.sample_rate != sample_rate || s1.sample_rate != sample_rate || s2.sample_rate != sample_rate)) {
          fail(w[0] + ": sample rate is not " + std::to_string(sample_rate));
          ok = false;
          return;
        }
        std::vector<float> e[2];
        if (!to_model(mix.samples, mix.sample_rate, &ln.mix) || !to_model(s1.samples, s1.sample_rate, &e[0]) ||
            !to_model(s2.samples, s2.sample_rate, &e[1])) {
          fail(w[0] + ": " + ws_engine_last_error());
          ok = false;
          return;
        }
        const int n_enroll = static_cast<int>(std::min(e[0].size(), e[1].size()));
        std::vector<float> enr(size_t(2) * n_enroll);
        memcpy(enr.data(), e[0].data(), size_t(n_enroll) * 4);
        memcpy(enr.data() + n_enroll, e[1].data(), size_t(n_enroll) * 4);
        ln.line = i, ln.n = static_cast<int>(ln.mix.size()), ln.pos = ln.done = 0, ln.pushes = 0, ln.ending = false;
        ln.n_file = static_cast<int>(mix.samples.size()), ln.rate = resample ? mix.sample_rate : sample_rate;
        ln.out.assign(size_t(2) * ln.n, 0.f);
        ln.got.assign(size_t(2) * cap, 0.f);
        ln.t0 = std::chrono::steady_clock::now();
        if ((tail ? ws_engine_tail_pool_attach(tp, enr.data(), WS_ENROLL_WAVE, n_enroll, nullptr, &ln.slot)
                  : ws_engine_live_pool_attach(lp, enr.data(), WS_ENROLL_WAVE, n_enroll, nullptr, &ln.slot)) != 0) {
          fail(w[0] + ": " + ws_engine_last_error());
          ok = false;
          return;
        }
        ln.live = true;
      };
      auto take = [&](Lane& ln, int m) {          // got [2][cap], m samples each, behind what came before
        for (int k = 0; k < 2; ++k) memcpy(ln.out.data() + size_t(k) * ln.n + ln.done, ln.got.data() + size_t(k) * cap, size_t(m) * 4);
        ln.done += m;
      };
      auto write_line = [&](Lane& ln) {           // the line is complete: write its files at the mixture's rate
        const auto& w = waves[ln.line];
        std::string err;
        ln.live = false;
        std::vector<float> out(size_t(2) * ln.n_file, 0.f);
        if (!from_model(ln.out.data(), 2, ln.n, ln.rate, ln.n_file, out.data())) {
          fail(w[0] + ": " + ws_engine_last_error());
          ok = false;
          return;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ln.t0).count();
        if (write_out && (!wesep_rt::write_wav(out_dir + "/" + w[0] + "-spk1.wav", out.data(), ln.n_file, ln.rate, &err) ||
                          !wesep_rt::write_wav(out_dir + "/" + w[0] + "-spk2.wav", out.data() + ln.n_file, ln.n_file, ln.rate, &err))) {
          fail(err);
          ok = false;
          return;
        }
        if (!dry && raw_out) {
          for (int k = 0; k < 2; ++k) {
            FILE* f = fopen((out_dir + "/" + w[0] + "-spk" + std::to_string(k + 1) + ".f32").c_str(), "wb");
            if (!f || fwrite(out.data() + size_t(k) * ln.n_file, 4, ln.n_file, f) != size_t(ln.n_file)) fail("cannot write raw output");
            if (f) fclose(f);
          }
        }
        std::lock_guard<std::mutex> l(io_mu);
        if (tail)
          printf("process: %s RTF: %.4f (tail pool of %d lines: %lld ticks, packets of %d samples, fade %d, %lld bytes of tail pool state)%s\n",
                 w[0].c_str(), ms / (1000.0 * ln.n_file / ln.rate), lanes_n, ln.pushes, packet, tail_fade,
                 ws_engine_info(engine, "tail_pool_state_bytes"), dry ? " [dry run]" : "");
        else
          printf("process: %s RTF: %.4f (live pool of %d lines: %lld pushes of %d samples, %lld bytes of live pool state)%s\n", w[0].c_str(),
                 ms / (1000.0 * ln.n_file / ln.rate), live_pool_n, ln.pushes, live_n, ws_engine_info(engine, "live_pool_state_bytes"),
                 dry ? " [dry run]" : "");
        audio_ms += 1000.0 * ln.n_file / ln.rate;
      };
      auto finish = [&](Lane& ln) {               // flush the slot, free it, write the line's files
        int m = 0;
        if (tail ? ws_engine_tail_pool_flush(tp, ln.slot, ln.got.data(), cap, &m) != 0 || ws_engine_tail_pool_detach(tp, ln.slot) != 0
                 : ws_engine_live_pool_flush(lp, ln.slot, ln.got.data(), cap, &m) != 0 || ws_engine_live_pool_detach(lp, ln.slot) != 0) {
          fail(waves[ln.line][0] + ": " + ws_engine_last_error());
          ok = false;
          return;
        }
        launches += ws_engine_info(engine, "n_launches"), forwards += ws_engine_info(engine, forwards_key);
        take(ln, m);
        write_line(ln);
      };
      // --live_hold_ms: ONE run of every line in flight -- the complete windows of all of them in the same forwards, the lines
      // that have ended as final -- then the ended lines' files and the next lines of the scp into their lanes
      auto run_held = [&]() {
        std::vector<int> slots, finals, caps, n_out, who;
        std::vector<float*> ests;
        for (int a = 0; a < lanes_n; ++a) {
          Lane& ln = lanes[a];
          if (!ln.live) continue;
          slots.push_back(ln.slot), finals.push_back(ln.ending ? 1 : 0), caps.push_back(cap), who.push_back(a), ests.push_back(ln.got.data());
        }
        if (slots.empty()) return;
        n_out.assign(slots.size(), 0);
        if (ws_engine_live_pool_run(lp, static_cast<int>(slots.size()), slots.data(), finals.data(), ests.data(), caps.data(), n_out.data()) != 0) {
          fail(std::string(flag) + ws_engine_last_error());
          ok = false;
          return;
        }
        launches += ws_engine_info(engine, "n_launches"), forwards += ws_engine_info(engine, forwards_key);
        pool_rounds += ws_engine_info(engine, "live_pool_rounds");
        for (size_t r = 0; r < who.size() && ok; ++r) {
          Lane& ln = lanes[who[r]];
          take(ln, n_out[r]);
          if (!ln.ending) continue;
          if (ws_engine_live_pool_detach(lp, ln.slot) != 0) {
            fail(waves[ln.line][0] + ": " + ws_engine_last_error());
            ok = false;
            return;
          }
          write_line(ln);
          if (ok) start(ln);
        }
      };
      for (int a = 0; a < lanes_n; ++a)
        if (ok) start(lanes[a]);
      while (ok && !failed) {
        std::vector<int> slots, ns, caps, n_out, who;
        std::vector<const float*> chunks;
        std::vector<float*> ests;
        if (live_hold) {                          // a store must leave every line below the pool's backlog limit: run first
          bool full = false;
          for (const Lane& ln : lanes)
            full = full || (ln.live && !ln.ending &&
                            (long long)(ln.pos - ln.done) + std::min(packet, ln.n - ln.pos) >= WS_LIVE_POOL_STORE_LIMIT((long long)window, window - overlap));
          if (full) run_held();
          if (!ok) break;
        }
        for (int a = 0; a < lanes_n; ++a) {
          Lane& ln = lanes[a];
          if (!ln.live || ln.ending) continue;
          // (a tail pool holds at most one window of samples that have not come out: ln.pos - ln.done of them are waiting)
          const int room = tail ? window - (ln.pos - ln.done) : packet;
          slots.push_back(ln.slot), ns.push_back(std::min({packet, ln.n - ln.pos, room})), caps.push_back(cap), who.push_back(a);
          chunks.push_back(ln.mix.data() + ln.pos), ests.push_back(ln.got.data());
        }
        if (slots.empty() && !live_hold) break;
        n_out.assign(slots.size(), 0);
        const int A = static_cast<int>(slots.size());
        if (live_hold) {
          bool waiting = false;                   // lines that have ended and wait for their last run
          for (const Lane& ln : lanes) waiting = waiting || (ln.live && ln.ending);
          if (slots.empty() && !waiting) break;
          if (!slots.empty()) {
            if (ws_engine_live_pool_store(lp, A, slots.data(), chunks.data(), ns.data()) != 0) {
              fail(std::string(flag) + ws_engine_last_error());
              ok = false;
              break;
            }
            ++rounds;
            for (size_t r = 0; r < who.size(); ++r) {
              Lane& ln = lanes[who[r]];
              ln.pos += ns[r], ++ln.pushes;
              ln.ending = ln.pos >= ln.n;
            }
          }
          long long rows_ready = 0, oldest_age = 0;
          if (ws_engine_live_pool_due(lp, &rows_ready, &oldest_age) != 0) {
            fail(std::string(flag) + ws_engine_last_error());
            ok = false;
            break;
          }
          // run: enough rows for a forward, a window that has waited its hold, or nothing left to store (only ended lines wait)
          if (rows_ready >= chunk_rows || (rows_ready > 0 && oldest_age >= live_hold_n) || slots.empty()) run_held();
          continue;
        }
        if (tail ? ws_engine_tail_pool_push(tp, A, slots.data(), chunks.data(), ns.data()) != 0 ||
                       ws_engine_tail_pool_tick(tp, A, slots.data(), ests.data(), caps.data(), n_out.data()) != 0
                 : ws_engine_live_pool_push(lp, A, slots.data(), chunks.data(), ns.data(), ests.data(), caps.data(), n_out.data()) != 0) {
          fail(std::string(flag) + ws_engine_last_error());
          ok = false;
          break;
        }
        launches += ws_engine_info(engine, "n_launches"), forwards += ws_engine_info(engine, forwards_key);
        pool_rounds += tail ? ws_engine_info(engine, "tail_pool_rows") : ws_engine_info(engine, "live_pool_rounds"), ++rounds;
        for (size_t r = 0; r < who.size() && ok; ++r) {
          Lane& ln = lanes[who[r]];
          take(ln, n_out[r]);
          ln.pos += ns[r], ++ln.pushes;
          if (ln.pos >= ln.n) {
            finish(ln);
            if (ok) start(ln);
          }
        }
      }
      ws_engine_live_pool_close(lp);
      ws_engine_tail_pool_close(tp);
      if (ok) {
        std::lock_guard<std::mutex> l(io_mu);
        if (tail)
          printf("tail pool: %lld ticks, %lld rows, %lld forwards, %lld launches\n", rounds, pool_rounds, forwards, launches);
        else
          printf("live pool: %lld pushes, %lld rounds, %lld forwards, %lld launches\n", rounds, pool_rounds, forwards, launches);
        total_audio_ms += audio_ms;
        total_busy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pool_t0).count();
      }
      ws_engine_destroy(engine);
      return;
    }
    // --stream_pool N: up to N lines in flight on one pool of 2 N slots; a lane takes the next line when its own ends.
    // --rate_pool N: the same through one rate pool (ws_engine_rate_pool_*), every line at its own file's rate; the accepted rates
    // are those of the scp's mixtures, read before the pool is opened; outputs have the mixture's rate and length.
    // One lane driver for both: PoolDriver holds what they differ in.
    if (pooled || rate_pooled) {
      struct Lane {
        bool live = false;
        size_t line = 0;
        wesep_rt::Wav mix;
        std::vector<float> out, chunk;
        int n = 0, pos = 0, done = 0, packet = 0, slot[2] = {-1, -1};
        long long pushes = 0;
        std::chrono::steady_clock::time_point t0;
      };
      struct PoolDriver {
        const char *flag, *name;          // in messages; in the printed lines
        int lanes = 0;
        bool any_rate = false;            // every line at its own file's rate; else every file must be at --sample_rate
        bool writes = false;              // the line's files are written
        std::function<int(const float* enroll, int n_enroll, int rate, int* slot)> attach;
        std::function<int(int n_active, const int* slots, const float* const* chunks, const int* n, float* const* est, const int* est_cap,
                          int* n_out)> push;
        std::function<int(int slot, float* est, int est_cap, int* n_out)> flush;
        std::function<int(int slot)> detach;
        std::function<int(int slot, int packet)> cap;     // samples a push of `packet` samples or the flush returns at most
        std::function<void()> close;
      } d;
      ws_pool* pool = nullptr;
      ws_rate_pool* rpool = nullptr;
      if (rate_pooled) {
        std::vector<int> rates;
        int max_packet = 1;
        for (const auto& w : waves) {
          wesep_rt::Wav hdr;
          std::string err;
          if (!wesep_rt::read_wav(w[1], &hdr, &err)) {
            fail(err);
            ws_engine_destroy(engine);
            return;
          }
          if (std::find(rates.begin(), rates.end(), hdr.sample_rate) == rates.end()) rates.push_back(hdr.sample_rate);
          max_packet = std::max(max_packet, static_cast<int>(stream_ms * hdr.sample_rate / 1000.0 + 0.5));
        }
        d.flag = "--rate_pool", d.name = "rate pool", d.lanes = rate_pool_n, d.any_rate = true, d.writes = write_out;
        if (ws_engine_rate_pool_open(engine, 2 * rate_pool_n, 64, stream_flags, rates.data(), static_cast<int>(rates.size()), max_packet, &rpool) != 0) {
          fail(std::string("--rate_pool: ") + ws_engine_last_error());
          ws_engine_destroy(engine);
          return;
        }
        d.attach = [&](const float* e, int ne, int rate, int* slot) { return ws_engine_rate_pool_attach(rpool, e, WS_ENROLL_WAVE, ne, 0, rate, slot); };
        d.push = [&](int na, const int* sl, const float* const* ch, const int* n, float* const* est, const int* cap, int* m) {
          return ws_engine_rate_pool_push(rpool, na, sl, ch, n, est, cap, m);
        };
        d.flush = [&](int slot, float* est, int cap, int* m) { return ws_engine_rate_pool_flush(rpool, slot, est, cap, m); };
        d.detach = [&](int slot) { return ws_engine_rate_pool_detach(rpool, slot); };
        d.cap = [&](int slot, int packet) { return std::max(ws_engine_rate_pool_push_cap(rpool, slot, packet), ws_engine_rate_pool_push_cap(rpool, slot, 0)); };
        d.close = [&] { ws_engine_rate_pool_close(rpool); };
      } else {
        d.flag = "--stream_pool", d.name = "pool", d.lanes = pool_n, d.any_rate = false, d.writes = !dry;
        if (ws_engine_pool_open_ex(engine, 2 * pool_n, 64, stream_flags, &pool) != 0) {
          fail(std::string("--stream_pool: ") + ws_engine_last_error());
          ws_engine_destroy(engine);
          return;
        }
        const int L = static_cast<int>(ws_engine_info(engine, "L"));
        d.attach = [&](const float* e, int ne, int, int* slot) { return ws_engine_pool_attach(pool, e, WS_ENROLL_WAVE, ne, slot); };
        d.push = [&](int na, const int* sl, const float* const* ch, const int* n, float* const* est, const int* cap, int* m) {
          return ws_engine_pool_push(pool, na, sl, ch, n, est, cap, m);
        };
        d.flush = [&](int slot, float* est, int cap, int* m) { return ws_engine_pool_flush(pool, slot, est, cap, m); };
        d.detach = [&](int slot) { return ws_engine_pool_detach(pool, slot); };
        d.cap = [L](int, int packet) { return std::max(WS_STREAM_PUSH_CAP(packet, L), WS_STREAM_FLUSH_CAP); };
        d.close = [&] { ws_engine_pool_close(pool); };
      }
      std::vector<Lane> lanes(d.lanes);
      std::vector<std::vector<float>> got(size_t(2) * d.lanes);
      bool ok = true;
      long long rounds = 0, launches = 0;
      double audio_ms = 0.0;
      const auto pool_t0 = std::chrono::steady_clock::now();
      auto start = [&](Lane& ln, int lane_id) {   // the next line of the scp into this lane: read it, attach its two enrollments
        const size_t i = next++;
        if (i >= waves.size() || failed) return;
        const auto& w = waves[i];
        wesep_rt::Wav s1, s2;
        std::string err;
        if (!wesep_rt::read_wav(w[1], &ln.mix, &err) || !wesep_rt::read_wav(w[2], &s1, &err) || !wesep_rt::read_wav(w[3], &s2, &err)) {
          fail(err);
          ok = false;
          return;
        }
        if (!d.any_rate && (ln.mix.sample_rate != sample_rate || s1.sample_rate != sample_rate || s2.sample_rate != sample_rate)) {
          fail(w[0] + ": sample rate is not " + std::to_string(sample_rate));
          ok = false;
          return;
        }
        const int rate = ln.mix.sample_rate;
        ln.line = i, ln.n = static_cast<int>(ln.mix.samples.size()), ln.pos = ln.done = 0, ln.pushes = 0;
        ln.packet = std::max(1, static_cast<int>(stream_ms * rate / 1000.0 + 0.5));      // M ms at the line's rate
        ln.out.assign(size_t(2) * ln.n, 0.f);
        ln.t0 = std::chrono::steady_clock::now();
        std::vector<float> e[2];               // the enrollments at the model's rate, cut to the shorter one
        if (!to_model(s1.samples, s1.sample_rate, &e[0]) || !to_model(s2.samples, s2.sample_rate, &e[1])) {
          fail(w[0] + ": " + ws_engine_last_error());
          ok = false;
          return;
        }
        const int n_enroll = static_cast<int>(std::min(e[0].size(), e[1].size()));
        for (int k = 0; k < 2; ++k) {
          if (d.attach(e[k].data(), n_enroll, rate, &ln.slot[k]) != 0) {
            fail(w[0] + ": " + ws_engine_last_error());
            ok = false;
            return;
          }
          got[size_t(2) * lane_id + k].assign(size_t(std::max(d.cap(ln.slot[k], ln.packet), 1)), 0.f);
        }
        ln.live = true;
      };
      auto finish = [&](Lane& ln, int lane_id) {  // flush both slots, free them, write the line's files at the mixture's rate
        const auto& w = waves[ln.line];
        const int rate = ln.mix.sample_rate;
        std::string err;
        for (int k = 0; k < 2 && ok; ++k) {
          int m = 0;
          std::vector<float>& g = got[size_t(2) * lane_id + k];
          if (d.flush(ln.slot[k], g.data(), static_cast<int>(g.size()), &m) != 0 || d.detach(ln.slot[k]) != 0) {
            fail(w[0] + ": " + ws_engine_last_error());
            ok = false;
            return;
          }
          launches += ws_engine_info(engine, "n_launches");
          memcpy(ln.out.data() + size_t(k) * ln.n + ln.done, g.data(), size_t(std::max(0, std::min(m, ln.n - ln.done))) * 4);
        }
        ln.live = false;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ln.t0).count();
        if (d.writes && (!wesep_rt::write_wav(out_dir + "/" + w[0] + "-spk1.wav", ln.out.data(), ln.n, rate, &err) ||
                         !wesep_rt::write_wav(out_dir + "/" + w[0] + "-spk2.wav", ln.out.data() + ln.n, ln.n, rate, &err))) {
          fail(err);
          ok = false;
          return;
        }
        if (d.writes && raw_out) {
          for (int k = 0; k < 2; ++k) {
            FILE* f = fopen((out_dir + "/" + w[0] + "-spk" + std::to_string(k + 1) + ".f32").c_str(), "wb");
            if (!f || fwrite(ln.out.data() + size_t(k) * ln.n, 4, ln.n, f) != size_t(ln.n)) fail("cannot write raw output");
            if (f) fclose(f);
          }
        }
        const std::string at = d.any_rate ? " at " + std::to_string(rate) + " Hz" : "";
        std::lock_guard<std::mutex> l(io_mu);
        printf("process: %s RTF: %.4f (%s of %d lines: %lld pushes of %d samples%s, %lld bytes of stream state)%s\n", w[0].c_str(),
               ms / (1000.0 * ln.n / rate), d.name, d.lanes, ln.pushes, ln.packet, at.c_str(), ws_engine_info(engine, "stream_state_bytes"),
               dry ? " [dry run]" : "");
        audio_ms += 1000.0 * ln.n / rate;
      };
      for (int a = 0; a < d.lanes; ++a)
        if (ok) start(lanes[a], a);
      while (ok && !failed) {
        std::vector<int> slots, ns, caps, n_out;
        std::vector<const float*> chunks;
        std::vector<float*> ests;
        for (int a = 0; a < d.lanes; ++a) {
          Lane& ln = lanes[a];
          if (!ln.live) continue;
          const int c = std::min(ln.packet, ln.n - ln.pos);
          ln.chunk.resize(c);
          for (int j = 0; j < c; ++j) ln.chunk[j] = static_cast<float>(ln.mix.samples[ln.pos + j]) / 32768.0f;
          for (int k = 0; k < 2; ++k) {
            slots.push_back(ln.slot[k]), ns.push_back(c), caps.push_back(static_cast<int>(got[size_t(2) * a + k].size()));
            chunks.push_back(ln.chunk.data()), ests.push_back(got[size_t(2) * a + k].data());
          }
        }
        if (slots.empty()) break;
        n_out.assign(slots.size(), 0);
        if (d.push(static_cast<int>(slots.size()), slots.data(), chunks.data(), ns.data(), ests.data(), caps.data(), n_out.data()) != 0) {
          fail(std::string(d.flag) + ": " + ws_engine_last_error());
          ok = false;
          break;
        }
        launches += ws_engine_info(engine, "n_launches"), ++rounds;
        size_t row = 0;
        for (int a = 0; a < d.lanes && ok; ++a) {
          Lane& ln = lanes[a];
          if (!ln.live) continue;
          for (int k = 0; k < 2; ++k, ++row)
            memcpy(ln.out.data() + size_t(k) * ln.n + ln.done, ests[row], size_t(std::max(0, std::min(n_out[row], ln.n - ln.done))) * 4);
          ln.done += std::min(n_out[row - 1], ln.n - ln.done), ln.pos += ns[row - 1], ++ln.pushes;
          if (ln.pos >= ln.n) {
            finish(ln, a);
            if (ok) start(ln, a);
          }
        }
      }
      d.close();
      if (ok) {
        std::lock_guard<std::mutex> l(io_mu);
        printf("%s: %lld rounds, %lld launches\n", d.name, rounds, launches);
        total_audio_ms += audio_ms;
        total_busy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pool_t0).count();
      }
      ws_engine_destroy(engine);
      return;
    }
    // --batch N > 1: group g = lines [g N, g N + N) in one ragged forward, two rows per line
    for (size_t g = batch > 1 ? next++ : ngroups; g < ngroups && !failed; g = next++) {
      const size_t i0 = g * batch, B = (i0 + batch <= waves.size() ? i0 + batch : waves.size()) - i0;
      std::vector<wesep_rt::Wav> mix(B), s1(B), s2(B);
      std::vector<int> lengths(2 * B), elens(2 * B);
      std::vector<std::vector<float>> mix_f(B), e1_f(B), e2_f(B);     // --resample: the line's files at the model's rate
      std::string err;
      int T = 0, Te = 0;
      bool ok = true;
      for (size_t b = 0; b < B && ok; ++b) {
        const auto& w = waves[i0 + b];
        if (!wesep_rt::read_wav(w[1], &mix[b], &err) || !wesep_rt::read_wav(w[2], &s1[b], &err) ||
            !wesep_rt::read_wav(w[3], &s2[b], &err)) {
          fail(err);
          ok = false;
        } else if (!resample && (mix[b].sample_rate != sample_rate || s1[b].sample_rate != sample_rate || s2[b].sample_rate != sample_rate)) {
          fail(w[0] + ": sample rate is not " + std::to_string(sample_rate));
          ok = false;
        } else if (resample && (!to_model(mix[b].samples, mix[b].sample_rate, &mix_f[b]) || !to_model(s1[b].samples, s1[b].sample_rate, &e1_f[b]) ||
                                !to_model(s2[b].samples, s2[b].sample_rate, &e2_f[b]))) {
          fail(w[0] + ": " + ws_engine_last_error());
          ok = false;
        } else {
          const int n = static_cast<int>(resample ? mix_f[b].size() : mix[b].samples.size());
          const int ne = static_cast<int>(resample ? std::min(e1_f[b].size(), e2_f[b].size())
                                                   : std::min(s1[b].samples.size(), s2[b].samples.size()));
          lengths[2 * b] = lengths[2 * b + 1] = n;
          elens[2 * b] = elens[2 * b + 1] = ne;
          T = n > T ? n : T;
          Te = ne > Te ? ne : Te;
        }
      }
      if (!ok) break;
      // the rows of ws_engine_forward_pcm16, for B lines: the mixture twice, one row per enrollment, scaled to [-1, 1]
      std::vector<float> m(2 * B * size_t(T), 0.f), enr(2 * B * size_t(Te), 0.f), out(2 * B * size_t(T), 0.f);
      for (size_t b = 0; b < B; ++b) {
        for (int k = 0; k < 2; ++k) {
          float* mr = m.data() + (2 * b + k) * size_t(T);
          float* er = enr.data() + (2 * b + k) * size_t(Te);
          if (resample) {
            memcpy(mr, mix_f[b].data(), size_t(lengths[2 * b]) * 4);
            memcpy(er, (k == 0 ? e1_f[b] : e2_f[b]).data(), size_t(elens[2 * b]) * 4);
            continue;
          }
          const std::vector<int16_t>& src = k == 0 ? s1[b].samples : s2[b].samples;
          for (int i = 0; i < lengths[2 * b]; ++i) mr[i] = static_cast<float>(mix[b].samples[i]) / 32768.0f;
          for (int i = 0; i < elens[2 * b]; ++i) er[i] = static_cast<float>(src[i]) / 32768.0f;
        }
      }
      const auto t0 = std::chrono::steady_clock::now();
      if (ws_engine_separate_ragged(engine, m.data(), static_cast<int>(2 * B), T, lengths.data(), enr.data(), WS_ENROLL_WAVE, Te,
                                    elens.data(), out.data()) != 0) {
        fail(waves[i0][0] + " (batch of " + std::to_string(B) + "): " + ws_engine_last_error());
        break;
      }
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      const long long batch_launches = ws_engine_info(engine, "n_launches");
      double audio_ms = 0.0;
      std::vector<float> back;
      for (size_t b = 0; b < B && ok; ++b) {
        const std::string& key = waves[i0 + b][0];
        int n = lengths[2 * b], Tp = T, out_rate = sample_rate;
        const float* o = out.data() + 2 * b * size_t(T);
        if (resample) {                   // the line's two estimates back at the mixture's rate and length
          const int n_m = n;
          std::vector<float> two(size_t(2) * n_m);
          for (int k = 0; k < 2; ++k) memcpy(two.data() + size_t(k) * n_m, o + size_t(k) * T, size_t(n_m) * 4);
          n = Tp = static_cast<int>(mix[b].samples.size()), out_rate = mix[b].sample_rate;
          back.assign(size_t(2) * n, 0.f);
          if (!from_model(two.data(), 2, n_m, out_rate, n, back.data())) {
            fail(key + ": " + ws_engine_last_error());
            ok = false;
            break;
          }
          o = back.data();
        }
        audio_ms += 1000.0 * n / out_rate;
        if (write_out && (!wesep_rt::write_wav(out_dir + "/" + key + "-spk1.wav", o, n, out_rate, &err) ||
                     !wesep_rt::write_wav(out_dir + "/" + key + "-spk2.wav", o + Tp, n, out_rate, &err))) {
          fail(err);
          ok = false;
        }
        if (ok && !dry && raw_out) {
          for (int k = 0; k < 2; ++k) {
            FILE* f = fopen((out_dir + "/" + key + "-spk" + std::to_string(k + 1) + ".f32").c_str(), "wb");
            if (!f || fwrite(o + size_t(k) * Tp, 4, n, f) != size_t(n)) fail("cannot write raw output");
            if (f) fclose(f);
          }
        }
      }
      if (!ok) break;
      std::lock_guard<std::mutex> l(io_mu);
      for (size_t b = 0; b < B; ++b)
        printf("process: %s RTF: %.4f (batch of %zu: %lld launches, %lld MiB arena)%s\n", waves[i0 + b][0].c_str(), ms / audio_ms,
               B, batch_launches, ws_engine_info(engine, "arena_bytes") >> 20, dry ? " [dry run]" : "");
      if (ws_engine_info(engine, "cluster_fallbacks") > fallbacks_seen) {
        fallbacks_seen = ws_engine_info(engine, "cluster_fallbacks");
        printf("note: %s: a cluster recurrence timed out (GPU shared); recomputed by the streaming kernels\n",
               waves[i0][0].c_str());
      }
      total_audio_ms += audio_ms;
      total_busy_ms += ms;
    }
    for (size_t i = batch > 1 ? waves.size() : next++; i < waves.size() && !failed; i = next++) {
      const auto& w = waves[i];
      wesep_rt::Wav mix, s1, s2;
      std::string err;
      if (!wesep_rt::read_wav(w[1], &mix, &err) || !wesep_rt::read_wav(w[2], &s1, &err) ||
          !wesep_rt::read_wav(w[3], &s2, &err)) {
        fail(err);
        break;
      }
      if (!resample && (mix.sample_rate != sample_rate || s1.sample_rate != sample_rate || s2.sample_rate != sample_rate)) {
        fail(w[0] + ": sample rate is not " + std::to_string(sample_rate));
        break;
      }
      const int n = static_cast<int>(mix.samples.size());
      const int out_rate = resample ? mix.sample_rate : sample_rate;      // outputs have the mixture's rate and length
      int n_enroll = static_cast<int>(s1.samples.size() < s2.samples.size() ? s1.samples.size() : s2.samples.size());
      std::vector<float> out(size_t(2) * n, 0.f);
      const auto t0 = std::chrono::steady_clock::now();
      int rc;
      long long stream_launches = 0, stream_pushes = 0, plain_launches = -1, long_w = 0, long_f = 0;
      int stream_samples = stream_n;
      if (resample) {
        // every file at the model's rate (the enrollments cut to the shorter one there); a stream takes the mixture as it is
        std::vector<float> mix_f, e1, e2;
        rc = to_model(s1.samples, s1.sample_rate, &e1) && to_model(s2.samples, s2.sample_rate, &e2) &&
                     (streamed || to_model(mix.samples, mix.sample_rate, &mix_f)) ? 0 : -1;
        n_enroll = static_cast<int>(std::min(e1.size(), e2.size()));
        std::vector<float> enr(size_t(2) * n_enroll);
        if (rc == 0) {
          memcpy(enr.data(), e1.data(), size_t(n_enroll) * 4);
          memcpy(enr.data() + n_enroll, e2.data(), size_t(n_enroll) * 4);
        }
        const int n_m = static_cast<int>(mix_f.size());
        if (rc == 0 && streamed) {
          stream_samples = std::max(1, static_cast<int>(stream_ms * out_rate / 1000.0 + 0.5));
          ws_rate_stream* rs = nullptr;
          rc = ws_engine_rate_stream_open(engine, 2, enr.data(), WS_ENROLL_WAVE, n_enroll, 0, 64, stream_flags, out_rate, stream_samples, &rs);
          const int cap = rc == 0 ? std::max(ws_engine_rate_stream_push_cap(rs, stream_samples), ws_engine_rate_stream_push_cap(rs, 0)) : 1;
          std::vector<float> chunk(size_t(2) * stream_samples), got(size_t(2) * cap);
          int done = 0;
          auto take = [&](int m) {                                      // est [2][m] behind what came before; never past n
            const int c = std::min(m, n - done);
            for (int k = 0; k < 2; ++k) memcpy(out.data() + size_t(k) * n + done, got.data() + size_t(k) * m, size_t(c) * 4);
            done += c;
          };
          for (int pos = 0; rc == 0 && pos < n; pos += stream_samples) {
            const int c = std::min(stream_samples, n - pos);
            int m = 0;
            for (int i = 0; i < c; ++i) chunk[i] = chunk[size_t(c) + i] = static_cast<float>(mix.samples[pos + i]) / 32768.0f;
            if ((rc = ws_engine_rate_stream_push(rs, chunk.data(), c, got.data(), cap, &m)) == 0) take(m);
            stream_launches += ws_engine_info(engine, "n_launches"), ++stream_pushes;
          }
          if (rc == 0) {
            int m = 0;
            if ((rc = ws_engine_rate_stream_flush(rs, got.data(), cap, &m)) == 0) take(m);
            stream_launches += ws_engine_info(engine, "n_launches");
          }
          ws_engine_rate_stream_close(rs);
        } else if (rc == 0) {
          std::vector<float> out_m(size_t(2) * n_m, 0.f);
          if (live) {
            rc = run_live(mix_f.data(), n_m, enr.data(), n_enroll, out_m.data());
          } else if (chunked) {
            rc = ws_engine_separate_long(engine, mix_f.data(), n_m, 2, enr.data(), WS_ENROLL_WAVE, n_enroll, nullptr, window, overlap,
                                         chunk_rows, out_m.data());
          } else {                                                      // the rows of ws_engine_forward_pcm16: the mixture twice
            std::vector<float> two(size_t(2) * n_m);
            memcpy(two.data(), mix_f.data(), size_t(n_m) * 4);
            memcpy(two.data() + n_m, mix_f.data(), size_t(n_m) * 4);
            rc = ws_engine_separate(engine, two.data(), 2, n_m, enr.data(), WS_ENROLL_WAVE, n_enroll, out_m.data());
          }
          plain_launches = ws_engine_info(engine, "n_launches");       // (the resampling back resets the engine's counters)
          long_w = ws_engine_info(engine, "long_windows"), long_f = ws_engine_info(engine, "long_forwards");
          if (rc == 0 && !from_model(out_m.data(), 2, n_m, out_rate, n, out.data())) rc = -1;
        }
      } else if (streamed) {
        // the rows of ws_engine_forward_pcm16, pushed as they would arrive; what becomes final goes behind what came before
        std::vector<float> enr(size_t(2) * n_enroll), chunk(size_t(2) * stream_n), got;
        for (int i = 0; i < n_enroll; ++i) {
          enr[i] = static_cast<float>(s1.samples[i]) / 32768.0f;
          enr[size_t(n_enroll) + i] = static_cast<float>(s2.samples[i]) / 32768.0f;
        }
        const int L = static_cast<int>(ws_engine_info(engine, "L"));
        const int cap = std::max(WS_STREAM_PUSH_CAP(stream_n, L), WS_STREAM_FLUSH_CAP);
        got.resize(size_t(2) * cap);
        ws_stream* st = nullptr;
        rc = ws_engine_stream_open_ex(engine, 2, enr.data(), WS_ENROLL_WAVE, n_enroll, 64, stream_flags, &st);
        int done = 0;
        auto take = [&](int m) {                                        // est [2][m] behind what came before
          for (int k = 0; k < 2; ++k) memcpy(out.data() + size_t(k) * n + done, got.data() + size_t(k) * m, size_t(m) * 4);
          done += m;
        };
        for (int pos = 0; rc == 0 && pos < n; pos += stream_n) {
          const int c = std::min(stream_n, n - pos);
          int m = 0;
          for (int i = 0; i < c; ++i) chunk[i] = chunk[size_t(c) + i] = static_cast<float>(mix.samples[pos + i]) / 32768.0f;
          if ((rc = ws_engine_stream_push(st, chunk.data(), c, got.data(), cap, &m)) == 0) take(m);
          stream_launches += ws_engine_info(engine, "n_launches"), ++stream_pushes;
        }
        if (rc == 0) {
          int m = 0;
          if ((rc = ws_engine_stream_flush(st, got.data(), cap, &m)) == 0) take(m);
          stream_launches += ws_engine_info(engine, "n_launches");
        }
        ws_engine_stream_close(st);
      } else if (chunked) {
        // the rows of ws_engine_forward_pcm16, the mixture once: scaled to [-1, 1], one enrollment row per target speaker
        std::vector<float> m(n), enr(size_t(2) * n_enroll);
        for (int i = 0; i < n; ++i) m[i] = static_cast<float>(mix.samples[i]) / 32768.0f;
        for (int i = 0; i < n_enroll; ++i) {
          enr[i] = static_cast<float>(s1.samples[i]) / 32768.0f;
          enr[size_t(n_enroll) + i] = static_cast<float>(s2.samples[i]) / 32768.0f;
        }
        rc = live ? run_live(m.data(), n, enr.data(), n_enroll, out.data())
                  : ws_engine_separate_long(engine, m.data(), n, 2, enr.data(), WS_ENROLL_WAVE, n_enroll, nullptr, window, overlap,
                                            chunk_rows, out.data());
      } else {
        rc = ws_engine_forward_pcm16(engine, mix.samples.data(), n, s1.samples.data(), s2.samples.data(), n_enroll, out.data());
      }
      if (rc != 0) {
        fail(w[0] + ": " + ws_engine_last_error());
        break;
      }
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      const double audio_ms = 1000.0 * n / out_rate;
      if (write_out && (!wesep_rt::write_wav(out_dir + "/" + w[0] + "-spk1.wav", out.data(), n, out_rate, &err) ||
                   !wesep_rt::write_wav(out_dir + "/" + w[0] + "-spk2.wav", out.data() + n, n, out_rate, &err))) {
        fail(err);
        break;
      }
      if (!dry && raw_out) {
        for (int k = 0; k < 2; ++k) {
          FILE* f = fopen((out_dir + "/" + w[0] + "-spk" + std::to_string(k + 1) + ".f32").c_str(), "wb");
          if (!f || fwrite(out.data() + size_t(k) * n, 4, n, f) != size_t(n)) fail("cannot write raw output");
          if (f) fclose(f);
        }
      }
      std::lock_guard<std::mutex> l(io_mu);
      if (streamed)
        printf("process: %s RTF: %.4f (%lld pushes of %d samples, %lld launches, %lld bytes of stream state)%s\n", w[0].c_str(),
               ms / audio_ms, stream_pushes, stream_samples, stream_launches, ws_engine_info(engine, "stream_state_bytes"),
               dry ? " [dry run]" : "");
      else if (live)
        printf("process: %s RTF: %.4f (%lld pushes of %d samples: %lld windows in %lld groups, %lld launches, %lld bytes of live state)%s\n",
               w[0].c_str(), ms / audio_ms, live_pushes, live_n, live_windows, live_groups, live_launches,
               ws_engine_info(engine, "live_state_bytes"), dry ? " [dry run]" : "");
      else if (chunked)
        printf("process: %s RTF: %.4f (%lld windows in %lld forwards: %lld launches, %lld MiB arena)%s\n", w[0].c_str(), ms / audio_ms,
               plain_launches >= 0 ? long_w : ws_engine_info(engine, "long_windows"),
               plain_launches >= 0 ? long_f : ws_engine_info(engine, "long_forwards"),
               plain_launches >= 0 ? plain_launches : ws_engine_info(engine, "n_launches"),
               ws_engine_info(engine, "arena_bytes") >> 20, dry ? " [dry run]" : "");
      else
        printf("process: %s RTF: %.4f (%lld launches, %lld MiB arena)%s\n", w[0].c_str(), ms / audio_ms,
               plain_launches >= 0 ? plain_launches : ws_engine_info(engine, "n_launches"), ws_engine_info(engine, "arena_bytes") >> 20, dry ? " [dry run]" : "");
      if (ws_engine_info(engine, "cluster_fallbacks") > fallbacks_seen) {
        fallbacks_seen = ws_engine_info(engine, "cluster_fallbacks");
        printf("note: %s: a cluster recurrence timed out (GPU shared); recomputed by the streaming kernels\n", w[0].c_str());
      }
      total_audio_ms += audio_ms;
      total_busy_ms += ms;
    }
    ws_engine_destroy(engine);
  };
  const auto wall0 = std::chrono::steady_clock::now();
  std::vector<std::thread> pool;
  for (int j = 1; j < jobs; ++j) pool.emplace_back(worker, j);
  worker(0);
  for (auto& t : pool) t.join();
  if (failed) return die(first_error);
  const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  // with one job this is the reference tool's total (engine time only); with more, wall time is what counts
  const double taken = jobs == 1 ? total_busy_ms : wall_ms;
  printf("Total: process %.0fms audio taken %.0fms.\nRTF: %.4f\n", total_audio_ms, taken,
         total_audio_ms > 0 ? taken / total_audio_ms : 0.0);
  return 0;
}
