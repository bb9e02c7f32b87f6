"""ctypes binding of the native runtime (include/wesep_engine.h, runtime/libwesep_engine.so): what a Python caller
(tests, `wesep_amd.bin.infer --engine`) uses; C++ callers link the library directly (runtime/separate_main.cc)."""
import ctypes as C
import os

import numpy as np

from ._lib import WesepHipError

ENGINE_ABI_VERSION = 2
DRY_RUN = 1
ENROLL_EMBEDDING, ENROLL_FBANK, ENROLL_WAVE = 0, 1, 2
ENROLL_SPEAKER = 3      # [R, E]: what Engine.embed returned (joint containers)
LIB_PATH = os.environ.get("WESEP_ENGINE_LIB") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "runtime", "libwesep_engine.so")
SYMBOLS = ("ws_engine_abi_version", "ws_engine_last_error", "ws_engine_create", "ws_engine_destroy", "ws_engine_info",
           "ws_engine_separate", "ws_engine_separate_ragged", "ws_engine_forward_pcm16", "ws_engine_embed",
           "ws_engine_separate_long", "ws_engine_stream_open", "ws_engine_stream_push", "ws_engine_stream_flush",
           "ws_engine_stream_reset", "ws_engine_stream_close", "ws_engine_pool_open", "ws_engine_pool_attach",
           "ws_engine_pool_push", "ws_engine_pool_flush", "ws_engine_pool_detach", "ws_engine_pool_close",
           "ws_engine_stream_open_ex", "ws_engine_pool_open_ex", "ws_engine_resample", "ws_engine_separate_rate",
           "ws_engine_rate_stream_open", "ws_engine_rate_stream_push", "ws_engine_rate_stream_flush",
           "ws_engine_rate_stream_reset", "ws_engine_rate_stream_close", "ws_engine_rate_stream_push_cap",
           "ws_engine_rate_pool_open", "ws_engine_rate_pool_attach", "ws_engine_rate_pool_push", "ws_engine_rate_pool_push_cap",
           "ws_engine_rate_pool_flush", "ws_engine_rate_pool_detach", "ws_engine_rate_pool_close",
           "ws_engine_live_open", "ws_engine_live_push", "ws_engine_live_flush", "ws_engine_live_reset", "ws_engine_live_close",
           "ws_engine_live_pool_open", "ws_engine_live_pool_attach", "ws_engine_live_pool_push", "ws_engine_live_pool_flush",
           "ws_engine_live_pool_detach", "ws_engine_live_pool_close",
           "ws_engine_live_pool_store", "ws_engine_live_pool_run", "ws_engine_live_pool_due",
           "ws_engine_tail_pool_open", "ws_engine_tail_pool_attach", "ws_engine_tail_pool_push", "ws_engine_tail_pool_tick",
           "ws_engine_tail_pool_flush", "ws_engine_tail_pool_detach", "ws_engine_tail_pool_close",
           "ws_engine_rate_tail_pool_open", "ws_engine_rate_tail_pool_attach", "ws_engine_rate_tail_pool_cap", "ws_engine_rate_tail_pool_room",
           "ws_engine_rate_tail_pool_push", "ws_engine_rate_tail_pool_tick", "ws_engine_rate_tail_pool_flush",
           "ws_engine_rate_tail_pool_detach", "ws_engine_rate_tail_pool_close")
STREAM_FLUSH_CAP = 160  # WS_STREAM_FLUSH_CAP
STREAM_BLOCK_KERNEL = 1  # WS_STREAM_BLOCK_KERNEL: every block of a stream / pool group as one entry-point call
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WesepHipError(f"{LIB_PATH} is missing: run `python -m wesep_amd.build` (needs hipcc)")
        l = C.CDLL(LIB_PATH)
        l.ws_engine_abi_version.restype = C.c_int
        l.ws_engine_last_error.restype = C.c_char_p
        l.ws_engine_create.restype = C.c_int
        l.ws_engine_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.ws_engine_destroy.restype = None
        l.ws_engine_destroy.argtypes = [C.c_void_p]
        l.ws_engine_info.restype = C.c_longlong
        l.ws_engine_info.argtypes = [C.c_void_p, C.c_char_p]
        l.ws_engine_separate.restype = C.c_int
        l.ws_engine_separate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p]
        l.ws_engine_separate_ragged.restype = C.c_int
        l.ws_engine_separate_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_int, C.c_void_p, C.c_void_p]
        l.ws_engine_forward_pcm16.restype = C.c_int
        l.ws_engine_forward_pcm16.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p]
        l.ws_engine_embed.restype = C.c_int
        l.ws_engine_embed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.ws_engine_separate_long.restype = C.c_int
        l.ws_engine_separate_long.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        l.ws_engine_stream_open.restype = C.c_int
        l.ws_engine_stream_open.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.ws_engine_stream_push.restype = C.c_int
        l.ws_engine_stream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_stream_flush.restype = C.c_int
        l.ws_engine_stream_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_stream_reset.restype = C.c_int
        l.ws_engine_stream_reset.argtypes = [C.c_void_p]
        l.ws_engine_stream_close.restype = None
        l.ws_engine_stream_close.argtypes = [C.c_void_p]
        l.ws_engine_pool_open.restype = C.c_int
        l.ws_engine_pool_open.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.ws_engine_pool_attach.restype = C.c_int
        l.ws_engine_pool_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_pool_push.restype = C.c_int
        l.ws_engine_pool_push.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        l.ws_engine_pool_flush.restype = C.c_int
        l.ws_engine_pool_flush.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_pool_detach.restype = C.c_int
        l.ws_engine_pool_detach.argtypes = [C.c_void_p, C.c_int]
        l.ws_engine_stream_open_ex.restype = C.c_int
        l.ws_engine_stream_open_ex.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint,
                                               C.POINTER(C.c_void_p)]
        l.ws_engine_pool_open_ex.restype = C.c_int
        l.ws_engine_pool_open_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_void_p)]
        l.ws_engine_pool_close.restype = None
        l.ws_engine_pool_close.argtypes = [C.c_void_p]
        l.ws_engine_resample.restype = C.c_int
        l.ws_engine_resample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_int)]
        l.ws_engine_separate_rate.restype = C.c_int
        l.ws_engine_separate_rate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p]
        l.ws_engine_rate_stream_open.restype = C.c_int
        l.ws_engine_rate_stream_open.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint,
                                                 C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.ws_engine_rate_stream_push.restype = C.c_int
        l.ws_engine_rate_stream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_rate_stream_flush.restype = C.c_int
        l.ws_engine_rate_stream_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_rate_stream_reset.restype = C.c_int
        l.ws_engine_rate_stream_reset.argtypes = [C.c_void_p]
        l.ws_engine_rate_stream_close.restype = None
        l.ws_engine_rate_stream_close.argtypes = [C.c_void_p]
        l.ws_engine_rate_stream_push_cap.restype = C.c_int
        l.ws_engine_rate_stream_push_cap.argtypes = [C.c_void_p, C.c_int]
        l.ws_engine_rate_pool_open.restype = C.c_int
        l.ws_engine_rate_pool_open.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.ws_engine_rate_pool_attach.restype = C.c_int
        l.ws_engine_rate_pool_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_rate_pool_push.restype = C.c_int
        l.ws_engine_rate_pool_push.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        l.ws_engine_rate_pool_push_cap.restype = C.c_int
        l.ws_engine_rate_pool_push_cap.argtypes = [C.c_void_p, C.c_int, C.c_int]
        l.ws_engine_rate_pool_flush.restype = C.c_int
        l.ws_engine_rate_pool_flush.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_rate_pool_detach.restype = C.c_int
        l.ws_engine_rate_pool_detach.argtypes = [C.c_void_p, C.c_int]
        l.ws_engine_rate_pool_close.restype = None
        l.ws_engine_rate_pool_close.argtypes = [C.c_void_p]
        l.ws_engine_live_open.restype = C.c_int
        l.ws_engine_live_open.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_void_p)]
        l.ws_engine_live_push.restype = C.c_int
        l.ws_engine_live_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_live_flush.restype = C.c_int
        l.ws_engine_live_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_live_reset.restype = C.c_int
        l.ws_engine_live_reset.argtypes = [C.c_void_p]
        l.ws_engine_live_close.restype = None
        l.ws_engine_live_close.argtypes = [C.c_void_p]
        l.ws_engine_live_pool_open.restype = C.c_int
        l.ws_engine_live_pool_open.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.ws_engine_live_pool_attach.restype = C.c_int
        l.ws_engine_live_pool_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        l.ws_engine_live_pool_push.restype = C.c_int
        l.ws_engine_live_pool_push.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        l.ws_engine_live_pool_flush.restype = C.c_int
        l.ws_engine_live_pool_flush.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_live_pool_store.restype = C.c_int
        l.ws_engine_live_pool_store.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.ws_engine_live_pool_run.restype = C.c_int
        l.ws_engine_live_pool_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.ws_engine_live_pool_due.restype = C.c_int
        l.ws_engine_live_pool_due.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        l.ws_engine_live_pool_detach.restype = C.c_int
        l.ws_engine_live_pool_detach.argtypes = [C.c_void_p, C.c_int]
        l.ws_engine_live_pool_close.restype = None
        l.ws_engine_live_pool_close.argtypes = [C.c_void_p]
        l.ws_engine_tail_pool_open.restype = C.c_int
        l.ws_engine_tail_pool_open.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.ws_engine_tail_pool_attach.restype = C.c_int
        l.ws_engine_tail_pool_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        l.ws_engine_tail_pool_push.restype = C.c_int
        l.ws_engine_tail_pool_push.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.ws_engine_tail_pool_tick.restype = C.c_int
        l.ws_engine_tail_pool_tick.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.ws_engine_tail_pool_flush.restype = C.c_int
        l.ws_engine_tail_pool_flush.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_tail_pool_detach.restype = C.c_int
        l.ws_engine_tail_pool_detach.argtypes = [C.c_void_p, C.c_int]
        l.ws_engine_tail_pool_close.restype = None
        l.ws_engine_tail_pool_close.argtypes = [C.c_void_p]
        l.ws_engine_rate_tail_pool_open.restype = C.c_int
        l.ws_engine_rate_tail_pool_open.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                    C.POINTER(C.c_void_p)]
        l.ws_engine_rate_tail_pool_attach.restype = C.c_int
        l.ws_engine_rate_tail_pool_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_rate_tail_pool_cap.restype = C.c_int
        l.ws_engine_rate_tail_pool_cap.argtypes = [C.c_void_p, C.c_int]
        l.ws_engine_rate_tail_pool_room.restype = C.c_int
        l.ws_engine_rate_tail_pool_room.argtypes = [C.c_void_p, C.c_int]
        l.ws_engine_rate_tail_pool_push.restype = C.c_int
        l.ws_engine_rate_tail_pool_push.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.ws_engine_rate_tail_pool_tick.restype = C.c_int
        l.ws_engine_rate_tail_pool_tick.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.ws_engine_rate_tail_pool_flush.restype = C.c_int
        l.ws_engine_rate_tail_pool_flush.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.ws_engine_rate_tail_pool_detach.restype = C.c_int
        l.ws_engine_rate_tail_pool_detach.argtypes = [C.c_void_p, C.c_int]
        l.ws_engine_rate_tail_pool_close.restype = None
        l.ws_engine_rate_tail_pool_close.argtypes = [C.c_void_p]
        if l.ws_engine_abi_version() != ENGINE_ABI_VERSION:
            raise WesepHipError("libwesep_engine.so ABI version mismatch; rebuild")
        _lib = l
    return _lib


def _check(rc, what):
    if rc != 0:
        raise WesepHipError(f"{what} failed (rc={rc}): {lib().ws_engine_last_error().decode('utf-8', 'replace')}")


def _quiesce_torch():
    """The engine launches on its own HIP stream.  Kernels of this library running concurrently on ANOTHER stream
    disturb FFT-type kernels (profiles/r02_kernel_race.md: engines sharing a GPU therefore take turns inside
    libwesep_engine.so); a Python process that also drives torch work on the same GPU gets the same guarantee here:
    whatever torch has in flight finishes before the engine starts."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()


def pack_rows(rows):
    """List of R float arrays [n_r, ...] with equal trailing dimensions -> (zero-filled [R, max n_r, ...] float32, int32 [R]
    of the n_r): the rectangle and the length table of a ragged call."""
    rows = [np.ascontiguousarray(x, dtype=np.float32) for x in rows]
    if not rows or any(x.ndim < 1 or x.shape[1:] != rows[0].shape[1:] for x in rows):
        raise ValueError("pack_rows: a non-empty list of arrays with equal trailing dimensions")
    lengths = np.array([x.shape[0] for x in rows], dtype=np.int32)
    out = np.zeros((len(rows), int(lengths.max())) + rows[0].shape[1:], dtype=np.float32)
    for r, x in enumerate(rows):
        out[r, :x.shape[0]] = x
    return out, lengths


def frames_of(lengths, hop=128):
    """Valid STFT frames of rows with `lengths` samples (centred framing: 1 + n // hop) -- the table the engine and
    BSRNN.forward(lengths=) hand to the length-aware kernels."""
    return 1 + np.asarray(lengths, dtype=np.int64) // hop


def long_windows(n, S, O):
    """Starts of the windows that ws_engine_separate_long cuts a recording of n samples into (window S, overlap O with
    0 <= O <= S // 2, hop S - O): [0] when n <= S (one window [0, n)), else 1 + ceil((n - S) / hop) windows of exactly S
    samples at w * hop, the last one aligned to the end (n - S)."""
    n, S, O = int(n), int(S), int(O)
    if n < 1 or S < 1 or O < 0 or O > S // 2:
        raise ValueError(f"long_windows: n = {n}, window = {S}, overlap = {O} (0 <= overlap <= window // 2)")
    if n <= S:
        return [0]
    H = S - O
    W = 1 + -(-(n - S) // H)
    return [min(w * H, n - S) for w in range(W)]


def _enroll_rows(enrolls, kind, lengths):
    """(rectangle, row pitch, int32 length table or None) of a list / array of enrollments for the C ABI"""
    fixed = kind in (ENROLL_EMBEDDING, ENROLL_SPEAKER)
    if isinstance(enrolls, (list, tuple)) and not fixed and lengths is None:
        enroll, elen = pack_rows(enrolls)
        lengths = elen if len(set(elen.tolist())) > 1 else None
    else:
        enroll = np.ascontiguousarray(enrolls, dtype=np.float32)
    if lengths is not None:
        if fixed:
            raise ValueError("embeddings have no lengths")
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        if lengths.shape != (enroll.shape[0],):
            raise ValueError("one enrollment length per row")
    return enroll, (0 if fixed else enroll.shape[1]), lengths


class Engine:
    """One loaded model on one GPU.  `dry_run=True` needs no GPU: validates the container and every launch's
    argument contract, computes nothing."""

    def __init__(self, weights_path, device=0, dry_run=False):
        self._h = C.c_void_p()
        _check(lib().ws_engine_create(os.fsencode(weights_path), device, DRY_RUN if dry_run else 0, C.byref(self._h)),
               "ws_engine_create")

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.ws_engine_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass

    def info(self, key):
        return int(lib().ws_engine_info(self._h, key.encode()))

    def separate(self, mix, enroll, kind):
        """mix [R, T] float32; enroll: [R, E] (ENROLL_EMBEDDING), [R, Te, F] (ENROLL_FBANK) or [R, Tw]
        (ENROLL_WAVE) -> est [R, T] float32 (numpy, host)."""
        mix = np.ascontiguousarray(mix, dtype=np.float32)
        enroll = np.ascontiguousarray(enroll, dtype=np.float32)
        R, T = mix.shape
        if enroll.shape[0] != R:
            raise ValueError("one enrollment per mixture row")
        est = np.zeros((R, T), dtype=np.float32)
        length = 0 if kind == ENROLL_EMBEDDING else enroll.shape[1]
        _quiesce_torch()
        _check(lib().ws_engine_separate(self._h, mix.ctypes.data, R, T, enroll.ctypes.data, kind, length,
                                        est.ctypes.data), "ws_engine_separate")
        return est

    def separate_ragged(self, mixes, enrolls, kind):
        """Utterances of different lengths in one forward (pBSRNN and TF-GridNet containers): mixes: list of R float32 [T_r]; enrolls: list
        of R arrays -- [E] (ENROLL_EMBEDDING), [Te_r, F] (ENROLL_FBANK) or [Tw_r] (ENROLL_WAVE) -> list of R float32 [T_r].
        Every estimate is what separate() returns for that utterance alone (include/wesep_engine.h,
        ws_engine_separate_ragged)."""
        mixes, enrolls = pack_rows(mixes), pack_rows(enrolls)
        mix, lengths = mixes
        enroll, elen = enrolls
        R, T = mix.shape
        if enroll.shape[0] != R:
            raise ValueError("one enrollment per mixture row")
        est = np.zeros((R, T), dtype=np.float32)
        fixed = kind == ENROLL_EMBEDDING
        if fixed and len(set(elen.tolist())) != 1:
            raise ValueError("fixed embeddings have one size")
        _quiesce_torch()
        _check(lib().ws_engine_separate_ragged(self._h, mix.ctypes.data, R, T, lengths.ctypes.data, enroll.ctypes.data, kind,
                                               0 if fixed else enroll.shape[1], None if fixed else elen.ctypes.data,
                                               est.ctypes.data), "ws_engine_separate_ragged")
        return [est[r, :n].copy() for r, n in enumerate(lengths.tolist())]

    def embed(self, enroll, kind, lengths=None):
        """The speaker stage alone (joint containers): enroll [R, Te, F] (ENROLL_FBANK) or [R, Tw] (ENROLL_WAVE), or a list
        of R such rows of different lengths; lengths: valid frames / samples per row of a rectangle -> [R, E] float32, the
        encoder's embedding before SpeakerTransform.  separate(mix, emb, ENROLL_SPEAKER) with the same R returns bit for
        bit what separate(mix, enroll, kind) does, without running the encoder again."""
        enroll, pitch, lengths = _enroll_rows(enroll, kind, lengths)
        E = self.info("spk_emb_dim")
        emb = np.zeros((enroll.shape[0], E if E > 0 else 256), dtype=np.float32)
        _quiesce_torch()
        _check(lib().ws_engine_embed(self._h, enroll.ctypes.data, kind, enroll.shape[0], pitch,
                                     None if lengths is None else lengths.ctypes.data, emb.ctypes.data), "ws_engine_embed")
        return emb

    def separate_long(self, mix, enrolls, kind, window, overlap, max_rows=8):
        """One long mixture [n] and K enrollments (an array as in separate(), or a list of rows of different lengths) ->
        [K, n] float32: the mixture as overlapping windows (long_windows(n, window, overlap)) through the separator,
        max_rows rows per forward, cross-faded on the device; the speaker stage runs once (include/wesep_engine.h,
        ws_engine_separate_long)."""
        mix = np.ascontiguousarray(mix, dtype=np.float32)
        if mix.ndim != 1:
            raise ValueError("separate_long: one mixture [n]")
        enroll, pitch, lengths = _enroll_rows(enrolls, kind, None)
        K, n = enroll.shape[0], mix.shape[0]
        est = np.zeros((K, n), dtype=np.float32)
        _quiesce_torch()
        _check(lib().ws_engine_separate_long(self._h, mix.ctypes.data, n, K, enroll.ctypes.data, kind, pitch,
                                             None if lengths is None else lengths.ctypes.data, int(window), int(overlap),
                                             int(max_rows), est.ctypes.data), "ws_engine_separate_long")
        return est

    def live(self, enrolls, kind, window, overlap, max_rows=8):
        """A live handle on ANY container: separate_long's windows run as their samples arrive.  enrolls as in
        separate_long() (K of them); the speaker stage runs once, here.  push() takes packets of any size and returns the
        samples that became final, flush() the rest; their concatenation is separate_long(mix, enrolls, kind, window,
        overlap, max_rows) -- bit for bit with max_rows = 1.  Latency: window .. window + hop samples.  Close the handle
        before the engine."""
        return EngineLive(self, enrolls, kind, window, overlap, max_rows)

    def live_pool(self, slots, K, window, overlap, max_rows=8):
        """A pool of `slots` independent live recordings on ANY container, K targets each: every window that one push
        completes, in whatever slot, goes through the separator in the same forwards (at most max_rows rows each).  Per slot
        the outputs are those of live() / separate_long() on that slot's audio -- bit for bit with max_rows = 1.  Close the
        pool before the engine."""
        return LivePool(self, slots, K, window, overlap, max_rows)

    def tail_pool(self, slots, K, window, fade, warm=None, max_rows=8):
        """A pool of `slots` independent live recordings on ANY container, K targets each, separated on their TRAILING windows:
        push() only stores audio; tick() runs the window of the newest `window` samples of every slot that has enough new audio
        and returns the newest part of it, cross-faded over `fade` samples into what the last window held back.  Latency: the
        tick period plus the fade; price: one full window a slot a tick.  warm: the samples a slot needs before its first
        window (None: window).  The output is a rule of its own (include/wesep_engine.h), not separate_long().  Close the pool
        before the engine."""
        return TailPool(self, slots, K, window, fade, warm, max_rows)

    def tail(self, enrolls, kind, window, fade, warm=None, max_rows=8):
        """A one-slot tail pool for one recording: push(chunk) appends and ticks, and returns [K, m] (m = 0 while the slot does not
        fire); flush() returns the rest.  enrolls as in separate_long() (K of them)."""
        return EngineTail(self, enrolls, kind, window, fade, warm, max_rows)

    def rate_tail_pool(self, slots, K, window, fade, rates, warm=None, max_rows=8):
        """tail_pool() whose slots carry and return audio at their own sample rates (`rates`: the rates it will accept; the
        container's own always is).  window, fade and warm stay samples at the container's rate (warm None: 3/4 of the window -- the
        filters' look-ahead keeps a resampled slot below a whole window before its first firing).  A tick is the tail pool's plus
        three launches, whatever the number of firing slots and of distinct rates.  TF-GridNet containers are refused.  Close
        the pool before the engine."""
        return RateTailPool(self, slots, K, window, fade, rates, warm, max_rows)

    def rate_tail(self, enrolls, kind, window, fade, sample_rate, enroll_rate=0, warm=None, max_rows=8):
        """A one-slot rate tail pool for one recording at sample_rate: push(chunk) appends and ticks, and returns [K, m] at
        sample_rate; flush() returns the rest.  Over its life it returns exactly the samples pushed."""
        return EngineRateTail(self, enrolls, kind, window, fade, sample_rate, enroll_rate, warm, max_rows)

    def stream(self, rows, enroll, kind, max_chunk_frames=64, block_kernel=False):
        """A stream of `rows` rows on a causal cLN Conv-TasNet / SpEx+ container (info("streaming") == 1): enroll as in
        separate(); the speaker stage runs once, here.  Close the stream before the engine.  block_kernel=True
        (WS_STREAM_BLOCK_KERNEL): every block is one entry-point call."""
        return EngineStream(self, rows, enroll, kind, max_chunk_frames, flags=STREAM_BLOCK_KERNEL if block_kernel else 0)

    def stream_pool(self, slots, max_chunk_frames=64, block_kernel=False):
        """A pool of `slots` independent streams on a causal cLN Conv-TasNet / SpEx+ container: each slot at its own
        position, packets of any size, one launch chain per push whatever the number of slots in it.  Close the pool before
        the engine.  block_kernel=True (WS_STREAM_BLOCK_KERNEL): every block is one entry-point call."""
        return StreamPool(self, slots, max_chunk_frames, flags=STREAM_BLOCK_KERNEL if block_kernel else 0)

    def resample(self, x, rate_in, rate_out):
        """x [R, n] float32 at rate_in -> [R, ceil(U n / D)] float32 at rate_out (numpy, host): the device resampler of
        wesep_amd.resample through the engine -- one upload, one launch, one download (ws_engine_resample)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] < 1:
            raise ValueError("Engine.resample: x is [R, n] with n >= 1")
        R, n = x.shape
        cap = -(-int(rate_out) * n // int(rate_in)) if rate_in > 0 and rate_out > 0 else 1      # ceil(U n / D); bad rates: refused below
        y, m = np.zeros((R, max(cap, 1)), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_resample(self._h, x.ctypes.data, R, n, int(rate_in), int(rate_out), y.ctypes.data, cap, C.byref(m)),
               "ws_engine_resample")
        return y[:, :m.value]

    def separate_rate(self, mix, enroll, kind, sample_rate, enroll_rate=0):
        """separate() on audio at the caller's rate: mix [R, T] at sample_rate -> est [R, T] at sample_rate; an ENROLL_WAVE
        enrollment is at enroll_rate (0: the container's).  Resample in, separate as it is, resample back and crop; with
        every rate equal to the container's it IS separate() (ws_engine_separate_rate)."""
        mix = np.ascontiguousarray(mix, dtype=np.float32)
        enroll = np.ascontiguousarray(enroll, dtype=np.float32)
        R, T = mix.shape
        if enroll.shape[0] != R:
            raise ValueError("one enrollment per mixture row")
        est = np.zeros((R, T), dtype=np.float32)
        length = 0 if kind in (ENROLL_EMBEDDING, ENROLL_SPEAKER) else enroll.shape[1]
        _quiesce_torch()
        _check(lib().ws_engine_separate_rate(self._h, mix.ctypes.data, R, T, int(sample_rate), enroll.ctypes.data, kind, length,
                                             int(enroll_rate), est.ctypes.data), "ws_engine_separate_rate")
        return est

    def rate_pool(self, slots, rates, max_chunk_frames=64, max_push=4800, block_kernel=False):
        """A stream pool whose slots have their own sample rates (`rates`: the rates it will accept; the container's own always
        is): one launch chain per push whatever the number of slots and distinct rates in it.  Close it before the engine."""
        return RatePool(self, slots, rates, max_chunk_frames, max_push, flags=STREAM_BLOCK_KERNEL if block_kernel else 0)

    def rate_stream(self, rows, enroll, kind, sample_rate, enroll_rate=0, max_chunk_frames=64, max_push=4800, block_kernel=False):
        """stream() whose pushes carry and return samples at sample_rate: two stateful resamplers around the stream, all on
        the device, one host synchronisation per push.  max_push: the samples a row the resamplers' buffers are sized for (a
        longer push is taken in pieces).  Close the stream before the engine."""
        return EngineRateStream(self, rows, enroll, kind, sample_rate, enroll_rate, max_chunk_frames, max_push,
                                flags=STREAM_BLOCK_KERNEL if block_kernel else 0)

    def forward_pcm16(self, mix, spk1, spk2):
        """int16 [n], int16 [n_enroll] x 2 -> float32 [2, n] in [-1, 1] (SeparateEngine::ForwardFunc)."""
        mix, spk1, spk2 = (np.ascontiguousarray(x, dtype=np.int16) for x in (mix, spk1, spk2))
        n_enroll = min(spk1.shape[0], spk2.shape[0])
        out = np.zeros((2, mix.shape[0]), dtype=np.float32)
        _quiesce_torch()
        _check(lib().ws_engine_forward_pcm16(self._h, mix.ctypes.data, mix.shape[0], spk1.ctypes.data,
                                             spk2.ctypes.data, n_enroll, out.ctypes.data), "ws_engine_forward_pcm16")
        return out


def stream_push_cap(n, L):
    """WS_STREAM_PUSH_CAP: samples a row that a push of n samples can emit at most."""
    return (n // (L // 2) + 1) * (L // 2)


class EngineStream:
    """ws_engine_stream_* (include/wesep_engine.h): audio in as it arrives, the samples that became final out.  The
    concatenation of every push() and the flush() is the model-output part of Engine.separate's row."""

    def __init__(self, engine, rows, enroll, kind, max_chunk_frames=64, flags=0):
        self._h, self._engine, self.rows = C.c_void_p(), engine, int(rows)      # (the engine must outlive the stream)
        enroll = np.ascontiguousarray(enroll, dtype=np.float32)
        if enroll.shape[0] != self.rows:
            raise ValueError("one enrollment per stream row")
        length = 0 if kind in (ENROLL_EMBEDDING, ENROLL_SPEAKER) else enroll.shape[1]
        _quiesce_torch()
        if flags:
            _check(lib().ws_engine_stream_open_ex(engine._h, self.rows, enroll.ctypes.data, kind, length, int(max_chunk_frames),
                                                  int(flags), C.byref(self._h)), "ws_engine_stream_open_ex")
        else:
            _check(lib().ws_engine_stream_open(engine._h, self.rows, enroll.ctypes.data, kind, length, int(max_chunk_frames),
                                               C.byref(self._h)), "ws_engine_stream_open")
        self._L = engine.info("L")

    def _out(self, buf, m):
        return buf[:self.rows * m].reshape(self.rows, m).copy()

    def push(self, chunk, est_cap=None):
        """chunk [rows, n], n >= 1 -> [rows, m] float32, the samples that became final (m = 0 while no frame is complete).
        est_cap: samples a row the output buffer holds (default: what always suffices)."""
        chunk = np.ascontiguousarray(chunk, dtype=np.float32)
        if chunk.ndim != 2 or chunk.shape[0] != self.rows:
            raise ValueError(f"EngineStream.push: chunk is {chunk.shape}, expected [{self.rows}, n >= 1]")
        n = chunk.shape[1]
        cap = stream_push_cap(n, self._L) if est_cap is None else int(est_cap)
        buf, m = np.zeros(self.rows * max(cap, 1), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_stream_push(self._h, chunk.ctypes.data, n, buf.ctypes.data, cap, C.byref(m)), "ws_engine_stream_push")
        return self._out(buf, m.value)

    def flush(self, est_cap=STREAM_FLUSH_CAP):
        """The end of the stream: the remaining frames on the zero-extended pending samples, then the overlap-add carry."""
        buf, m = np.zeros(self.rows * max(int(est_cap), 1), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_stream_flush(self._h, buf.ctypes.data, int(est_cap), C.byref(m)), "ws_engine_stream_flush")
        return self._out(buf, m.value)

    def reset(self):
        """Back to sample 0; the enrollment is kept."""
        _check(lib().ws_engine_stream_reset(self._h), "ws_engine_stream_reset")

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(self._engine, "_h", None):
            _lib.ws_engine_stream_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


def live_push_cap(n, H):
    """WS_LIVE_PUSH_CAP: samples a target that a live push of n samples can emit at most (H = window - overlap)."""
    return (n // H + 1) * H


def live_flush_cap(S, O):
    """WS_LIVE_FLUSH_CAP: samples a target that a live flush can emit at most."""
    return 2 * S - O


def live_group_launches(K, max_rows):
    """WS_LIVE_GROUP_LAUNCHES: what a group of windows adds to its forwards' entry-point calls."""
    return 2 + (1 if K > 1 and max_rows > 1 else 0)


class EngineLive:
    """ws_engine_live_* (include/wesep_engine.h): one mixture in as it arrives, K targets out.  The concatenation of every
    push() and the flush() is Engine.separate_long on the concatenated input."""

    def __init__(self, engine, enrolls, kind, window, overlap, max_rows=8):
        self._h, self._engine = C.c_void_p(), engine      # (the engine must outlive the handle)
        enroll, pitch, lengths = _enroll_rows(enrolls, kind, None)
        self.K, self.window, self.overlap, self.max_rows = enroll.shape[0], int(window), int(overlap), int(max_rows)
        _quiesce_torch()
        _check(lib().ws_engine_live_open(engine._h, self.K, enroll.ctypes.data, kind, pitch,
                                         None if lengths is None else lengths.ctypes.data, self.window, self.overlap,
                                         self.max_rows, C.byref(self._h)), "ws_engine_live_open")

    def push(self, chunk, est_cap=None):
        """chunk [n], n >= 1 -> [K, m] float32, the samples that became final (m = 0 while no window became complete).
        est_cap: samples a target the output buffer holds (default: what always suffices)."""
        chunk = np.ascontiguousarray(chunk, dtype=np.float32)
        if chunk.ndim != 1:
            raise ValueError(f"EngineLive.push: chunk is {chunk.shape}, expected [n >= 1]")
        n = chunk.shape[0]
        cap = live_push_cap(n, self.window - self.overlap) if est_cap is None else int(est_cap)
        buf, m = np.zeros((self.K, max(cap, 1)), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_live_push(self._h, chunk.ctypes.data, n, buf.ctypes.data, cap, C.byref(m)), "ws_engine_live_push")
        return buf[:, :m.value].copy()

    def flush(self, est_cap=None):
        """The end of the recording: the end-aligned last window if one is due, then every sample not yet out."""
        cap = live_flush_cap(self.window, self.overlap) if est_cap is None else int(est_cap)
        buf, m = np.zeros((self.K, max(cap, 1)), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_live_flush(self._h, buf.ctypes.data, cap, C.byref(m)), "ws_engine_live_flush")
        return buf[:, :m.value].copy()

    def reset(self):
        """Back to sample 0; the enrollments are kept."""
        _check(lib().ws_engine_live_reset(self._h), "ws_engine_live_reset")

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(self._engine, "_h", None):
            _lib.ws_engine_live_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


LIVE_POOL_ROUND_LAUNCHES = 3        # WS_LIVE_POOL_ROUND_LAUNCHES: the gather, the scatter into the rings and the cross-fade of a round


def live_pool_launches(round_plans):
    """"n_launches" after a live-pool push: round_plans is one list per round of its forwards' rectangular counts."""
    return sum(sum(f) + LIVE_POOL_ROUND_LAUNCHES for f in round_plans) + 1


def live_pool_store_limit(S, H):
    """WS_LIVE_POOL_STORE_LIMIT: a store must leave a slot with fewer pending samples than this."""
    return 2 * S + H


def live_pool_run_cap(S, H):
    """WS_LIVE_POOL_RUN_CAP: samples a target that a live-pool run can emit at most for one slot."""
    return 2 * S + H


class LivePool:
    """ws_engine_live_pool_* (include/wesep_engine.h): many live recordings, the windows that one push completes through the
    same forwards.  Every slot is an EngineLive: the concatenation of what its pushes and its flush return is
    Engine.separate_long on that slot's audio, whatever the other slots were fed in the meantime.  store() / due() / run()
    put the windows on the caller's clock: packets are stored without a launch, and one run works off every complete window
    of every slot in the same forwards, and ends the recordings named final."""

    def __init__(self, engine, slots, K, window, overlap, max_rows=8):
        self._h, self._engine = C.c_void_p(), engine      # (the engine must outlive the pool)
        self.slots, self.K, self.window, self.overlap, self.max_rows = int(slots), int(K), int(window), int(overlap), int(max_rows)
        self._fed = {}                                    # attached, not ended: slot -> [samples fed, windows run]
        _quiesce_torch()
        _check(lib().ws_engine_live_pool_open(engine._h, self.slots, self.K, self.window, self.overlap, self.max_rows,
                                              C.byref(self._h)), "ws_engine_live_pool_open")

    def attach(self, enrolls, kind):
        """K enrollments as in Engine.separate_long() -> the slot they took.  The speaker stage runs here, once."""
        enroll, pitch, lengths = _enroll_rows(enrolls, kind, None)
        if enroll.shape[0] != self.K:
            raise ValueError(f"LivePool.attach: {enroll.shape[0]} enrollments, the pool was opened for K = {self.K}")
        slot = C.c_int(-1)
        _quiesce_torch()
        _check(lib().ws_engine_live_pool_attach(self._h, enroll.ctypes.data, kind, pitch,
                                                None if lengths is None else lengths.ctypes.data, C.byref(slot)),
               "ws_engine_live_pool_attach")
        self._fed[slot.value] = [0, 0]
        return slot.value

    def _windows(self, N):
        """Wr(N) of the emission rule: the windows that are complete after N samples"""
        S, H = self.window, self.window - self.overlap
        return 0 if N < S else 1 + (N - S) // H

    def _emitted(self, Wr):
        """E of the emission rule: the samples before the start of the newest window run"""
        return max(Wr - 1, 0) * (self.window - self.overlap)

    def push(self, chunks, est_cap=None):
        """{slot: chunk [n_slot >= 1]} -> {slot: float32 [K, m_slot]}, the samples of each slot that became final (m = 0 while
        no window of the slot became complete).  est_cap: {slot: samples a target the buffer holds} (default: what suffices)."""
        ids = list(chunks)
        data = [np.ascontiguousarray(chunks[i], dtype=np.float32).reshape(-1) for i in ids]
        n = np.array([x.shape[0] for x in data], dtype=np.int32)
        H = self.window - self.overlap
        caps = np.array([live_push_cap(int(k), H) if est_cap is None else int(est_cap[i]) for i, k in zip(ids, n)], dtype=np.int32)
        bufs = [np.zeros((self.K, max(int(c), 1)), dtype=np.float32) for c in caps]
        A = len(ids)
        slots, m = np.array(ids, dtype=np.int32), np.zeros(max(A, 1), dtype=np.int32)
        cp = (C.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
        ep = (C.c_void_p * max(A, 1))(*[b.ctypes.data for b in bufs])
        _quiesce_torch()
        _check(lib().ws_engine_live_pool_push(self._h, A, slots.ctypes.data, C.cast(cp, C.c_void_p), n.ctypes.data,
                                              C.cast(ep, C.c_void_p), caps.ctypes.data, m.ctypes.data), "ws_engine_live_pool_push")
        for i, k in zip(ids, n):
            f = self._fed[int(i)]
            f[0] += int(k)
            f[1] = self._windows(f[0])
        return {i: b[:, :int(k)].copy() for i, b, k in zip(ids, bufs, m)}

    def store(self, chunks):
        """{slot: chunk [n_slot >= 1]}: the samples wait on the host for the next run.  No launch."""
        ids = list(chunks)
        data = [np.ascontiguousarray(chunks[i], dtype=np.float32).reshape(-1) for i in ids]
        n = np.array([x.shape[0] for x in data], dtype=np.int32)
        A = len(ids)
        slots = np.array(ids, dtype=np.int32)
        cp = (C.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
        _check(lib().ws_engine_live_pool_store(self._h, A, slots.ctypes.data, C.cast(cp, C.c_void_p), n.ctypes.data), "ws_engine_live_pool_store")
        for i, k in zip(ids, n):
            self._fed[int(i)][0] += int(k)

    def due(self):
        """-> (rows_ready, oldest_age): separator rows of the complete windows that no run has taken yet, and the samples the
        slot that waits longest has received since its oldest such window became complete.  No launch, no change of state."""
        rows, age = C.c_longlong(0), C.c_longlong(0)
        _check(lib().ws_engine_live_pool_due(self._h, C.byref(rows), C.byref(age)), "ws_engine_live_pool_due")
        return rows.value, age.value

    def run(self, slots=None, final=(), est_cap=None):
        """Runs every complete window of the named slots in shared forwards and ends the recordings of the slots in `final`
        -> {slot: float32 [K, m_slot]}.  slots=None: every attached slot with a complete window that has not run, and the slots
        in final.  est_cap: {slot: samples a target the buffer holds} (default: exactly what comes out)."""
        final = [int(s) for s in final]
        if slots is None:
            ids = sorted(s for s, (N, Wr) in self._fed.items() if s in final or self._windows(N) > Wr)
        else:
            ids = [int(s) for s in slots]
        ids += [s for s in final if s not in ids]
        if not ids:
            return {}
        A = len(ids)
        fin = np.array([1 if s in final else 0 for s in ids], dtype=np.int32)
        want = []                                         # per slot what comes out: up to the newest window's start, or to the end
        for s in ids:
            N, Wr = self._fed.get(s, (0, 0))
            want.append((N if s in final else self._emitted(self._windows(N))) - self._emitted(Wr))
        caps = np.array([w if est_cap is None else int(est_cap[s]) for s, w in zip(ids, want)], dtype=np.int32)
        bufs = [np.zeros((self.K, max(int(c), 1)), dtype=np.float32) for c in caps]
        arr, m = np.array(ids, dtype=np.int32), np.zeros(A, dtype=np.int32)
        ep = (C.c_void_p * A)(*[b.ctypes.data for b in bufs])
        _quiesce_torch()
        _check(lib().ws_engine_live_pool_run(self._h, A, arr.ctypes.data, fin.ctypes.data, C.cast(ep, C.c_void_p), caps.ctypes.data,
                                             m.ctypes.data), "ws_engine_live_pool_run")
        for s in ids:
            if s in final:
                self._fed.pop(s, None)
            else:
                self._fed[s][1] = self._windows(self._fed[s][0])
        return {i: b[:, :int(k)].copy() for i, b, k in zip(ids, bufs, m)}

    def flush(self, slot, est_cap=None):
        """The end of one slot's recording: the end-aligned last window if one is due, then every sample not yet out."""
        N, Wr = self._fed.get(int(slot), (0, 0))             # (stored audio: more may come out than after pushes alone)
        cap = max(live_flush_cap(self.window, self.overlap), N - self._emitted(Wr)) if est_cap is None else int(est_cap)
        buf, m = np.zeros((self.K, max(cap, 1)), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_live_pool_flush(self._h, int(slot), buf.ctypes.data, cap, C.byref(m)), "ws_engine_live_pool_flush")
        self._fed.pop(int(slot), None)
        return buf[:, :m.value].copy()

    def detach(self, slot):
        """Frees the slot for the next attach."""
        _check(lib().ws_engine_live_pool_detach(self._h, int(slot)), "ws_engine_live_pool_detach")
        self._fed.pop(int(slot), None)

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(self._engine, "_h", None):
            _lib.ws_engine_live_pool_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


TAIL_TICK_LAUNCHES = 2              # WS_TAIL_TICK_LAUNCHES: the gather and the emission of a tick


def tail_launches(forward_plans):
    """"n_launches" after a tail-pool tick (or a flush that runs a window): forward_plans is its forwards' rectangular counts."""
    return sum(forward_plans) + TAIL_TICK_LAUNCHES + 1


class TailPool:
    """ws_engine_tail_pool_* (include/wesep_engine.h): many live recordings separated on their trailing windows, fired by the
    caller's tick.  Per slot the concatenation of what its ticks and its flush return has exactly as many samples as were
    pushed; the rule is restated in tests/emu_tail.py."""

    def __init__(self, engine, slots, K, window, fade, warm=None, max_rows=8):
        self._h, self._engine = C.c_void_p(), engine      # (the engine must outlive the pool)
        self.slots, self.K, self.window, self.fade, self.max_rows = int(slots), int(K), int(window), int(fade), int(max_rows)
        self.warm = self.window if warm is None else int(warm)
        self._live = set()                                # attached and not flushed: what tick(None) names
        _quiesce_torch()
        _check(lib().ws_engine_tail_pool_open(engine._h, self.slots, self.K, self.window, self.fade, self.warm, self.max_rows,
                                              C.byref(self._h)), "ws_engine_tail_pool_open")

    def attach(self, enrolls, kind):
        """K enrollments as in Engine.separate_long() -> the slot they took.  The speaker stage runs here, once."""
        enroll, pitch, lengths = _enroll_rows(enrolls, kind, None)
        if enroll.shape[0] != self.K:
            raise ValueError(f"TailPool.attach: {enroll.shape[0]} enrollments, the pool was opened for K = {self.K}")
        slot = C.c_int(-1)
        _quiesce_torch()
        _check(lib().ws_engine_tail_pool_attach(self._h, enroll.ctypes.data, kind, pitch,
                                                None if lengths is None else lengths.ctypes.data, C.byref(slot)),
               "ws_engine_tail_pool_attach")
        self._live.add(slot.value)
        return slot.value

    def push(self, chunks):
        """{slot: chunk [n_slot >= 1]}: the samples wait on the host for the next tick.  No launch."""
        ids = list(chunks)
        data = [np.ascontiguousarray(chunks[i], dtype=np.float32).reshape(-1) for i in ids]
        n = np.array([x.shape[0] for x in data], dtype=np.int32)
        A = len(ids)
        slots = np.array(ids, dtype=np.int32)
        cp = (C.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
        _check(lib().ws_engine_tail_pool_push(self._h, A, slots.ctypes.data, C.cast(cp, C.c_void_p), n.ctypes.data), "ws_engine_tail_pool_push")

    def tick(self, slots=None, est_cap=None):
        """-> {slot: float32 [K, m_slot]} for the slots that fired.  slots: the slots to name (None: every attached, unflushed
        one).  est_cap: {slot: samples a target the buffer holds} (default: what always suffices, the window)."""
        ids = sorted(self._live) if slots is None else [int(s) for s in slots]
        if not ids:
            return {}
        A = len(ids)
        caps = np.array([self.window if est_cap is None else int(est_cap[i]) for i in ids], dtype=np.int32)
        bufs = [np.zeros((self.K, max(int(c), 1)), dtype=np.float32) for c in caps]
        arr, m = np.array(ids, dtype=np.int32), np.zeros(A, dtype=np.int32)
        ep = (C.c_void_p * A)(*[b.ctypes.data for b in bufs])
        _quiesce_torch()
        _check(lib().ws_engine_tail_pool_tick(self._h, A, arr.ctypes.data, C.cast(ep, C.c_void_p), caps.ctypes.data, m.ctypes.data),
               "ws_engine_tail_pool_tick")
        return {i: b[:, :int(k)].copy() for i, b, k in zip(ids, bufs, m) if int(k) > 0}

    def flush(self, slot, est_cap=None):
        """The end of one slot's recording: one last window if there is new audio (or the slot never fired), else the hold."""
        cap = self.window if est_cap is None else int(est_cap)
        buf, m = np.zeros((self.K, max(cap, 1)), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_tail_pool_flush(self._h, int(slot), buf.ctypes.data, cap, C.byref(m)), "ws_engine_tail_pool_flush")
        self._live.discard(int(slot))
        return buf[:, :m.value].copy()

    def detach(self, slot):
        """Frees the slot for the next attach."""
        _check(lib().ws_engine_tail_pool_detach(self._h, int(slot)), "ws_engine_tail_pool_detach")
        self._live.discard(int(slot))

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(self._engine, "_h", None):
            _lib.ws_engine_tail_pool_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


class EngineTail:
    """Engine.tail(): one recording on a one-slot TailPool.  push() appends and ticks; a chunk that would leave more than one
    window of audio that has not come out is fed in pieces with a tick between them."""

    def __init__(self, engine, enrolls, kind, window, fade, warm=None, max_rows=8):
        enroll, _, _ = _enroll_rows(enrolls, kind, None)
        self.pool = TailPool(engine, 1, enroll.shape[0], window, fade, warm, max_rows)
        self.K, self.window = self.pool.K, self.pool.window
        self.slot = self.pool.attach(enrolls, kind)
        self._waiting = 0                                 # samples pushed that have not come out

    def push(self, chunk):
        """chunk [n], n >= 1 -> [K, m] float32, possibly empty."""
        chunk = np.ascontiguousarray(chunk, dtype=np.float32).reshape(-1)
        parts, at = [np.zeros((self.K, 0), np.float32)], 0
        while at < chunk.shape[0]:
            take = min(chunk.shape[0] - at, self.window - self._waiting)
            if take < 1:
                raise WesepHipError("EngineTail.push: a window of audio is waiting and the slot does not fire (warm exceeds what "
                                    "a window can hold beside the samples that have not come out)")
            self.pool.push({self.slot: chunk[at:at + take]})
            at += take
            self._waiting += take
            got = self.pool.tick([self.slot]).get(self.slot)
            if got is not None:
                parts.append(got)
                self._waiting -= got.shape[1]
        return np.concatenate(parts, axis=1)

    def flush(self):
        return self.pool.flush(self.slot)

    def close(self):
        self.pool.close()


RATE_TAIL_TICK_LAUNCHES = 3         # WS_RATE_TAIL_TICK_LAUNCHES: the gather, the emission and resampler B of a tick


def rate_tail_launches(forward_plans):
    """"n_launches" after a rate-tail-pool tick (or a flush that runs a window): forward_plans is its forwards' rectangular
    counts."""
    return sum(forward_plans) + RATE_TAIL_TICK_LAUNCHES + 1


class RateTailPool:
    """ws_engine_rate_tail_pool_* (include/wesep_engine.h): a TailPool whose slots carry and return audio at their own sample
    rates.  Per slot the concatenation of what its ticks and its flush return has exactly as many samples as were pushed; the
    rule is restated in tests/emu_rate_tail.py."""

    def __init__(self, engine, slots, K, window, fade, rates, warm=None, max_rows=8):
        self._h, self._engine = C.c_void_p(), engine      # (the engine must outlive the pool)
        self.slots, self.K, self.window, self.fade, self.max_rows = int(slots), int(K), int(window), int(fade), int(max_rows)
        self.warm = 3 * self.window // 4 if warm is None else int(warm)    # (a resampled slot never has a whole window before it fires)
        self._live = set()                                # attached and not flushed: what tick(None) names
        rates = np.ascontiguousarray(list(rates), dtype=np.int32)
        _quiesce_torch()
        _check(lib().ws_engine_rate_tail_pool_open(engine._h, self.slots, self.K, self.window, self.fade, self.warm, self.max_rows,
                                                   rates.ctypes.data, len(rates), C.byref(self._h)), "ws_engine_rate_tail_pool_open")

    def attach(self, enrolls, kind, sample_rate, enroll_rate=0):
        """K enrollments as in Engine.separate_long(), the slot's sample rate -> the slot they took.  A waveform enrollment is at
        enroll_rate (0: the container's).  The speaker stage runs here, once."""
        enroll, pitch, lengths = _enroll_rows(enrolls, kind, None)
        if enroll.shape[0] != self.K:
            raise ValueError(f"RateTailPool.attach: {enroll.shape[0]} enrollments, the pool was opened for K = {self.K}")
        slot = C.c_int(-1)
        _quiesce_torch()
        _check(lib().ws_engine_rate_tail_pool_attach(self._h, enroll.ctypes.data, kind, pitch,
                                                     None if lengths is None else lengths.ctypes.data, int(enroll_rate), int(sample_rate),
                                                     C.byref(slot)), "ws_engine_rate_tail_pool_attach")
        self._live.add(slot.value)
        return slot.value

    def cap(self, slot):
        """Samples a target that a tick or the flush of `slot` returns at most (ws_engine_rate_tail_pool_cap)."""
        return int(lib().ws_engine_rate_tail_pool_cap(self._h, int(slot)))

    def room(self, slot):
        """The largest push `slot` takes now, in samples at its rate (0: tick first; ws_engine_rate_tail_pool_room)."""
        return int(lib().ws_engine_rate_tail_pool_room(self._h, int(slot)))

    def push(self, chunks):
        """{slot: chunk [n_slot >= 1] at the slot's rate}: the samples wait on the host for the next tick.  No launch."""
        ids = list(chunks)
        data = [np.ascontiguousarray(chunks[i], dtype=np.float32).reshape(-1) for i in ids]
        n = np.array([x.shape[0] for x in data], dtype=np.int32)
        A = len(ids)
        slots = np.array(ids, dtype=np.int32)
        cp = (C.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
        _check(lib().ws_engine_rate_tail_pool_push(self._h, A, slots.ctypes.data, C.cast(cp, C.c_void_p), n.ctypes.data),
               "ws_engine_rate_tail_pool_push")

    def tick(self, slots=None, est_cap=None):
        """-> {slot: float32 [K, m_slot] at the slot's rate} for the slots that returned samples.  slots: the slots to name
        (None: every attached, unflushed one).  est_cap: {slot: samples a target the buffer holds} (default: cap(slot))."""
        ids = sorted(self._live) if slots is None else [int(s) for s in slots]
        if not ids:
            return {}
        A = len(ids)
        caps = np.array([max(self.cap(i), 0) if est_cap is None else int(est_cap[i]) for i in ids], dtype=np.int32)
        bufs = [np.zeros((self.K, max(int(c), 1)), dtype=np.float32) for c in caps]
        arr, m = np.array(ids, dtype=np.int32), np.zeros(A, dtype=np.int32)
        ep = (C.c_void_p * A)(*[b.ctypes.data for b in bufs])
        _quiesce_torch()
        _check(lib().ws_engine_rate_tail_pool_tick(self._h, A, arr.ctypes.data, C.cast(ep, C.c_void_p), caps.ctypes.data, m.ctypes.data),
               "ws_engine_rate_tail_pool_tick")
        return {i: b[:, :int(k)].copy() for i, b, k in zip(ids, bufs, m) if int(k) > 0}

    def flush(self, slot, est_cap=None):
        """The end of one slot's recording: the last window, resampler B's rest, cropped to the samples pushed."""
        cap = max(self.cap(slot), 0) if est_cap is None else int(est_cap)
        buf, m = np.zeros((self.K, max(cap, 1)), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_rate_tail_pool_flush(self._h, int(slot), buf.ctypes.data, cap, C.byref(m)), "ws_engine_rate_tail_pool_flush")
        self._live.discard(int(slot))
        return buf[:, :m.value].copy()

    def detach(self, slot):
        """Frees the slot for the next attach."""
        _check(lib().ws_engine_rate_tail_pool_detach(self._h, int(slot)), "ws_engine_rate_tail_pool_detach")
        self._live.discard(int(slot))

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(self._engine, "_h", None):
            _lib.ws_engine_rate_tail_pool_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


class EngineRateTail:
    """Engine.rate_tail(): one recording on a one-slot RateTailPool.  push() appends and ticks; a chunk that would leave more
    than one window of audio that has not come out is fed in pieces with a tick between them."""

    def __init__(self, engine, enrolls, kind, window, fade, sample_rate, enroll_rate=0, warm=None, max_rows=8):
        enroll, _, _ = _enroll_rows(enrolls, kind, None)
        self.pool = RateTailPool(engine, 1, enroll.shape[0], window, fade, [int(sample_rate)], warm, max_rows)
        self.K, self.window, self.sample_rate = self.pool.K, self.pool.window, int(sample_rate)
        self.slot = self.pool.attach(enrolls, kind, sample_rate, enroll_rate)

    def push(self, chunk):
        """chunk [n] at sample_rate, n >= 1 -> [K, m] float32 at sample_rate, possibly empty."""
        chunk = np.ascontiguousarray(chunk, dtype=np.float32).reshape(-1)
        parts, at = [np.zeros((self.K, 0), np.float32)], 0
        while at < chunk.shape[0]:
            take = min(chunk.shape[0] - at, self.pool.room(self.slot))
            if take < 1:
                raise WesepHipError("EngineRateTail.push: a window of audio is waiting and the slot does not fire")
            self.pool.push({self.slot: chunk[at:at + take]})
            at += take
            got = self.pool.tick([self.slot]).get(self.slot)
            if got is not None:
                parts.append(got)
        return np.concatenate(parts, axis=1)

    def flush(self):
        return self.pool.flush(self.slot)

    def close(self):
        self.pool.close()


RATE_STREAM_PIECE_LAUNCHES = 2      # WS_RATE_STREAM_PIECE_LAUNCHES: one ws_resample_stream_fwd per resampler that received samples


def separate_rate_launches(mix_resampled, enroll_resampled):
    """WS_SEPARATE_RATE_LAUNCHES: what ws_engine_separate_rate adds to ws_engine_separate's entry-point calls."""
    return 2 * bool(mix_resampled) + bool(enroll_resampled)


class EngineRateStream:
    """ws_engine_rate_stream_* (include/wesep_engine.h): an EngineStream at the caller's sample rate.  The concatenation of
    every push() and the flush() is Engine.resample -> EngineStream (same flags) -> Engine.resample, cropped to the samples
    pushed."""

    def __init__(self, engine, rows, enroll, kind, sample_rate, enroll_rate=0, max_chunk_frames=64, max_push=4800, flags=0):
        self._h, self._engine, self.rows = C.c_void_p(), engine, int(rows)      # (the engine must outlive the stream)
        enroll = np.ascontiguousarray(enroll, dtype=np.float32)
        if enroll.shape[0] != self.rows:
            raise ValueError("one enrollment per stream row")
        length = 0 if kind in (ENROLL_EMBEDDING, ENROLL_SPEAKER) else enroll.shape[1]
        _quiesce_torch()
        _check(lib().ws_engine_rate_stream_open(engine._h, self.rows, enroll.ctypes.data, kind, length, int(enroll_rate),
                                                int(max_chunk_frames), int(flags), int(sample_rate), int(max_push),
                                                C.byref(self._h)), "ws_engine_rate_stream_open")

    def push_cap(self, n):
        """samples a row that a push of n >= 1 samples returns at most (n = 0: the flush)."""
        return int(lib().ws_engine_rate_stream_push_cap(self._h, int(n)))

    def _out(self, buf, m):
        return buf[:self.rows * m].reshape(self.rows, m).copy()

    def push(self, chunk, est_cap=None):
        """chunk [rows, n] at sample_rate, n >= 1 -> [rows, m] float32 at sample_rate, the samples that became final."""
        chunk = np.ascontiguousarray(chunk, dtype=np.float32)
        if chunk.ndim != 2 or chunk.shape[0] != self.rows:
            raise ValueError(f"EngineRateStream.push: chunk is {chunk.shape}, expected [{self.rows}, n >= 1]")
        n = chunk.shape[1]
        cap = self.push_cap(n) if est_cap is None else int(est_cap)
        buf, m = np.zeros(self.rows * max(cap, 1), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_rate_stream_push(self._h, chunk.ctypes.data, n, buf.ctypes.data, cap, C.byref(m)),
               "ws_engine_rate_stream_push")
        return self._out(buf, m.value)

    def flush(self, est_cap=None):
        """The end of the stream: A's flush, the stream's rest and flush, B's flush; the total is at most the samples pushed."""
        cap = self.push_cap(0) if est_cap is None else int(est_cap)
        buf, m = np.zeros(self.rows * max(cap, 1), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_rate_stream_flush(self._h, buf.ctypes.data, cap, C.byref(m)), "ws_engine_rate_stream_flush")
        return self._out(buf, m.value)

    def reset(self):
        """Back to sample 0; the enrollment is kept."""
        _check(lib().ws_engine_rate_stream_reset(self._h), "ws_engine_rate_stream_reset")

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(self._engine, "_h", None):
            _lib.ws_engine_rate_stream_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


def stream_block_group_launches(R, X):
    """WS_STREAM_BLOCK_GROUP_LAUNCHES: entry-point calls of one group of a stream opened with block_kernel=True."""
    return R * X + 10


def pool_block_group_launches(R, X):
    """WS_POOL_BLOCK_GROUP_LAUNCHES: entry-point calls of one group of a pool opened with block_kernel=True."""
    return R * X + 9


def pool_group_launches(R, X):
    """WS_POOL_GROUP_LAUNCHES: entry-point calls of one group of a pool push, whatever the number of slots in it."""
    return 3 * R * X + 9


class StreamPool:
    """ws_engine_pool_* (include/wesep_engine.h): many independent streams through one launch chain per push.  Every slot
    is a stream of one row: the concatenation of what its pushes and its flush return is the model-output part of
    Engine.separate's row on that slot's audio, whatever the other slots were fed in the meantime."""

    def __init__(self, engine, slots, max_chunk_frames=64, flags=0):
        self._h, self._engine, self.slots = C.c_void_p(), engine, int(slots)    # (the engine must outlive the pool)
        _quiesce_torch()
        if flags:
            _check(lib().ws_engine_pool_open_ex(engine._h, self.slots, int(max_chunk_frames), int(flags), C.byref(self._h)),
                   "ws_engine_pool_open_ex")
        else:
            _check(lib().ws_engine_pool_open(engine._h, self.slots, int(max_chunk_frames), C.byref(self._h)), "ws_engine_pool_open")
        self._L = engine.info("L")

    def attach(self, enroll, kind):
        """One enrollment -- [E] (ENROLL_EMBEDDING / ENROLL_SPEAKER) or [Tw] (ENROLL_WAVE) -- -> the slot it took.  The
        speaker stage runs here, once."""
        enroll = np.ascontiguousarray(enroll, dtype=np.float32).reshape(-1)
        length = 0 if kind in (ENROLL_EMBEDDING, ENROLL_SPEAKER) else enroll.shape[0]
        slot = C.c_int(-1)
        _quiesce_torch()
        _check(lib().ws_engine_pool_attach(self._h, enroll.ctypes.data, kind, length, C.byref(slot)), "ws_engine_pool_attach")
        return slot.value

    def push(self, chunks, est_cap=None):
        """{slot: chunk [n_slot >= 1]} -> {slot: float32 [m_slot]}, the samples of each slot that became final (m = 0 while no
        frame is complete).  est_cap: {slot: samples the output buffer holds} (default: what always suffices)."""
        ids = list(chunks)
        data = [np.ascontiguousarray(chunks[i], dtype=np.float32).reshape(-1) for i in ids]
        n = np.array([x.shape[0] for x in data], dtype=np.int32)
        caps = np.array([stream_push_cap(int(k), self._L) if est_cap is None else int(est_cap[i]) for i, k in zip(ids, n)],
                        dtype=np.int32)
        bufs = [np.zeros(max(int(c), 1), dtype=np.float32) for c in caps]
        A = len(ids)
        slots, m = np.array(ids, dtype=np.int32), np.zeros(max(A, 1), dtype=np.int32)
        cp = (C.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
        ep = (C.c_void_p * max(A, 1))(*[b.ctypes.data for b in bufs])
        _quiesce_torch()
        _check(lib().ws_engine_pool_push(self._h, A, slots.ctypes.data, C.cast(cp, C.c_void_p), n.ctypes.data,
                                         C.cast(ep, C.c_void_p), caps.ctypes.data, m.ctypes.data), "ws_engine_pool_push")
        return {i: b[:int(k)].copy() for i, b, k in zip(ids, bufs, m)}

    def flush(self, slot, est_cap=STREAM_FLUSH_CAP):
        """The end of one slot's stream: its remaining frames on the zero-extended pending samples, then the overlap-add carry."""
        buf, m = np.zeros(max(int(est_cap), 1), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_pool_flush(self._h, int(slot), buf.ctypes.data, int(est_cap), C.byref(m)), "ws_engine_pool_flush")
        return buf[:m.value].copy()

    def detach(self, slot):
        """Frees the slot for the next attach."""
        _check(lib().ws_engine_pool_detach(self._h, int(slot)), "ws_engine_pool_detach")

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(self._engine, "_h", None):
            _lib.ws_engine_pool_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


RATE_POOL_PIECE_LAUNCHES = 3        # WS_RATE_POOL_PIECE_LAUNCHES: resampler A, the pending samples' compaction, resampler B
RATE_POOL_BLOCK_PIECE_LAUNCHES = 3  # WS_RATE_POOL_BLOCK_PIECE_LAUNCHES


def rate_pool_group_launches(R, X):
    """WS_RATE_POOL_GROUP_LAUNCHES: a pool group, its gather and its scatter -- whatever the slots and rates in it."""
    return pool_group_launches(R, X) + 2


def rate_pool_block_group_launches(R, X):
    """WS_RATE_POOL_BLOCK_GROUP_LAUNCHES: the same for a pool opened with block_kernel=True."""
    return pool_block_group_launches(R, X) + 2


class RatePool:
    """ws_engine_rate_pool_* (include/wesep_engine.h): a StreamPool whose slots carry and return audio at their own sample
    rates.  Every slot is an EngineRateStream of one row: the concatenation of what its pushes and its flush return is what
    that stream returns for the same packets, whatever the other slots, their rates and their audio were."""

    def __init__(self, engine, slots, rates, max_chunk_frames=64, max_push=4800, flags=0):
        self._h, self._engine, self.slots = C.c_void_p(), engine, int(slots)    # (the engine must outlive the pool)
        rates = np.ascontiguousarray(list(rates), dtype=np.int32)
        _quiesce_torch()
        _check(lib().ws_engine_rate_pool_open(engine._h, self.slots, int(max_chunk_frames), int(flags), rates.ctypes.data, len(rates),
                                              int(max_push), C.byref(self._h)), "ws_engine_rate_pool_open")

    def attach(self, enroll, kind, sample_rate, enroll_rate=0):
        """One enrollment -- [E] (ENROLL_EMBEDDING / ENROLL_SPEAKER) or [Tw] (ENROLL_WAVE, at enroll_rate or the container's)
        -- and the rate of the slot's audio -> the slot it took."""
        enroll = np.ascontiguousarray(enroll, dtype=np.float32).reshape(-1)
        length = 0 if kind in (ENROLL_EMBEDDING, ENROLL_SPEAKER) else enroll.shape[0]
        slot = C.c_int(-1)
        _quiesce_torch()
        _check(lib().ws_engine_rate_pool_attach(self._h, enroll.ctypes.data, kind, length, int(enroll_rate), int(sample_rate),
                                                C.byref(slot)), "ws_engine_rate_pool_attach")
        return slot.value

    def push_cap(self, slot, n):
        """samples that a push of n >= 1 samples to `slot` returns at most (n = 0: the flush)."""
        return int(lib().ws_engine_rate_pool_push_cap(self._h, int(slot), int(n)))

    def push(self, chunks, est_cap=None):
        """{slot: chunk [n_slot >= 1] at the slot's rate} -> {slot: float32 [m_slot]} at the slot's rate."""
        ids = list(chunks)
        data = [np.ascontiguousarray(chunks[i], dtype=np.float32).reshape(-1) for i in ids]
        n = np.array([x.shape[0] for x in data], dtype=np.int32)
        caps = np.array([self.push_cap(i, int(k)) if est_cap is None else int(est_cap[i]) for i, k in zip(ids, n)], dtype=np.int32)
        bufs = [np.zeros(max(int(c), 1), dtype=np.float32) for c in caps]
        A = len(ids)
        slots, m = np.array(ids, dtype=np.int32), np.zeros(max(A, 1), dtype=np.int32)
        cp = (C.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
        ep = (C.c_void_p * max(A, 1))(*[b.ctypes.data for b in bufs])
        _quiesce_torch()
        _check(lib().ws_engine_rate_pool_push(self._h, A, slots.ctypes.data, C.cast(cp, C.c_void_p), n.ctypes.data,
                                              C.cast(ep, C.c_void_p), caps.ctypes.data, m.ctypes.data), "ws_engine_rate_pool_push")
        return {i: b[:int(k)].copy() for i, b, k in zip(ids, bufs, m)}

    def flush(self, slot, est_cap=None):
        """The end of one slot's stream; the slot's total is at most the samples pushed to it."""
        cap = self.push_cap(slot, 0) if est_cap is None else int(est_cap)
        buf, m = np.zeros(max(cap, 1), dtype=np.float32), C.c_int(0)
        _quiesce_torch()
        _check(lib().ws_engine_rate_pool_flush(self._h, int(slot), buf.ctypes.data, cap, C.byref(m)), "ws_engine_rate_pool_flush")
        return buf[:m.value].copy()

    def detach(self, slot):
        """Frees the slot for the next attach, at any accepted rate."""
        _check(lib().ws_engine_rate_pool_detach(self._h, int(slot)), "ws_engine_rate_pool_detach")

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(self._engine, "_h", None):
            _lib.ws_engine_rate_pool_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass
