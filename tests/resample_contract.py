"""Shared restatement of the resampler's contract (include/wesep_hip.h, "sample rates") for the resample tests.

The filter is defined by formula -- the published sinc_interp_hann design with lowpass_filter_width = 6, rolloff = 0.99:
    g = gcd, D = rate_in / g, U = rate_out / g, base = min(D, U) * 0.99, w = ceil(6 D / base), K = 2 w + D
    t = clamp((-p / U + (k - w) / D) * base, -6, 6)
    taps[p][k] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos^2(pi t / 12) * base / D        (double, rounded to float once)
    y[q] = sum_{k < K} taps[q % U][k] * x[(q // U) * D + k - w],  q < ceil(U n_in / D),  x = 0 outside [0, n_in)
Everything here is numpy fp64 (the table through the C library's sin and cos, one entry at a time, in the order of
operations above).  The error bound of a sample computed by sequential fp32 accumulation over K terms is the standard
    |fl(sum) - sum| <= gamma_K * sum_k |taps32[p][k]| |x_k|,   gamma_K = K 2^-24 / (1 - K 2^-24)
with the float-rounded taps on both sides (the products are exact in fp64; fmaf rounds once per term)."""
import functools
import math

import numpy as np

PAIRS = [(8000, 16000), (48000, 16000), (44100, 16000), (16000, 8000), (16000, 48000), (16000, 44100), (22050, 16000)]
GEOM = {(8000, 16000): (2, 1, 7, 15), (48000, 16000): (1, 3, 19, 41), (44100, 16000): (160, 441, 17, 475),
        (16000, 8000): (1, 2, 13, 28), (16000, 48000): (3, 1, 7, 15), (16000, 44100): (441, 160, 7, 174),
        (22050, 16000): (320, 441, 9, 459)}      # (U, D, w, K), the table of the filter's definition


def geometry(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    D, U = rate_in // g, rate_out // g
    base = min(D, U) * 0.99
    w = int(math.ceil(6.0 * D / base))
    return U, D, w, 2 * w + D


@functools.lru_cache(maxsize=None)
def taps64(rate_in, rate_out):
    """[U, K] float64, before the rounding to float"""
    U, D, w, K = geometry(rate_in, rate_out)
    base = min(D, U) * 0.99
    out = np.empty((U, K), dtype=np.float64)
    for p in range(U):
        for k in range(K):
            t = (-float(p) / float(U) + float(k - w) / float(D)) * base
            t = -6.0 if t < -6.0 else (6.0 if t > 6.0 else t)
            sinc = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
            c = math.cos(math.pi * t / 12.0)
            out[p, k] = sinc * (c * c) * base / float(D)
    return out


@functools.lru_cache(maxsize=None)
def taps32(rate_in, rate_out):
    """[U, K] float32: the table the kernel reads"""
    return taps64(rate_in, rate_out).astype(np.float32)


def out_len(n_in, rate_in, rate_out):
    U, D, _, _ = geometry(rate_in, rate_out)
    return -(-U * n_in // D)


def _windows(x, rate_in, rate_out):
    """[n_out, K] float64: the zero-extended input samples under each output's taps, and each output's phase"""
    U, D, w, K = geometry(rate_in, rate_out)
    n_in = x.shape[-1]
    n_out = -(-U * n_in // D)
    q = np.arange(n_out)
    xp = np.concatenate([np.zeros(w), np.asarray(x, dtype=np.float64), np.zeros(K + D)])
    idx = (q // U)[:, None] * D + np.arange(K)[None, :]          # (q // U) D + k - w, shifted by the w zeros in front
    return xp[idx], q % U


def reference(x, rate_in, rate_out, taps=None):
    """y [n_out] float64 for one row x [n_in], with the float-rounded table (or `taps`, e.g. taps64)"""
    t = np.asarray(taps32(rate_in, rate_out) if taps is None else taps, dtype=np.float64)
    win, p = _windows(x, rate_in, rate_out)
    return np.einsum("qk,qk->q", win, t[p])


def bound(x, rate_in, rate_out):
    """[n_out] float64: gamma_K sum_k |taps32[p][k]| |x_k| per output sample"""
    K = geometry(rate_in, rate_out)[3]
    u = K * 2.0 ** -24
    win, p = _windows(x, rate_in, rate_out)
    return u / (1.0 - u) * np.einsum("qk,qk->q", np.abs(win), np.abs(taps32(rate_in, rate_out).astype(np.float64))[p])


# ---- emission rules ----
def emitted(N, rate_in, rate_out):
    """outputs a streaming resampler has returned after N input samples"""
    U, D, w, _ = geometry(rate_in, rate_out)
    return U * max(0, (N - w) // D)


def plain_emitted(N, L):
    """samples a row the plain Conv-TasNet stream has returned after N samples (frame k runs once k s + 160 <= N)"""
    s = L // 2
    return ((N - 160) // s + 1) * s if N >= 160 else 0


def plain_total(N, L):
    """samples a row the plain stream returns in all, flush included (N >= L)"""
    s = L // 2
    return ((N - L) // s) * s + L


def rate_stream_emitted(N, sample_rate, model_rate, L):
    """B's emission on the plain stream's emission on A's emission"""
    return emitted(plain_emitted(emitted(N, sample_rate, model_rate), L), model_rate, sample_rate)


def rate_stream_total(N, sample_rate, model_rate, L):
    """samples a rate stream returns in all: the composition's length, cropped to the samples pushed"""
    return min(N, out_len(plain_total(out_len(N, sample_rate, model_rate), L), model_rate, sample_rate))


def sine_error(rate_in, rate_out, y, freq=1000.0):
    """max |y - analytic sine| over the middle three quarters of y (y: the resampled sin(2 pi f t))"""
    n = y.shape[-1]
    q = np.arange(n)
    ref = np.sin(2 * np.pi * freq * q / rate_out)
    lo, hi = n // 8, n - n // 8
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64)[..., lo:hi] - ref[lo:hi])))


def sine(rate, seconds=0.25, freq=1000.0):
    n = int(round(rate * seconds))
    return np.sin(2 * np.pi * freq * np.arange(n) / rate)
