"""GPU: the resampling kernels through the C ABI (wesep_amd.dev / wesep_amd.resample) against the fp64 restatement
(tests/resample_contract.py): every sample within gamma_K sum |taps32| |x|, nothing read behind n_in, nothing written
behind n_out; the streaming form bit for bit the whole-signal form under any chunking, rows independent, runs repeatable."""
import numpy as np
import pytest
import torch

from tests import resample_contract as RC

pytestmark = pytest.mark.gpu
STREAM_PAIRS = [(8000, 16000), (48000, 16000), (44100, 16000), (16000, 44100)]
GUARD = 12345.0


@pytest.fixture(scope="module")
def signal():
    """[3, 1999] float64 in (-1, 1), made once and never modified"""
    x = np.random.default_rng(7).uniform(-1.0, 1.0, size=(3, 1999))
    x.setflags(write=False)
    return x


def _sizes(pair):
    _, _, w, K = RC.GEOM[pair]
    return [1, w, K - 1, K, 257, 1999]


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("pair", RC.PAIRS)
def test_whole_signal_against_fp64(pair, R, signal):
    from wesep_amd import dev
    from wesep_amd.resample import taps_on
    d = torch.device("cuda:0")
    taps = taps_on(*pair, d)
    assert np.array_equal(taps.cpu().numpy(), RC.taps32(*pair))
    for n_in in _sizes(pair):
        n_out = RC.out_len(n_in, *pair)
        x32 = signal[:R, :n_in].astype(np.float32)
        xd = torch.full((R, n_in + 3), float("nan"), device=d)           # unaligned rows, NaN behind n_in
        xd[:, :n_in] = torch.from_numpy(x32).to(d)
        yd = torch.full((R, n_out + 5), GUARD, device=d)
        dev.resample_fwd(xd, n_in, *pair, taps, yd)
        y = yd.cpu().numpy().astype(np.float64)
        assert np.all(y[:, n_out:] == GUARD), (pair, R, n_in, "wrote behind n_out")
        assert np.all(np.isfinite(y[:, :n_out])), (pair, R, n_in)
        worst = 0.0
        for r in range(R):
            ref, bnd = RC.reference(x32[r], *pair), RC.bound(x32[r], *pair)
            e = np.abs(y[r, :n_out] - ref)
            worst = max(worst, float(np.max(e / np.maximum(bnd, 1e-300))))
            assert np.all(e <= bnd), (pair, R, n_in, r, float(e.max()), float(bnd[np.argmax(e - bnd)]))
        print(f"{pair} R {R} n_in {n_in}: worst error / bound {worst:.3f}")


def _chunkings(K, n):
    rng = np.random.default_rng(3)
    rnd, left = [], n
    while left:
        c = int(min(left, rng.integers(1, 501)))
        rnd.append(c)
        left -= c
    mixed, left, i = [], n, 0
    while left:
        c = min(left, (K - 1, 1, K)[i % 3])
        mixed.append(c)
        left -= c
        i += 1
    return {"all1": [1] * n, "all7": [7] * (n // 7) + ([n % 7] if n % 7 else []), "K-1,1,K": mixed, "random": rnd, "one": [n]}


@pytest.mark.parametrize("pair", STREAM_PAIRS)
def test_streaming_is_the_whole_signal_bit_for_bit(pair, signal):
    from wesep_amd.resample import StreamResampler, resample
    d = torch.device("cuda:0")
    K, n = RC.GEOM[pair][3], 1999
    x = torch.from_numpy(signal[:2, :n].astype(np.float32)).to(d)
    whole = resample(x, *pair)
    assert whole.shape == (2, RC.out_len(n, *pair))
    for name, chunks in _chunkings(K, n).items():
        # max_push 500 cuts a longer chunk into pieces; "one" is ONE streaming launch over all 1999 samples
        st = StreamResampler(2, *pair, max_push=2000 if name == "one" else 500, device=d)
        outs, seen = [], 0
        for c in chunks:
            y = st.push(x[:, seen:seen + c])
            seen += c
            assert y.shape[1] == RC.emitted(seen, *pair) - RC.emitted(seen - c, *pair), (pair, name, seen)
            outs.append(y)
            if c > 1 or seen % 97 == 0:        # the history is the input from max(0, G D - w) on (all1: every 97th push)
                assert st.history.shape[1] < K and torch.equal(st.history, x[:, seen - st.history.shape[1]:seen]), (pair, name, seen)
        outs.append(st.flush())
        y = torch.cat(outs, dim=1)
        assert y.shape == whole.shape and torch.equal(y, whole), (pair, name)
        st.reset()                              # a second stream on the same object: the same bits again
        y2 = torch.cat([st.push(x[:, :1000]), st.push(x[:, 1000:]), st.flush()], dim=1)
        assert torch.equal(y2, whole), (pair, name, "after reset")


@pytest.mark.parametrize("pair", [(8000, 16000), (44100, 16000)])
def test_rows_are_independent_and_runs_repeat(pair, signal):
    from wesep_amd.resample import resample
    d = torch.device("cuda:0")
    x = torch.from_numpy(signal.astype(np.float32)).to(d)
    y3 = resample(x, *pair)
    for r in range(3):
        assert torch.equal(resample(x[r:r + 1].contiguous(), *pair)[0], y3[r]), (pair, r)
    assert torch.equal(resample(x, *pair), y3)


@pytest.mark.parametrize("pair", [(8000, 16000), (48000, 16000)])
def test_sine_through_the_kernel(pair):
    from wesep_amd.resample import resample
    x = torch.from_numpy(RC.sine(pair[0]).astype(np.float32)).cuda()[None]
    e = RC.sine_error(*pair, resample(x, *pair)[0].cpu().numpy())
    print(f"{pair}: 1 kHz sine through the kernel, max error over the middle three quarters {e:.2e}")
    assert e <= 2e-3
