"""GPU: audio at the caller's sample rate through the engine -- Engine.resample against wesep_amd.resample, separate_rate and
the rate stream against the composition Engine.resample -> Engine.separate / the plain stream -> Engine.resample, cropped."""
import numpy as np
import pytest
import torch

from tests import resample_contract as RC
from tests.test_zzz_stream_pool_gpu import _engine, _rel
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
_BS = {}


def _audio(rate, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(2, n, generator=g)).numpy()


def _tasnet(tmp_path_factory):
    eng, _, enroll, kind = _engine(False, tmp_path_factory)
    return eng, np.stack([enroll["a"], enroll["b"]]), kind


def _bsrnn(tmp_path_factory):
    if "e" not in _BS:
        from wesep_amd.models import get_model
        torch.manual_seed(5)
        model = get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False, joint_training=False)
        path = str(tmp_path_factory.mktemp("rate") / "b.wsw")
        export_engine(model, path)
        _BS["e"] = E.Engine(path)
    return _BS["e"], torch.randn(2, 256, generator=torch.Generator().manual_seed(6)).numpy(), E.ENROLL_EMBEDDING


@pytest.mark.parametrize("pair", [(8000, 16000), (16000, 48000), (44100, 16000)])
def test_engine_resample_is_the_device_resampler(pair, tmp_path_factory):
    from wesep_amd.resample import resample
    eng, _, _ = _tasnet(tmp_path_factory)
    x = _audio(pair[0], 1999, 1)
    y = eng.resample(x, *pair)
    ref = resample(torch.from_numpy(x).cuda(), *pair).cpu().numpy()
    assert y.shape == ref.shape == (2, RC.out_len(1999, *pair)) and np.array_equal(y, ref)
    assert eng.info("n_launches") == 1


@pytest.mark.parametrize("arch", ["pBSRNN", "ConvTasNet"])
@pytest.mark.parametrize("rate", [8000, 48000])
def test_separate_rate_is_the_composition(arch, rate, tmp_path_factory):
    eng, enroll, kind = (_bsrnn if arch == "pBSRNN" else _tasnet)(tmp_path_factory)
    T = 2000 * rate // 16000 + 3
    x = _audio(rate, T, 2)
    x_m = eng.resample(x, rate, 16000)
    y_m = eng.separate(x_m, enroll, kind)
    plain = eng.info("n_launches")
    ref = eng.resample(y_m, 16000, rate)[:, :T]
    est = eng.separate_rate(x, enroll, kind, rate)
    assert eng.info("n_launches") == plain + 2
    assert est.shape == (2, T) and np.all(np.isfinite(est)) and np.array_equal(est, ref)
    assert np.array_equal(eng.separate_rate(x_m, enroll, kind, 16000), y_m) and eng.info("n_launches") == plain


def _stream_all(st, x, sizes):
    outs, pos = [], 0
    for c in sizes:
        outs.append(st.push(x[:, pos:pos + c]))
        pos += c
    assert pos == x.shape[1]
    outs.append(st.flush())
    return np.concatenate(outs, axis=1)


def _composition(eng, enroll, kind, x, rate, block_kernel):
    x_m = eng.resample(x, rate, 16000)
    st = eng.stream(2, enroll, kind, max_chunk_frames=16, block_kernel=block_kernel)
    y_m = _stream_all(st, x_m, [x_m.shape[1]])
    st.close()
    return eng.resample(y_m, 16000, rate)[:, :x.shape[1]]


def _packets(n, lo, hi, seed):
    rng, out = np.random.default_rng(seed), []
    while n:
        out.append(int(min(n, rng.integers(lo, hi + 1))))
        n -= out[-1]
    return out


@pytest.mark.parametrize("rate,n", [(8000, 3001), (48000, 12007)])
def test_flagged_rate_stream_is_the_composition_bit_for_bit(rate, n, tmp_path_factory):
    eng, enroll, kind = _tasnet(tmp_path_factory)
    x = _audio(rate, n, 3)
    ref = _composition(eng, enroll, kind, x, rate, True)
    total = RC.rate_stream_total(n, rate, 16000, 20)
    assert ref.shape[1] >= total
    got = {}
    for name, sizes in (("fixed", [80] * (n // 80) + ([n % 80] if n % 80 else [])), ("random", _packets(n, 1, 4000, 4))):
        st = eng.rate_stream(2, enroll, kind, rate, max_chunk_frames=16, max_push=1500, block_kernel=True)
        state = eng.info("stream_state_bytes")
        got[name] = _stream_all(st, x, sizes)
        assert eng.info("stream_state_bytes") == state
        st.close()
        assert got[name].shape == (2, total) and np.all(np.isfinite(got[name]))
        assert np.array_equal(got[name], ref[:, :total]), (rate, name)
    assert np.array_equal(got["fixed"], got["random"])


@pytest.mark.parametrize("rate,n", [(8000, 3001), (48000, 12007)])
def test_default_rate_stream_against_the_composition(rate, n, tmp_path_factory):
    eng, enroll, kind = _tasnet(tmp_path_factory)
    x = _audio(rate, n, 3)
    ref = _composition(eng, enroll, kind, x, rate, False)
    st = eng.rate_stream(2, enroll, kind, rate, max_chunk_frames=16, max_push=1500)
    got = _stream_all(st, x, _packets(n, 1, 4000, 5))
    st.close()
    e = _rel(got, ref[:, :got.shape[1]])
    print(f"rate {rate}: default-path rate stream against the composition: rel {e:.2e}, "
          f"bit-identical: {np.array_equal(got, ref[:, :got.shape[1]])}")
    assert got.shape == (2, RC.rate_stream_total(n, rate, 16000, 20)) and e <= 1e-4


@pytest.mark.parametrize("block_kernel", [False, True])
def test_rate_stream_at_the_container_rate_is_the_plain_stream(block_kernel, tmp_path_factory):
    eng, enroll, kind = _tasnet(tmp_path_factory)
    x = _audio(16000, 2411, 8)
    sizes = _packets(2411, 1, 500, 9)
    a = eng.stream(2, enroll, kind, max_chunk_frames=16, block_kernel=block_kernel)
    ya = _stream_all(a, x, sizes)
    a.close()
    b = eng.rate_stream(2, enroll, kind, 16000, max_chunk_frames=16, block_kernel=block_kernel)
    yb = _stream_all(b, x, sizes)
    b.close()
    assert ya.shape == yb.shape and np.array_equal(ya, yb)
