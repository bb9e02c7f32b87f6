"""GPU: the chunked kernels of csrc/stream.hip against the whole-sequence kernels they restate (bit for bit) and a float64
restatement, and ConvTasNetStreamer against the same model's `forward` on the device.  Shapes are the smallest at which the
ring wraps, a chunk is longer than the receptive field, and a chunk is a single frame.  Measured values are printed
(profiles/stream_tasnet.md records them)."""
import pytest
import torch

from tests.test_stream_tasnet_host_cpu import T_TOTAL, chunkings, make_case, rel, stream, whole

pytestmark = pytest.mark.gpu


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- ws_dwconv_stream_fwd ------------------------------------------------------------------------------------------------
R_, C_, T_ = 2, 8, 37
CHUNKS = {"ones": [1] * 37, "mixed": [3, 5, 1, 7, 2, 9, 4, 6], "long": [20, 17]}     # 20, 17 > (P - 1) * dil <= 8
_DW = {}


def _dw_case(P, dil, stats_kind):
    """Inputs, the whole-sequence kernel's output and the float64 restatement for one (P, dil, statistics): made once."""
    key = (P, dil, stats_kind)
    if key in _DW:
        return _DW[key]
    from wesep_amd import dev
    from wesep_amd import functional_tasnet as FT
    d = _cuda()
    g = torch.Generator().manual_seed(100 * P + dil)
    x = (torch.randn(R_ * T_, C_, generator=g) * 1.5 + 0.3).to(d)
    gamma, beta = (torch.rand(C_, generator=g) + 0.5).to(d), (torch.randn(C_, generator=g) * 0.1).to(d)
    w, b = (torch.randn(C_, P, generator=g) * 0.5).to(d), (torch.randn(C_, generator=g) * 0.1).to(d)
    if stats_kind == "cLN":
        st, st_div = FT.norm_stats(x, "cLN", R_, T_, C_), 1
        rows = st.double().cpu()
    else:                       # eval-mode BN: identity statistics, one row for the whole call
        st, st_div = torch.tensor([[0.0, 1.0]], device=d), R_ * T_
        rows = st.double().cpu().expand(R_ * T_, 2)
    whole_y = torch.empty(R_ * T_, C_, device=d)
    dev.dwconv_fwd(x, st, gamma, beta, w, b, R_, T_, C_, P, dil, st_div, whole_y, causal=True)
    xn = ((x.double().cpu() - rows[:, 0:1]) * rows[:, 1:2] * gamma.double().cpu() + beta.double().cpu()).view(R_, T_, C_)
    y64 = b.double().cpu().expand(R_, T_, C_).clone()
    for p in range(P):
        off = (P - 1 - p) * dil
        if off < T_:
            y64[:, off:] += w.double().cpu()[:, p] * xn[:, :T_ - off]
    _DW[key] = (x, st, st_div, gamma, beta, w, b, whole_y.view(R_, T_, C_), y64)
    return _DW[key]


@pytest.mark.parametrize("stats_kind", ["cLN", "identity"])
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("chunks", sorted(CHUNKS))
@pytest.mark.parametrize("P,dil", [(3, 1), (3, 4), (5, 2)])
def test_dwconv_stream_is_the_whole_sequence_kernel_bit_for_bit(P, dil, chunks, extra, stats_kind):
    from wesep_amd import dev
    x, st, st_div, gamma, beta, w, b, whole_y, y64 = _dw_case(P, dil, stats_kind)
    d = x.device
    sizes = CHUNKS[chunks]
    assert sum(sizes) == T_
    cap = (P - 1) * dil + max(sizes) + extra                       # extra = 0: the contract at equality
    ring = torch.full((R_, cap, C_), float("nan"), device=d)
    xs = x.view(R_, T_, C_)
    got, t0 = [], 0
    for n in sizes:
        xc = xs[:, t0:t0 + n].reshape(R_ * n, C_).contiguous()
        if stats_kind == "cLN":                                     # the whole sequence's statistics, sliced
            sc, div = st.view(R_, T_, 2)[:, t0:t0 + n].reshape(R_ * n, 2).contiguous(), 1
        else:
            sc, div = st, R_ * n
        yc = torch.empty(R_ * n, C_, device=d)
        dev.dwconv_stream_fwd(xc, sc, gamma, beta, w, b, R_, n, C_, P, dil, div, t0, ring, yc)
        got.append(yc.view(R_, n, C_))
        t0 += n
    got = torch.cat(got, 1)
    assert torch.isfinite(got).all()                                # NaN in the ring never reaches an output
    assert torch.equal(got, whole_y), float((got - whole_y).abs().max())
    e = rel(got, y64)
    print(f"dwconv_stream P={P} dil={dil} {chunks} cap+{extra} {stats_kind}: rel vs float64 {e:.3e}")
    assert e < 1e-5


@pytest.mark.parametrize("Cc", [512, 1028])
def test_dwconv_stream_wide_channels_bit_for_bit(Cc):
    """The launch shapes the 8-channel cases do not reach: 128 channel quads (two frames per workgroup, the SpEx+ width)
    and 257 quads (more quads than threads: the channel loop runs twice)."""
    from wesep_amd import dev
    from wesep_amd import functional_tasnet as FT
    d = _cuda()
    R, T, P, dil = 2, 9, 3, 2
    g = torch.Generator().manual_seed(Cc)
    x = torch.randn(R * T, Cc, generator=g).to(d)
    gamma, beta = (torch.rand(Cc, generator=g) + 0.5).to(d), (torch.randn(Cc, generator=g) * 0.1).to(d)
    w, b = (torch.randn(Cc, P, generator=g) * 0.5).to(d), (torch.randn(Cc, generator=g) * 0.1).to(d)
    st = FT.norm_stats(x, "cLN", R, T, Cc)
    ref = torch.empty(R * T, Cc, device=d)
    dev.dwconv_fwd(x, st, gamma, beta, w, b, R, T, Cc, P, dil, 1, ref, causal=True)
    ring = torch.full((R, (P - 1) * dil + 5, Cc), float("nan"), device=d)
    got, t0 = [], 0
    for n in (4, 5):
        yc = torch.empty(R * n, Cc, device=d)
        dev.dwconv_stream_fwd(x.view(R, T, Cc)[:, t0:t0 + n].reshape(R * n, Cc).contiguous(),
                              st.view(R, T, 2)[:, t0:t0 + n].reshape(R * n, 2).contiguous(), gamma, beta, w, b, R, n, Cc, P, dil, 1,
                              t0, ring, yc)
        got.append(yc.view(R, n, Cc))
        t0 += n
    assert torch.equal(torch.cat(got, 1), ref.view(R, T, Cc))


def test_dwconv_stream_refuses_a_ring_below_the_bound():
    from wesep_amd import _lib as L
    from wesep_amd import dev
    x, st, st_div, gamma, beta, w, b, _, _ = _dw_case(3, 4, "cLN")
    ring = torch.zeros(R_, 2 * 4 + 5 - 1, C_, device=x.device)
    y = torch.empty(R_ * 5, C_, device=x.device)
    with pytest.raises(L.WesepHipError, match=r"cap=12 is below \(P - 1\) \* dil \+ Tc = 13"):
        dev.dwconv_stream_fwd(x[:R_ * 5].contiguous(), st[:R_ * 5].contiguous(), gamma, beta, w, b, R_, 5, C_, 3, 4, 1, 0, ring, y)


# ---- ws_ola_stream_fwd -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lk,hop", [(20, 10), (16, 8), (40, 10)])
def test_ola_stream_is_ola_fwd_bit_for_bit(Lk, hop):
    from wesep_amd import dev
    d = _cuda()
    R, Tf = 3, 16
    g = torch.Generator().manual_seed(Lk)
    fr = torch.randn(R, Tf, Lk, generator=g).to(d)
    bias = torch.tensor([0.37], device=d)
    Tout = (Tf - 1) * hop + Lk
    ref = torch.empty(R, Tout, device=d)
    dev.ola_fwd(fr.view(R * Tf, Lk), bias, R, Tf, Lk, hop, Tout, ref)
    carry = bias.expand(R, Lk - hop).contiguous()                  # a reset: the carry is the bias
    outs, t = [], 0
    for n in (1, 4, 2, 9):
        est = torch.empty(R, n * hop, device=d)
        dev.ola_stream_fwd(fr[:, t:t + n].reshape(R * n, Lk).contiguous(), bias, R, n, Lk, hop, carry, est)
        outs.append(est)
        t += n
    got = torch.cat(outs + [carry], 1)                              # flush: the carry is the last L - hop samples
    assert got.shape == ref.shape and torch.equal(got, ref), float((got - ref).abs().max())


# ---- the streamer against the same model's forward -----------------------------------------------------------------------
GPU_CONFIGS = ["multi_cln_concatconv", "plain_bn_skip_film_sigmoid", "multi_cln_joint_spexplus"]
_CASES = {}


def _case(name):
    if name not in _CASES:
        model, x, enroll = make_case(name, 2, device=_cuda())
        _CASES[name] = (model, x, enroll, whole(model, x, enroll))
    return _CASES[name]


@pytest.mark.parametrize("chunking", sorted(chunkings()))
@pytest.mark.parametrize("name", GPU_CONFIGS)
def test_streamer_matches_forward_on_the_device(name, chunking):
    """rel L2 against `forward` below 1e-4, the project's bound for 'a row in a rectangle against the row alone'
    (tests/test_ragged_gridnet_gpu.py::_check_rows)."""
    from wesep_amd.streaming import ConvTasNetStreamer
    model, x, enroll, ref = _case(name)
    st = ConvTasNetStreamer(model, 2, max_chunk_frames=64)
    st.enroll(enroll)
    got, counts = stream(st, x, chunkings()[chunking])
    Lmax = st.latency_samples
    assert all(emitted == (max(0, (pushed - Lmax) // 10 + 1) * 10 if pushed >= Lmax else 0) for pushed, emitted in counts)
    assert got.shape == ref.shape == (2, ((T_TOTAL - 20) // 10) * 10 + 20) and torch.isfinite(got).all()
    assert float(ref.abs().max()) > 0
    e = rel(got, ref)
    print(f"streamer {name} {chunking}: rel L2 vs forward {e:.3e}")
    assert e < 1e-4, (name, chunking, e)


@pytest.mark.parametrize("name", GPU_CONFIGS)
def test_reset_reproduces_the_outputs_bit_for_bit(name):
    from wesep_amd.streaming import ConvTasNetStreamer
    model, x, enroll, ref = _case(name)
    st = ConvTasNetStreamer(model, 2, max_chunk_frames=64)
    st.enroll(enroll)
    a, _ = stream(st, x, chunkings()["random1to400"])
    st.reset()
    b, _ = stream(st, x, chunkings()["random1to400"])
    assert torch.equal(a, b)
    st.reset()
    c, _ = stream(st, x, chunkings()["all160"])                     # another chunking: the same length
    assert c.shape == a.shape == ref.shape
    assert st.state_bytes > 0 and st.latency_samples == (20 if "plain" in name else 160)
