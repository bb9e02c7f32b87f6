"""GPU: `ws_tcn_mid_stream_fwd` (csrc/stream.hip) -- bit-identical over chunkings, against a float64 restatement of the
header's formula and against the unfused chain of launches it replaces -- and `ConvTasNetStreamer(fused=True)` against the
same model's `forward` on the device.  Measured values are printed (profiles/engine_stream.md records them: 6.9e-8 to
1.1e-7 against float64, 0 against the unfused chain, 0 for the streamer against `forward`).

Bounds: 1e-5 relative L2 for the kernel, the bound tests/test_stream_tasnet_gpu.py holds ws_dwconv_stream_fwd to (fp32
sums of at most 1028 terms and at most 5 taps: a few 1e-7); 1e-4 for the streamer, the project's bound for a chunked
forward against the whole one."""
import pytest
import torch

from tests.test_stream_fused_host_cpu import FUSED_CONFIGS, make_fused_case
from tests.test_stream_tasnet_host_cpu import SMALL, T_TOTAL, chunkings, rel, stream, whole

pytestmark = pytest.mark.gpu

R_ = 2
EPS = 1e-5
CHUNKS37 = {"ones": [1] * 37, "mixed": [3, 5, 1, 7, 2, 9, 4, 6], "long": [20, 17], "whole": [37]}
CHUNKS9 = {"split": [4, 5], "whole": [9]}
_MID = {}


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _prelu64(v, a):
    return torch.where(v > 0, v, a * v)


def _mid_case(H, T, P, dil, with_rb):
    """Inputs, the float64 restatement and the unfused chain's results for one shape: made once, never modified."""
    key = (H, T, P, dil, with_rb)
    if key in _MID:
        return _MID[key]
    from wesep_amd import dev
    from wesep_amd import functional_tasnet as FT
    d = _cuda()
    g = torch.Generator().manual_seed(1000 * P + 10 * dil + H)
    M = R_ * T
    c = torch.randn(M, H, generator=g) * 1.5 + 0.3
    rb = torch.randn(R_, H, generator=g) * 0.7 if with_rb else None
    a1, a2 = torch.tensor([0.2]), torch.tensor([0.35])
    g1, b1 = torch.rand(H, generator=g) + 0.5, torch.randn(H, generator=g) * 0.1
    wd, bd = torch.randn(H, P, generator=g) * 0.5, torch.randn(H, generator=g) * 0.1
    # float64, from the formula in the header
    y1 = c.double().view(R_, T, H) + (rb.double().view(R_, 1, H) if with_rb else 0.0)
    y1 = _prelu64(y1, a1.double())
    xn = (y1 - y1.mean(2, keepdim=True)) / torch.sqrt(y1.var(2, unbiased=False, keepdim=True) + EPS) * g1.double() + b1.double()
    z = bd.double().expand(R_, T, H).clone()
    for p in range(P):
        off = (P - 1 - p) * dil
        if off < T:
            z[:, off:] += wd.double()[:, p] * xn[:, :T - off]
    y2 = _prelu64(z, a2.double())
    yn = (y2 - y2.mean(2, keepdim=True)) / torch.sqrt(y2.var(2, unbiased=False, keepdim=True) + EPS)
    dv = {k: (v.to(d) if v is not None else None) for k, v in
          dict(c=c, rb=rb, a1=a1, a2=a2, g1=g1, b1=b1, wd=wd, bd=bd).items()}
    # the unfused chain on the device, the whole sequence as one chunk
    cc = dv["c"].clone()                                            # prelu_fwd adds rb into its input in place
    u1, uz, u2 = (torch.empty(M, H, device=d) for _ in range(3))
    s1, s2 = torch.empty(M, 2, device=d), torch.empty(M, 2, device=d)
    uring = torch.full((R_, (P - 1) * dil + T, H), float("nan"), device=d)
    dev.prelu_fwd(cc, dv["rb"], dv["a1"], M, H, T, u1)
    dev.group_stats(u1, FT._cln_geom(M, H), s1, EPS)
    dev.dwconv_stream_fwd(u1, s1, dv["g1"], dv["b1"], dv["wd"], dv["bd"], R_, T, H, P, dil, 1, 0, uring, uz)
    dev.prelu_fwd(uz, None, dv["a2"], M, H, T, u2)
    dev.group_stats(u2, FT._cln_geom(M, H), s2, EPS)
    unf = (u2.view(R_, T, H), _normed(u2.view(R_, T, H), s2.view(R_, T, 2)), uring[:, :T].clone())
    _MID[key] = (dv, (y2, yn, xn), unf)
    return _MID[key]


def _normed(y2, st2):
    return (y2.double() - st2[..., 0:1].double()) * st2[..., 1:2].double()


def _run_fused(dv, T, H, P, dil, sizes, extra):
    """(y2 [R, T, H], st2 [R, T, 2], xn [R, T, H] read back from the written slots after every chunk, the final ring)."""
    from wesep_amd import dev
    d = dv["c"].device
    assert sum(sizes) == T
    cap = (P - 1) * dil + max(sizes) + extra                         # extra = 0: the contract at equality
    ring = torch.full((R_, cap, H), float("nan"), device=d)
    cs = dv["c"].view(R_, T, H)
    ys, ss, xs, t0 = [], [], [], 0
    for n in sizes:
        cc = cs[:, t0:t0 + n].reshape(R_ * n, H).contiguous()
        keep = cc.clone()
        y2, st2 = torch.empty(R_ * n, H, device=d), torch.empty(R_ * n, 2, device=d)
        dev.tcn_mid_stream_fwd(cc, dv["rb"], dv["a1"], dv["g1"], dv["b1"], dv["wd"], dv["bd"], dv["a2"], R_, n, H, P, dil, EPS,
                               t0, ring, y2, st2)
        assert torch.equal(cc, keep)                                 # c is read only
        ys.append(y2.view(R_, n, H))
        ss.append(st2.view(R_, n, 2))
        xs.append(ring[:, (t0 + torch.arange(n, device=d)) % cap].clone())
        t0 += n
    return torch.cat(ys, 1), torch.cat(ss, 1), torch.cat(xs, 1), ring


def _check_mid(H, T, P, dil, with_rb, extra, chunk_sets):
    dv, ref64, unf = _mid_case(H, T, P, dil, with_rb)
    runs = {k: _run_fused(dv, T, H, P, dil, sizes, extra) for k, sizes in chunk_sets.items()}
    y0, s0, x0, _ = runs["whole"]
    worst = {}
    for k, (y2, st2, xn, ring) in runs.items():
        # (a) bit for bit the single chunk with the whole sequence
        assert torch.equal(y2, y0) and torch.equal(st2, s0) and torch.equal(xn, x0), k
        # (b) every output finite; slots no frame maps to still NaN; the others hold their latest frame's xn
        assert torch.isfinite(y2).all() and torch.isfinite(st2).all() and torch.isfinite(xn).all(), k
        cap = ring.shape[1]
        last = {a % cap: a for a in range(T)}
        for slot in range(cap):
            if slot in last:
                assert torch.equal(ring[:, slot], xn[:, last[slot]]), (k, slot)
            else:
                assert torch.isnan(ring[:, slot]).all(), (k, slot)
    # (c) the float64 restatement, (d) the unfused chain on this device
    got = (y0, _normed(y0, s0), x0)
    for tag, ref in (("float64", ref64), ("unfused", unf)):
        errs = [rel(a, b) for a, b in zip(got, ref)]
        worst[tag] = max(errs)
        print(f"tcn_mid H={H} P={P} dil={dil} rb={with_rb} cap+{extra}: vs {tag} y2 {errs[0]:.3e} normed {errs[1]:.3e} "
              f"ring {errs[2]:.3e}")
        assert all(e < 1e-5 for e in errs), (tag, errs)
    return worst


@pytest.mark.parametrize("with_rb", [True, False])
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("P,dil", [(3, 1), (3, 4), (5, 2)])
def test_tcn_mid_stream_fewer_quads_than_a_wave(P, dil, extra, with_rb):
    _check_mid(8, 37, P, dil, with_rb, extra, CHUNKS37)


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("P,dil", [(3, 1), (3, 4), (5, 2)])
@pytest.mark.parametrize("H", [512, 1028])
def test_tcn_mid_stream_wide_channels(H, P, dil, extra):
    """128 quads (two waves, the SpEx+ width) and 257 quads (more quads than 256 threads: a thread owns two)."""
    _check_mid(H, 9, P, dil, True, extra, CHUNKS9)


def test_tcn_mid_stream_refusals():
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    z = lambda *s: torch.zeros(*s, device=d)

    def call(H=8, P=3, dil=4, t0=0, cap=13, null=False, alias=False):
        Tc = 5
        c = z(R_ * Tc, H)
        dev.tcn_mid_stream_fwd(c, z(R_, H), None if null else z(1), z(H), z(H), z(H, P), z(H), z(1), R_, Tc, H, P, dil, EPS, t0,
                               z(R_, cap, H), c if alias else z(R_ * Tc, H), z(R_ * Tc, 2))

    call()                                                          # the base case is accepted
    for kw, msg in ((dict(null=True), "null pointer"), (dict(H=6), "H=6 is not a multiple of 4"),
                    (dict(H=4100), "H=4100 above 4096"), (dict(P=4, cap=17), r"P=4 \(odd P <= 7\)"),
                    (dict(P=9, cap=37), r"P=9 \(odd P <= 7\)"), (dict(dil=0), "bad geometry"),
                    (dict(t0=-1), "t0=-1 is negative"), (dict(cap=12), r"cap=12 is below \(P - 1\) \* dil \+ Tc = 13"),
                    (dict(alias=True), "y2 overlaps c")):
        with pytest.raises(L.WesepHipError, match=msg):
            call(**kw)
    torch.cuda.synchronize()


# ---- the streamer ---------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(name):
    if name not in _CASES:
        model, x, enroll = make_fused_case(name, 2, device=_cuda())
        _CASES[name] = (model, x, enroll, whole(model, x, enroll))
    return _CASES[name]


@pytest.mark.parametrize("chunking", ["all160", "all7", "random1to400", "one"])
@pytest.mark.parametrize("name", sorted(FUSED_CONFIGS))
def test_fused_streamer_matches_forward_on_the_device(name, chunking):
    from wesep_amd.streaming import ConvTasNetStreamer
    model, x, enroll, ref = _case(name)
    st = ConvTasNetStreamer(model, 2, max_chunk_frames=64, fused=True)
    st.enroll(enroll)
    got, counts = stream(st, x, chunkings()[chunking])
    Lmax = st.latency_samples
    assert all(emitted == (max(0, (pushed - Lmax) // 10 + 1) * 10 if pushed >= Lmax else 0) for pushed, emitted in counts)
    assert got.shape == ref.shape == (2, ((T_TOTAL - 20) // 10) * 10 + 20) and torch.isfinite(got).all()
    assert float(ref.abs().max()) > 0
    e = rel(got, ref)
    print(f"fused streamer {name} {chunking}: rel L2 vs forward {e:.3e}")
    assert e < 1e-4, (name, chunking, e)


def test_fused_streamer_refuses_bn_by_name():
    from wesep_amd.models import get_model
    from wesep_amd.streaming import ConvTasNetStreamer
    model = get_model("ConvTasNet")(**dict(SMALL, norm="BN")).to(_cuda()).eval()
    with pytest.raises(NotImplementedError, match="BN"):
        ConvTasNetStreamer(model, 2, fused=True)


@pytest.mark.parametrize("name", ["multi_cln_concatconv", "plain_cln_skip_film"])
def test_fused_push_makes_four_fewer_calls_per_block(name, monkeypatch):
    """Every C-ABI call of the library goes through _lib.check: count them for one push of one group of frames."""
    from wesep_amd import _lib as L
    from wesep_amd.streaming import ConvTasNetStreamer
    model, x, enroll, _ = _case(name)
    calls = []
    real = L.check
    monkeypatch.setattr(L, "check", lambda rc, what="": (calls.append(what), real(rc, what))[1])
    counts = {}
    for fused in (False, True):
        st = ConvTasNetStreamer(model, 2, max_chunk_frames=64, fused=fused)
        st.enroll(enroll)
        del calls[:]
        st.push(x[:, :400])
        counts[fused] = len(calls)
        assert calls.count("ws_tcn_mid_stream_fwd") == (SMALL["X"] * SMALL["R"] if fused else 0)
    print(f"C-ABI calls per push, {name}: unfused {counts[False]}, fused {counts[True]}")
    assert counts[False] - counts[True] == 4 * SMALL["X"] * SMALL["R"]
