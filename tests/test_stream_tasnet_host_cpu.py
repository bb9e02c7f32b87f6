"""CPU: streaming Conv-TasNet without a GPU -- the two new symbols and their argument contracts in the built library, and
the host logic of wesep_amd/streaming.py (pending samples, emission rule, rings, carry, flush, refusals) on the torch
emulation of tests/emu_stream.py against the SAME model's whole-utterance forward.  No streaming fixture comes from the
reference (it has no chunked forward): the causal blocks and cLN of `forward` are what the reference fixtures pin.
Every test here fails on the commit before: the symbols and the module do not exist."""
import ctypes
import os
import re

import pytest
import torch

from tests import emu_stream
from wesep_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_TOTAL = 1603
SMALL = dict(N=32, L=20, B=32, H=64, P=3, X=3, R=2, spk_emb_dim=256, causal=True, joint_training=False)
# the streamed configurations; joint SpEx+ needs N = 256: ResNet4SpExplus is hard-wired to 3 x 256 input channels
CONFIGS = {
    "multi_cln_concatconv": dict(SMALL, norm="cLN", spk_fuse_type="concatConv"),
    "plain_bn_skip_film_sigmoid": dict(SMALL, norm="BN", skip_con=True, spk_fuse_type="FiLM", activate="sigmoid",
                                       encoder_type="Plain", decoder_type="Plain", use_spk_transform=False),
    "multi_cln_joint_spexplus": dict(SMALL, N=256, norm="cLN", joint_training=True),
    "multi_bn_additive_skip": dict(SMALL, norm="BN", skip_con=True, spk_fuse_type="additive"),
    "plain_cln_multiply_relu": dict(SMALL, norm="cLN", spk_fuse_type="multiply", encoder_type="Plain", decoder_type="Plain"),
    "multi_cln_concat": dict(SMALL, norm="cLN", spk_fuse_type="concat", use_spk_transform=False),
}


def chunkings(total=T_TOTAL):
    g = torch.Generator().manual_seed(11)
    rnd, left = [], total
    while left > 0:
        n = min(left, int(torch.randint(1, 401, (1,), generator=g)))
        rnd.append(n)
        left -= n
    even = lambda n: [n] * (total // n) + ([total % n] if total % n else [])
    return {"all160": even(160), "all10": even(10), "all7": even(7), "random1to400": rnd, "one": [total]}


def make_case(name, rows, device="cpu", seed=5):
    """(model in eval mode, mixture [rows, T], enrollment) for one configuration; BatchNorm buffers are made non-trivial."""
    from wesep_amd.models import get_model
    torch.manual_seed(seed)
    kw = CONFIGS[name]
    model = get_model("ConvTasNet")(**kw)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 1.5)
    model = model.to(device).eval()
    x = torch.randn(rows, T_TOTAL, device=device)
    enroll = torch.randn(rows, 900 if kw["joint_training"] else 256, device=device)
    return model, x, enroll


def whole(model, x, enroll):
    """model(x, emb)[0] as [rows, T_out] (the plain ends' forward returns the same rows as [rows, 1, T_out])."""
    with torch.no_grad():
        out = model(x, enroll)
    return out.squeeze(1) if torch.is_tensor(out) else out[0]


def stream(st, x, sizes):
    """(concatenated pushes + flush, emitted sample count after every push)"""
    outs, counts, pos = [], [], 0
    for n in sizes:
        y = st.push(x[:, pos:pos + n])
        pos += n
        assert y.shape[0] == x.shape[0]
        outs.append(y)
        counts.append((pos, sum(o.shape[1] for o in outs)))
    outs.append(st.flush())
    return torch.cat(outs, 1), counts


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_stream_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    lib = L.lib()
    for name in ("ws_dwconv_stream_fwd", "ws_ola_stream_fwd"):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
        assert name in L.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    from wesep_amd import dev
    assert callable(dev.dwconv_stream_fwd) and callable(dev.ola_stream_fwd)
    assert lib.ws_abi_version() == 20 == L.ABI_VERSION          # new symbols only: the ABI number does not move
    assert re.search(r"^#define WS_ABI_VERSION 20\b", header, flags=re.M)


def test_stream_kernels_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    bufs = [(ctypes.c_float * 4096)() for _ in range(8)]
    x, st, gm, bt, w, b, ring, y = (ctypes.cast(v, ctypes.c_void_p) for v in bufs)
    err = lambda: lib.ws_last_error().decode()
    # ws_dwconv_stream_fwd(x, stats, gamma, beta, w, b, R, Tc, C, P, dil, st_div, t0, cap, ring, y, stream); bound: 2 * 4 + 5 = 13
    call = lambda *a: lib.ws_dwconv_stream_fwd(*a, None)
    assert call(x, st, gm, bt, w, b, 2, 5, 8, 3, 4, 1, 0, 12, ring, y) == -1 and "cap=12 is below (P - 1) * dil + Tc = 13" in err()
    assert call(x, st, gm, bt, w, b, 2, 5, 6, 3, 4, 1, 0, 13, ring, y) == -1 and "C=6 is not a multiple of 4" in err()
    assert call(x, st, gm, bt, w, b, 2, 5, 8, 3, 4, 1, -1, 13, ring, y) == -1 and "t0=-1 is negative" in err()
    assert call(x, st, gm, bt, w, b, 2, 5, 8, 3, 4, 1, 0, 13, None, y) == -1 and "ws_dwconv_stream_fwd: null pointer" in err()
    assert call(None, st, gm, bt, w, b, 2, 5, 8, 3, 4, 1, 0, 13, ring, y) == -1 and "null pointer" in err()
    assert call(x, st, gm, bt, w, b, 2, 5, 8, 4, 4, 1, 0, 17, ring, y) == -1 and "P=4 (odd P <= 7)" in err()
    assert call(x, st, gm, bt, w, b, 2, 5, 8, 9, 4, 1, 0, 37, ring, y) == -1 and "P=9 (odd P <= 7)" in err()
    assert call(x, st, gm, bt, w, b, 2, 5, 8, 3, 4, 1, 0, 13, ring, x) == -1 and "y overlaps x" in err()
    assert call(x, st, gm, bt, w, b, 2, 0, 8, 3, 4, 1, 0, 13, ring, y) == -1 and "bad geometry" in err()
    # ws_ola_stream_fwd(frames, bias, R, Tc, L, hop, carry, est, stream)
    ola = lambda *a: lib.ws_ola_stream_fwd(*a, None)
    assert ola(x, b, 2, 4, 25, 10, ring, y) == -1 and "L=25 is not a multiple of hop=10" in err()
    assert ola(x, b, 2, 4, 5, 10, ring, y) == -1 and "L=5 is not a multiple of hop=10" in err()
    assert ola(None, b, 2, 4, 20, 10, ring, y) == -1 and "frames or est is NULL" in err()
    assert ola(x, b, 2, 4, 20, 10, None, y) == -1 and "carry is NULL" in err()
    assert ola(x, b, 2, 0, 20, 10, ring, y) == -1 and "ws_ola_stream_fwd: bad args" in err()


# ---- the emulation itself: the ring and the carry against the whole-sequence entry points -------------------------------
@pytest.mark.parametrize("P,dil,extra", [(3, 1, 0), (3, 4, 0), (5, 2, 3)])
def test_emulated_ring_and_carry_match_the_whole_sequence(P, dil, extra):
    from tests import emu_dev
    torch.manual_seed(2)
    R, Cc, T = 2, 8, 37
    x = torch.randn(R, T, Cc)
    stats = torch.stack([x.mean(2).reshape(-1), 1 / torch.sqrt(x.var(2, unbiased=False).reshape(-1) + 1e-5)], 1).contiguous()
    gm, bt, w, b = torch.rand(Cc) + 0.5, torch.randn(Cc) * 0.1, torch.randn(Cc, P), torch.randn(Cc)
    ref = torch.empty(R * T, Cc)
    emu_dev.dwconv_fwd(x.reshape(R * T, Cc), stats, gm, bt, w, b, R, T, Cc, P, dil, 1, ref, causal=True)
    sizes = [3, 5, 1, 7, 2, 9, 4, 6]
    ring = torch.full((R, (P - 1) * dil + max(sizes) + extra, Cc), float("nan"))
    got, t0 = [], 0
    for n in sizes:
        yc = torch.empty(R * n, Cc)
        sc = stats.reshape(R, T, 2)[:, t0:t0 + n].reshape(-1, 2).contiguous()
        emu_stream.dwconv_stream_fwd(x[:, t0:t0 + n].reshape(R * n, Cc).contiguous(), sc, gm, bt, w, b, R, n, Cc, P, dil, 1, t0,
                                     ring, yc)
        got.append(yc.reshape(R, n, Cc))
        t0 += n
    got = torch.cat(got, 1)
    assert torch.isfinite(got).all() and rel(got, ref.reshape(R, T, Cc)) < 1e-6
    L_, hop, Tf = 40, 10, 16
    fr, bias = torch.randn(R, Tf, L_), torch.tensor([0.3])
    full = torch.empty(R, (Tf - 1) * hop + L_)
    emu_dev.ola_fwd(fr.reshape(R * Tf, L_), bias, R, Tf, L_, hop, full.shape[1], full)
    carry, outs, t = bias.expand(R, L_ - hop).clone(), [], 0
    for n in (1, 4, 2, 9):
        est = torch.empty(R, n * hop)
        emu_stream.ola_stream_fwd(fr[:, t:t + n].reshape(R * n, L_).contiguous(), bias, R, n, L_, hop, carry, est)
        outs.append(est)
        t += n
    assert rel(torch.cat(outs + [carry], 1), full) < 1e-6


# ---- the streamer on the emulation --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main_case():
    """The model of the issue (Multi ends, cLN, concatConv), its input and its whole-utterance estimate: computed once.
    The whole-utterance forward needs the emulation too, so it is installed with a module-scoped MonkeyPatch."""
    mp = pytest.MonkeyPatch()
    emu_stream.install(mp)
    model, x, emb = make_case("multi_cln_concatconv", 2)
    ref = whole(model, x, emb)
    mp.undo()
    return model, x, emb, ref


@pytest.mark.parametrize("chunking", sorted(chunkings()))
def test_streamer_matches_forward_for_any_chunking(chunking, main_case, monkeypatch):
    from wesep_amd.streaming import ConvTasNetStreamer
    emu_stream.install(monkeypatch)
    model, x, emb, ref = main_case
    sizes = chunkings()[chunking]
    assert sum(sizes) == T_TOTAL
    st = ConvTasNetStreamer(model, 2, max_chunk_frames=64)
    st.enroll(emb)
    assert st.latency_samples == 160 and st.state_bytes > 0
    got, counts = stream(st, x, sizes)
    s, Lmax = 10, 160
    for pushed, emitted in counts:                                   # the emission rule, after every push
        assert emitted == (max(0, (pushed - Lmax) // s + 1) * s if pushed >= Lmax else 0), (pushed, emitted)
    assert got.shape == ref.shape == (2, ((T_TOTAL - 20) // 10) * 10 + 20)
    e = rel(got, ref)
    print(f"stream {chunking}: rel L2 {e:.3e}")
    assert e < 1e-4, (chunking, e)


@pytest.mark.parametrize("name", [n for n in sorted(CONFIGS) if n != "multi_cln_concatconv"])
def test_streamer_covers_the_other_configurations(name, monkeypatch):
    from wesep_amd.streaming import ConvTasNetStreamer
    emu_stream.install(monkeypatch)
    monkeypatch.setattr("wesep_amd.functional_tasnet.SPK_MODE", None)
    model, x, enroll = make_case(name, 2)
    ref = whole(model, x, enroll)
    st = ConvTasNetStreamer(model, 2, max_chunk_frames=50)
    st.enroll(enroll)
    plain = CONFIGS[name].get("encoder_type") == "Plain"
    assert st.latency_samples == (20 if plain else 160)
    got, counts = stream(st, x, chunkings()["random1to400"])
    Lmax = st.latency_samples
    assert all(emitted == (max(0, (pushed - Lmax) // 10 + 1) * 10 if pushed >= Lmax else 0) for pushed, emitted in counts)
    assert got.shape == ref.shape
    e = rel(got, ref)
    print(f"stream {name}: rel L2 {e:.3e}")
    assert e < 1e-4, (name, e)
    st.reset()                                                      # the enrollment is kept; the same pushes, the same result
    again, _ = stream(st, x, chunkings()["random1to400"])
    assert torch.equal(again, got)


def test_small_pushes_flush_and_misuse(main_case, monkeypatch):
    from wesep_amd.streaming import ConvTasNetStreamer
    emu_stream.install(monkeypatch)
    model, x, emb, ref = main_case
    st = ConvTasNetStreamer(model, 2)
    with pytest.raises(L.WesepHipError, match="no enrollment yet"):
        st.push(x[:, :10])
    st.enroll(emb)
    y = st.push(x[:, :9])                                            # fewer than one hop
    assert y.shape == (2, 0) and y.dtype == torch.float32
    with pytest.raises(RuntimeError, match="input of 9 samples is shorter than the encoder window 20"):
        st.flush()
    assert st.push(x[:, 9:159]).shape == (2, 0)                      # 159 samples: no frame has its long window yet
    first = st.push(x[:, 159:160])
    assert first.shape == (2, 10) and st.frames_emitted == 1 and st.samples_pushed == 160
    with pytest.raises(ValueError, match=r"expected \[2, n >= 1\]"):
        st.push(x[:1, :10])
    with pytest.raises(ValueError, match="expected"):
        st.push(x[:, :0])
    tail = st.flush()                                                # 160 samples: T' = 15 frames, 160 samples in all
    assert tail.shape == (2, 150)
    with pytest.raises(L.WesepHipError, match="was flushed"):
        st.push(x[:, :10])
    with pytest.raises(L.WesepHipError, match="flushed already"):
        st.flush()
    short = whole(model, x[:, :160], emb)
    assert short.shape == (2, 160) and rel(torch.cat([first, tail], 1), short) < 1e-4
    st.reset()
    model.train()
    with pytest.raises(L.WesepHipError, match="training mode"):
        st.push(x[:, :10])
    model.eval()


def test_construction_refusals_name_their_reason():
    from wesep_amd.models import get_model
    from wesep_amd.streaming import ConvTasNetStreamer
    mk = lambda **kw: get_model("ConvTasNet")(**dict(SMALL, **kw)).eval()
    with pytest.raises(NotImplementedError, match="non-causal blocks look ahead"):
        ConvTasNetStreamer(mk(causal=False, norm="cLN"), 2)
    with pytest.raises(NotImplementedError, match="norm='gLN' takes its statistics over the whole utterance"):
        ConvTasNetStreamer(mk(norm="gLN"), 2)
    with pytest.raises(NotImplementedError, match="Deep ends cannot be streamed"):
        ConvTasNetStreamer(mk(norm="cLN", encoder_type="Deep", decoder_type="Deep"), 2)
    with pytest.raises(L.WesepHipError, match="training mode"):
        ConvTasNetStreamer(mk(norm="cLN").train(), 2)
    with pytest.raises(TypeError, match="a ConvTasNet is needed"):
        ConvTasNetStreamer(torch.nn.Linear(2, 2), 2)
    with pytest.raises(ValueError, match="must be positive"):
        ConvTasNetStreamer(mk(norm="cLN"), 0)
