"""CPU: `ConvTasNetStreamer(fused=True)` without a GPU -- the new symbol in the built library with its refusals, and the
host side of the fused path on the torch emulation of tests/emu_stream_fused.py against the SAME model's whole-utterance
forward.  The `fused=False` default must issue the launches it issued before: the recorded `dev` call names of a block
are compared with the sequence written down here.  Every test fails without the feature (no symbol, no keyword)."""
import ctypes
import os
import re

import pytest
import torch

from tests import emu_stream_fused
from tests.test_stream_tasnet_host_cpu import CONFIGS, SMALL, T_TOTAL, chunkings, make_case, rel, stream, whole
from wesep_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one block of the unfused streamer, as `dev` calls: GEMM, the five launches the fused kernel replaces, GEMM
UNFUSED_MID = ["prelu_fwd", "group_stats", "dwconv_stream_fwd", "prelu_fwd", "group_stats"]
FUSED_CONFIGS = {
    "multi_cln_concatconv": CONFIGS["multi_cln_concatconv"],
    "plain_cln_skip_film": dict(SMALL, norm="cLN", skip_con=True, spk_fuse_type="FiLM", encoder_type="Plain",
                                decoder_type="Plain", use_spk_transform=False),
    "multi_cln_joint_spexplus": CONFIGS["multi_cln_joint_spexplus"],
}


def make_fused_case(name, rows, device="cpu"):
    CONFIGS.setdefault(name, FUSED_CONFIGS[name])                   # make_case looks its configuration up by name
    return make_case(name, rows, device=device)


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    m = re.search(r"^int\s+ws_tcn_mid_stream_fwd\s*\(([^;]*)\);", header, flags=re.M)
    assert m, "ws_tcn_mid_stream_fwd is not declared in wesep_hip.h"
    res, args = L._SIGS["ws_tcn_mid_stream_fwd"]
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")) == 20
    assert "ws_tcn_mid_stream_fwd" in L.EXPORTED_SYMBOLS and L.lib().ws_tcn_mid_stream_fwd is not None
    from wesep_amd import dev
    assert callable(dev.tcn_mid_stream_fwd)
    assert L.lib().ws_abi_version() == 20 == L.ABI_VERSION          # a new symbol only
    assert re.search(r"^#define WS_TCN_MID_MAXH (\d+)", header, flags=re.M).group(1) == "4096"


def test_kernel_refuses_bad_arguments_before_any_launch():
    lib = L.lib()
    bufs = [(ctypes.c_float * 8192)() for _ in range(11)]
    c, rb, a1, g1, b1, wd, bd, a2, ring, y2, st2 = (ctypes.cast(v, ctypes.c_void_p) for v in bufs)
    err = lambda: lib.ws_last_error().decode()
    eps = ctypes.c_float(1e-5)

    def call(c=c, rb=rb, a1=a1, g1=g1, b1=b1, wd=wd, bd=bd, a2=a2, R=2, Tc=5, H=8, P=3, dil=4, t0=0, cap=13, ring=ring,
             y2=y2, st2=st2):
        return lib.ws_tcn_mid_stream_fwd(c, rb, a1, g1, b1, wd, bd, a2, R, Tc, H, P, dil, eps, t0, cap, ring, y2, st2, None)

    for name in ("c", "a1", "g1", "b1", "wd", "bd", "a2", "ring", "y2", "st2"):          # every pointer but rb
        assert call(**{name: None}) == -1 and "ws_tcn_mid_stream_fwd: null pointer" in err(), name
    assert call(H=6) == -1 and "H=6 is not a multiple of 4" in err()
    assert call(H=4100) == -1 and "H=4100 above 4096" in err()
    assert call(P=4, cap=17) == -1 and "P=4 (odd P <= 7)" in err()
    assert call(P=9, cap=37) == -1 and "P=9 (odd P <= 7)" in err()
    assert call(dil=0) == -1 and "bad geometry" in err()
    assert call(t0=-1) == -1 and "t0=-1 is negative" in err()
    assert call(cap=12) == -1 and "cap=12 is below (P - 1) * dil + Tc = 13" in err()
    assert call(y2=c) == -1 and "y2 overlaps c" in err()


@pytest.mark.parametrize("P,dil,extra,with_rb", [(3, 1, 0, True), (3, 4, 0, False), (5, 2, 3, True)])
def test_emulation_is_chunking_independent(P, dil, extra, with_rb):
    """The emulation itself: any chunking against one chunk with the whole sequence (the kernel's contract, to rounding)."""
    torch.manual_seed(3)
    R, H, T = 2, 8, 37
    c, rb = torch.randn(R * T, H) * 1.5 + 0.3, torch.randn(R, H) if with_rb else None
    a1, a2 = torch.tensor([0.2]), torch.tensor([0.35])
    gm, bt, wd, bd = torch.rand(H) + 0.5, torch.randn(H) * 0.1, torch.randn(H, P) * 0.5, torch.randn(H) * 0.1

    def run(sizes):
        ring = torch.full((R, (P - 1) * dil + max(sizes) + extra, H), float("nan"))
        ys, ss, t0 = [], [], 0
        for n in sizes:
            y2, st2 = torch.empty(R * n, H), torch.empty(R * n, 2)
            emu_stream_fused.tcn_mid_stream_fwd(c.view(R, T, H)[:, t0:t0 + n].reshape(R * n, H).contiguous(), rb, a1, gm, bt,
                                                wd, bd, a2, R, n, H, P, dil, 1e-5, t0, ring, y2, st2)
            ys.append(y2.view(R, n, H))
            ss.append(st2.view(R, n, 2))
            t0 += n
        return torch.cat(ys, 1), torch.cat(ss, 1)

    y_ref, s_ref = run([T])
    for sizes in ([1] * 37, [3, 5, 1, 7, 2, 9, 4, 6], [20, 17]):
        y, s = run(sizes)
        assert torch.isfinite(y).all() and rel(y, y_ref) < 1e-6 and rel(s, s_ref) < 1e-5


_REF = {}


def _case(name):
    """(model, x, enrollment, whole-utterance estimate) on the emulation: computed once per configuration."""
    if name not in _REF:
        mp = pytest.MonkeyPatch()
        emu_stream_fused.install(mp)
        mp.setattr("wesep_amd.functional_tasnet.SPK_MODE", None)
        model, x, enroll = make_fused_case(name, 2)
        _REF[name] = (model, x, enroll, whole(model, x, enroll))
        mp.undo()
    return _REF[name]


@pytest.mark.parametrize("chunking", ["all160", "all7", "random1to400", "one"])
@pytest.mark.parametrize("name", sorted(FUSED_CONFIGS))
def test_fused_streamer_matches_forward(name, chunking, monkeypatch):
    from wesep_amd.streaming import ConvTasNetStreamer
    emu_stream_fused.install(monkeypatch)
    monkeypatch.setattr("wesep_amd.functional_tasnet.SPK_MODE", None)
    model, x, enroll, ref = _case(name)
    st = ConvTasNetStreamer(model, 2, max_chunk_frames=64, fused=True)
    st.enroll(enroll)
    got, counts = stream(st, x, chunkings()[chunking])
    Lmax = st.latency_samples
    assert all(emitted == (max(0, (pushed - Lmax) // 10 + 1) * 10 if pushed >= Lmax else 0) for pushed, emitted in counts)
    assert got.shape == ref.shape == (2, ((T_TOTAL - 20) // 10) * 10 + 20) and float(ref.abs().max()) > 0
    e = rel(got, ref)
    print(f"fused stream {name} {chunking}: rel L2 {e:.3e}")
    assert e < 1e-4, (name, chunking, e)


def _recorded_names(model, x, enroll, monkeypatch, **kw):
    from wesep_amd.streaming import ConvTasNetStreamer
    record = []
    with monkeypatch.context() as mp:
        emu_stream_fused.install(mp, record)
        mp.setattr("wesep_amd.functional_tasnet.SPK_MODE", None)
        st = ConvTasNetStreamer(model, 2, max_chunk_frames=64, **kw)
        st.enroll(enroll)
        del record[:]
        st.push(x[:, :400])                                         # 25 frames: one group
        out = list(record)
    return out


def _collapse(names):
    """The unfused record with every block's five middle launches replaced by the fused one; the number replaced."""
    out, i, n = [], 0, 0
    while i < len(names):
        if names[i:i + 5] == UNFUSED_MID:
            out.append("tcn_mid_stream_fwd")
            i, n = i + 5, n + 1
        else:
            out.append(names[i])
            i += 1
    return out, n


@pytest.mark.parametrize("name", ["multi_cln_concatconv", "plain_cln_skip_film"])
def test_default_launch_sequence_is_unchanged_and_fused_replaces_five_per_block(name, monkeypatch):
    model, x, enroll, _ = _case(name)
    default = _recorded_names(model, x, enroll, monkeypatch)
    unfused = _recorded_names(model, x, enroll, monkeypatch, fused=False)
    fused = _recorded_names(model, x, enroll, monkeypatch, fused=True)
    nblocks = SMALL["X"] * SMALL["R"]
    assert default == unfused and "tcn_mid_stream_fwd" not in unfused
    expect, n = _collapse(unfused)
    assert n == nblocks                                              # every block issued GEMM, the five, GEMM
    for i in [k for k in range(len(unfused)) if unfused[k:k + 5] == UNFUSED_MID]:
        assert unfused[i - 1] == "gemm_nt" and unfused[i + 5] == "gemm_nt"
    assert fused == expect and len(unfused) - len(fused) == 4 * nblocks


def test_fused_refuses_bn_by_name(monkeypatch):
    from wesep_amd import functional_tasnet as FT
    from wesep_amd.models import get_model
    from wesep_amd.streaming import ConvTasNetStreamer
    emu_stream_fused.install(monkeypatch)
    model = get_model("ConvTasNet")(**dict(SMALL, norm="BN")).eval()
    with pytest.raises(NotImplementedError, match="BN"):
        ConvTasNetStreamer(model, 2, fused=True)
    ConvTasNetStreamer(model, 2, fused=False)
    with pytest.raises(NotImplementedError, match="norm='BN'"):     # refused before any argument is touched
        FT.conv_block_stream(torch.zeros(4, 8), None, (2, 2, "BN", 1, None), None, 0, *([None] * 12), fused=True)
