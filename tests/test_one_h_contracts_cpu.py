"""CPU: argument-contract dry run (tests/abi_dryrun.py) of the training step with h as two fp16 planes (WESEP_H2P=1: on a
machine without a GPU the format is off unless asked for, dev.h2p_on): the new entry point ws_gemm_tnb_h16 and the new values of
existing fields (ws_gemm_b2p a_fmt 4, ws_lstm_fused_args.hfmt bit 3, ws_lstm_cluster2_args.rfmt bit 1, ws_lstm_args.rfmt 16) must
pass every entry point's validation on the host paths that select them, and the library still speaks ABI 20."""
import pytest
import torch

from tests import abi_dryrun
from tests.test_abi_contracts_cpu import _check, _fwd_bwd

if torch.cuda.is_available():
    pytest.skip("argument-contract dry run is for GPU-less machines", allow_module_level=True)


def _spy(monkeypatch, name, seen):
    import wesep_amd.dev as dev
    real = getattr(dev, name)

    def fn(*a, **k):
        seen.append((name, k.get("hfmt", k.get("a_fmt", k.get("h2p")))))
        return real(*a, **k)
    monkeypatch.setattr(dev, name, fn)


@pytest.mark.parametrize("R,T", [(2, 16000), (32, 8192)])
def test_bsrnn_step_with_h_in_fp16_planes_contracts(monkeypatch, R, T):
    """R = 2: the streaming / fused branches; R = 32 (the headline row count): 1024 time-view sequences take the cluster2 branch
    with its predicated fall-back, the band view the fused kernel."""
    from wesep_amd import _lib as L
    from wesep_amd.models import get_model
    monkeypatch.setenv("WESEP_H2P", "1")
    calls = abi_dryrun.install(monkeypatch)
    seen = []
    for name in ("lstm_fwd_fused", "gemm_b2p", "lstm_fwd", "lstm_fwd_cluster2", "gemm_tnb_h16"):
        _spy(monkeypatch, name, seen)
    model = get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, joint_training=False)
    _fwd_bwd(model, torch.randn(R, T), torch.randn(R, 256))
    used = _check(calls, 30)
    assert L.lib().ws_abi_version() == 20
    assert {"ws_gemm_tnb_h16", "ws_gemm_tnb", "ws_gemm_b2p"} <= used
    assert ("gemm_b2p", 4) in seen and any(n == "gemm_tnb_h16" for n, _ in seen)
    assert any(n == "lstm_fwd_fused" and v & 8 for n, v in seen) or any(n == "lstm_fwd" and v for n, v in seen)
    if R == 32:
        assert ("lstm_fwd_cluster2", True) in seen and ("lstm_fwd", True) in seen


def test_the_pair_format_stays_selectable(monkeypatch):
    from wesep_amd.models import get_model
    monkeypatch.setenv("WESEP_H2P", "0")
    calls = abi_dryrun.install(monkeypatch)
    model = get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, joint_training=False)
    _fwd_bwd(model, torch.randn(2, 16000), torch.randn(2, 256))
    used = _check(calls, 30)
    assert "ws_gemm_tnb_h16" not in used and "ws_gemm_tnb" in used
