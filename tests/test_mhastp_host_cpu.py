"""CPU: MHASTP / MQMHASTP pooling of the wespeaker ResNet encoders (models/resnet.py) -- the module tree and
`state_dict` names against the restatement (tests/pooling_ref.py), the argument contracts of the new entry points in a
jointly trained step (tests/abi_dryrun.py), the export and the native runtime's launch plan (dry run), and the
configurations the kernels refuse.  Numerics are on the GPU (tests/test_mhastp_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import abi_dryrun
from tests import pooling_ref as PR

needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="dry runs are for GPU-less machines")
CASES = [("ResNet34", "MQMHASTP"), ("ResNet50", "MHASTP")]
NEW_ENTRY_POINTS = {"ws_mhastp_pack", "ws_mhastp_fwd", "ws_mhastp_bwd"}


def _bsrnn(spk_model, pool, **kw):
    from wesep_amd.models import get_model
    return get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                              joint_training=True, spk_feat=True, spk_model=spk_model,
                              spk_args=dict(feat_dim=80, embed_dim=256, pooling_func=pool, two_emb_layer=False), **kw)


@pytest.mark.parametrize("spk_model,pool", CASES)
def test_state_dict_matches_the_restatement(spk_model, pool):
    model = _bsrnn(spk_model, pool)
    ours = {k: tuple(v.shape) for k, v in model.spk_model.state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in PR.ResNetPooled(spk_model, pooling_func=pool).state_dict_encoder().items()}
    assert ours == ref
    in_dim = 2560 * (4 if spk_model == "ResNet50" else 1)
    q = 2 if pool == "MQMHASTP" else 1
    assert model.spk_model.seg_1.weight.shape == (256, q * 2 * in_dim)
    assert model.spk_model.pool.get_out_dim() == q * 2 * in_dim
    if pool == "MQMHASTP":
        assert ours["pool.n_query.1.heads_att_trans.7.att_0.weight"] == (64, 320, 1)
        assert ours["pool.n_query.1.heads_att_trans.7.att_1.weight"] == (320, 64, 1)
    else:
        assert ours["pool.heads_att_trans.1.att_0.weight"] == (64, 5120, 1)
        assert ours["pool.heads_att_trans.1.att_1.weight"] == (1, 64, 1)


@pytest.mark.parametrize("spk_model,pool", CASES)
def test_restatement_checkpoint_loads(spk_model, pool):
    from wesep_amd.models.resnet import get_speaker_model
    ref = PR.ResNetPooled(spk_model, pooling_func=pool, seed=3).state_dict_encoder()
    enc = get_speaker_model(spk_model)(feat_dim=80, embed_dim=256, pooling_func=pool, two_emb_layer=False)
    enc.load_state_dict(ref, strict=True)
    sd = enc.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in ref.items())


@pytest.mark.skipif(torch.cuda.is_available(), reason="argument-contract dry run is for GPU-less machines")
@pytest.mark.parametrize("spk_model,pool", CASES)
def test_joint_training_step_contracts(monkeypatch, spk_model, pool):
    calls = abi_dryrun.install(monkeypatch)
    model = _bsrnn(spk_model, pool).train()
    est, _ = model(torch.randn(2, 8000), torch.randn(2, 120, 80))
    est.sum().backward()
    assert all(p.grad is not None for p in model.spk_model.pool.parameters())
    abi_dryrun.assert_contracts_hold(calls, 100)
    assert NEW_ENTRY_POINTS <= {w for w, _, _ in calls}


@pytest.mark.skipif(torch.cuda.is_available(), reason="argument-contract dry run is for GPU-less machines")
def test_frozen_pool_contracts(monkeypatch):
    """No weight gradients asked for: the backward is the dx launch alone (no workspace, no slabs)."""
    calls = abi_dryrun.install(monkeypatch)
    model = _bsrnn("ResNet34", "MQMHASTP").train()
    for p in model.spk_model.pool.parameters():
        p.requires_grad_(False)
    est, _ = model(torch.randn(2, 8000), torch.randn(2, 120, 80))
    est.sum().backward()
    assert all(p.grad is None for p in model.spk_model.pool.parameters())
    abi_dryrun.assert_contracts_hold(calls, 100)
    assert "ws_mhastp_bwd" in {w for w, _, _ in calls}


@needs_no_gpu
@pytest.mark.parametrize("spk_model,pool", CASES)
def test_export_and_engine_dry_run(tmp_path, spk_model, pool):
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    path = str(tmp_path / "p.wsw")
    export_engine(_bsrnn(spk_model, pool), path)
    eng = E.Engine(path, dry_run=True)
    assert eng.info("feat_dim") == 80 and eng.info("spk_kind") == 0
    assert eng.info("spk_pool") == {"MHASTP": 1, "MQMHASTP": 2}[pool]
    assert eng.info("spk_pool_queries") == (2 if pool == "MQMHASTP" else 1)
    eng.separate(np.zeros((2, 16000), np.float32), np.zeros((2, 98, 80), np.float32), E.ENROLL_FBANK)
    eng.close()


@needs_no_gpu
def test_engine_refuses_a_pool_without_its_tensors(tmp_path):
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import engine_meta, write_container
    model = _bsrnn("ResNet34", "MQMHASTP")
    state = {k: v for k, v in model.state_dict().items() if "n_query.1." not in k}
    path = str(tmp_path / "bad.wsw")
    write_container(path, engine_meta(model), state)
    with pytest.raises(E.WesepHipError, match="n_query.1"):
        E.Engine(path, dry_run=True)


def test_unsupported_configurations_raise():
    from wesep_amd.models.resnet import MHASTP, MQMHASTP, ResNet34, ResNet50
    with pytest.raises(NotImplementedError, match="layer_num"):
        MHASTP(in_dim=2560, layer_num=3)
    with pytest.raises(NotImplementedError, match="bottleneck_dim"):
        MQMHASTP(in_dim=2560, bottleneck_dim=128)
    MHASTP(in_dim=2560, layer_num=1, bottleneck_dim=128)          # layer_num 1 has no bottleneck
    with pytest.raises(NotImplementedError, match="does not divide"):
        MHASTP(in_dim=2560, head_num=5).check_channels(256)
    with pytest.raises(NotImplementedError, match="LDS"):        # ResNet50 with one head: 10240 features a frame
        MHASTP(in_dim=10240, head_num=1).check_channels(1024)
    assert ResNet34(80, 256, pooling_func="MHASTP").pool.d_model == 1280
    assert ResNet50(80, 256, pooling_func="MQMHASTP").pool.n_query[0].d_model == 1280
