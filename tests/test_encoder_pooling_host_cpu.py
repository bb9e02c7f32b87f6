"""CPU: every wespeaker pooling layer in the 1-D speaker encoders (ECAPA-TDNN, CAM++; models/ecapa_tdnn.py,
models/campplus.py) -- the module tree and `state_dict` names against the restatement (tests/encoder_pooling_ref.py,
including CAM++'s pool.* / xvector.stats.* aliases), strict loads, the argument contracts of a jointly trained step
(tests/abi_dryrun.py, the split MHASTP entry points among them), the export and the native runtime's launch plan (dry
run), containers written before spk_pool existed, and the pool geometries the kernels refuse.  Numerics are on the GPU
(tests/test_encoder_pooling_gpu.py, tests/test_zz_engine_encoder_pooling_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import abi_dryrun
from tests import encoder_pooling_ref as ER

needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="dry runs are for GPU-less machines")
ENCODERS = ("ECAPA_TDNN_c512", "ECAPA_TDNN_GLOB_c1024", "CAMPPlus")
SPLIT_ENTRY_POINTS = {"ws_mhastp_fwd_split", "ws_mhastp_bwd_split"}


def _encoder(name, pool):
    from wesep_amd.models.resnet import get_speaker_model
    if name == "CAMPPlus":
        return get_speaker_model(name)(feat_dim=80, embed_dim=512, pooling_func=pool)
    return get_speaker_model(name)(feat_dim=80, embed_dim=192, pooling_func=pool)


def _restated(name, pool, seed=0):
    if name == "CAMPPlus":
        return ER.campplus_state_dict(pool, seed=seed)
    return ER.ecapa_state_dict(pool, channels=1024 if "c1024" in name else 512, glob="GLOB" in name, seed=seed)


def _bsrnn(spk_model, pool, **kw):
    from wesep_amd.models import get_model
    E = 512 if spk_model == "CAMPPlus" else 192
    return get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                              joint_training=True, spk_feat=True, spk_model=spk_model, spk_emb_dim=E,
                              spk_args=dict(feat_dim=80, embed_dim=E, pooling_func=pool), **kw)


@pytest.mark.parametrize("name", ENCODERS)
@pytest.mark.parametrize("pool", ER.POOLS)
def test_state_dict_matches_the_restatement(name, pool):
    ours = {k: tuple(v.shape) for k, v in _encoder(name, pool).state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in _restated(name, pool)[0].items()}
    assert ours == ref
    D = ER.make_pool(pool, 512 if name == "CAMPPlus" else 1536).get_out_dim()
    if name == "CAMPPlus":
        assert ours["xvector.dense.linear.weight"] == (512, D, 1)
        pool_keys = sorted(k[len("pool."):] for k in ours if k.startswith("pool."))
        assert pool_keys == sorted(k[len("xvector.stats."):] for k in ours if k.startswith("xvector.stats."))
        assert bool(pool_keys) == (pool in ("ASTP", "MHASTP", "MQMHASTP"))
    else:
        assert ours["bn.weight"] == (D,) and ours["linear.weight"] == (192, D)
    if pool == "MQMHASTP":
        dm = (512 if name == "CAMPPlus" else 1536) // 8
        assert ours["pool.n_query.1.heads_att_trans.7.att_1.weight"] == (dm, 64, 1)


@pytest.mark.parametrize("name", ENCODERS)
@pytest.mark.parametrize("pool", ("ASTP", "MHASTP", "MQMHASTP", "TAP"))
def test_restatement_checkpoint_loads(name, pool):
    ref, _ = _restated(name, pool, seed=3)
    enc = _encoder(name, pool)
    enc.load_state_dict(ref, strict=True)
    sd = enc.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in ref.items())
    if name == "CAMPPlus" and pool != "TAP":       # one object under two names
        assert enc.pool is enc.xvector.stats


def test_ecapa_global_context_reaches_astp_only():
    from wesep_amd.models.ecapa_tdnn import ECAPA_TDNN_GLOB_c512
    assert ECAPA_TDNN_GLOB_c512(80, 192, pooling_func="ASTP").pool.linear1.in_channels == 3 * 1536
    assert ECAPA_TDNN_GLOB_c512(80, 192, pooling_func="MHASTP").pool.d_model == 768


@pytest.mark.skipif(torch.cuda.is_available(), reason="argument-contract dry run is for GPU-less machines")
@pytest.mark.parametrize("spk_model,pool", [("ECAPA_TDNN_c512", "MHASTP"), ("CAMPPlus", "MQMHASTP")])
def test_joint_training_step_contracts(monkeypatch, spk_model, pool):
    calls = abi_dryrun.install(monkeypatch)
    model = _bsrnn(spk_model, pool).train()
    est, _ = model(torch.randn(2, 8000), torch.randn(2, 120, 80))
    est.sum().backward()
    assert all(p.grad is not None for p in model.spk_model.pool.parameters())
    abi_dryrun.assert_contracts_hold(calls, 100)
    names = {w for w, _, _ in calls}
    assert SPLIT_ENTRY_POINTS <= names
    assert not {"ws_mhastp_fwd", "ws_mhastp_bwd"} & names          # the 1-D encoders use the split grid only


@needs_no_gpu
@pytest.mark.parametrize("spk_model,pool", [(m, p) for m in ("ECAPA_TDNN_c512", "CAMPPlus") for p in ER.POOLS])
def test_export_and_engine_dry_run(tmp_path, spk_model, pool):
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import SPK_POOL, export_engine
    path = str(tmp_path / "p.wsw")
    export_engine(_bsrnn(spk_model, pool).eval(), path)
    eng = E.Engine(path, dry_run=True)
    assert eng.info("spk_kind") == (2 if spk_model == "CAMPPlus" else 1)
    assert eng.info("spk_pool") == SPK_POOL[pool]
    if pool in ("MHASTP", "MQMHASTP"):
        assert eng.info("spk_pool_queries") == (2 if pool == "MQMHASTP" else 1)
        assert eng.info("spk_pool_heads") == (8 if pool == "MQMHASTP" else 2)
    for frames in (40, 98, 1001):                                     # 0.4 s, 1 s, 10 s of enrollment
        eng.separate(np.zeros((1, 16000), np.float32), np.zeros((1, frames, 80), np.float32), E.ENROLL_FBANK)
    eng.close()


@needs_no_gpu
@pytest.mark.parametrize("spk_model,default", [("ECAPA_TDNN_c512", 3), ("CAMPPlus", 0)])
def test_containers_without_spk_pool_keep_the_default(tmp_path, spk_model, default):
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import engine_meta, write_container
    model = _bsrnn(spk_model, "ASTP" if default == 3 else "TSTP").eval()
    meta = engine_meta(model)
    assert meta.pop("spk_pool") == default
    path = str(tmp_path / "old.wsw")
    write_container(path, meta, model.state_dict())
    eng = E.Engine(path, dry_run=True)
    assert eng.info("spk_pool") == default
    eng.separate(np.zeros((1, 16000), np.float32), np.zeros((1, 98, 80), np.float32), E.ENROLL_FBANK)
    eng.close()


@needs_no_gpu
def test_engine_refuses_a_pool_without_its_tensors(tmp_path):
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import engine_meta, write_container
    model = _bsrnn("CAMPPlus", "ASTP")
    state = {k: v for k, v in model.state_dict().items() if not k.startswith("spk_model.pool.linear2")}
    path = str(tmp_path / "bad.wsw")
    write_container(path, engine_meta(model), state)
    with pytest.raises(E.WesepHipError, match="pool.linear2"):
        E.Engine(path, dry_run=True)


def test_unbuilt_pool_geometries_raise():
    from wesep_amd.models.campplus import CAMPPlus
    from wesep_amd.models.ecapa_tdnn import ECAPA_TDNN_c512
    from wesep_amd.models.resnet import MHASTP
    with pytest.raises(NotImplementedError, match="pooling_func 'SAP'"):
        ECAPA_TDNN_c512(80, 192, pooling_func="SAP")
    with pytest.raises(NotImplementedError, match="pooling_func 'XVEC'"):
        CAMPPlus(pooling_func="XVEC")
    with pytest.raises(NotImplementedError, match="LDS"):             # one head of 16384 features a frame
        MHASTP(in_dim=16384, head_num=1).check_channels(16384)
    with pytest.raises(NotImplementedError, match="layer_num"):
        MHASTP(in_dim=512, layer_num=3)


def test_the_issue_examples_build():
    """`CAMPPlus(pooling_func="MQMHASTP")` and `ECAPA_TDNN_c512(80, 192, pooling_func="MHASTP")` -- both raised before."""
    from wesep_amd.models.campplus import CAMPPlus
    from wesep_amd.models.ecapa_tdnn import ECAPA_TDNN_c512
    cam = CAMPPlus(pooling_func="MQMHASTP")
    assert cam.pool_out_dim == 2 * 2 * 512 and cam.xvector.stats is cam.pool
    ec = ECAPA_TDNN_c512(80, 192, pooling_func="MHASTP")
    assert ec.pool_out_dim == 2 * 1536 and ec.pool.head_num == 2 and ec.pool.d_s == 1


def test_split_sizes_cover_the_chip():
    from wesep_amd import dev
    n, part = dev.mhastp_split_sizes(32, 1, 398, 1536, 1, 2, 256)      # ECAPA MHASTP at the joint shape: 64 (row, head)
    assert 64 * n >= 256 and n * 16 <= 398 + 15 and part == n * 32 * 2 * 4 * 768
    assert dev.mhastp_split_sizes(1, 1, 1, 512, 2, 8, 256)[0] == 1         # one frame: one split
    assert dev.mhastp_split_sizes(1024, 1, 1000, 512, 1, 2, 256)[0] == 1  # enough rows already
    from wesep_amd._lib import WesepHipError
    with pytest.raises(WesepHipError, match="ws_mhastp_split_sizes"):
        dev.mhastp_split_sizes(1, 1, 10, 510, 1, 4, 256)                  # 4 heads do not divide 510
