"""GPU: the native runtime's ECAPA-TDNN and CAM++ launch plans with a non-default pooling layer (runtime/speaker.cc,
meta spk_pool; MHASTP / MQMHASTP on ws_mhastp_fwd_split) against the Python module tree in eval mode on the same device:
pBSRNN with ECAPA-MQMHASTP, CAM++-ASTP and CAM++-MQMHASTP, and a DPCCN with ECAPA-MHASTP."""
import pytest
import torch

from wesep_amd import engine as E
from wesep_amd.bin.export_engine import SPK_POOL, export_engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spk_model,pool", [("ECAPA_TDNN_c512", "MQMHASTP"), ("CAMPPlus", "ASTP"),
                                            ("CAMPPlus", "MQMHASTP")])
def test_engine_bsrnn_encoder_pool_matches_python(tmp_path, spk_model, pool):
    from tests.test_engine_gpu import _cuda, _joint
    from tests.test_zz_engine_pooling_gpu import _check
    d = _cuda()
    Ed = 512 if spk_model == "CAMPPlus" else 192
    model, eng = _joint(tmp_path, spk_model, d, seed=29, spk_emb_dim=Ed,
                        spk_args=dict(feat_dim=80, embed_dim=Ed, pooling_func=pool))
    assert eng.info("spk_kind") == (2 if spk_model == "CAMPPlus" else 1) and eng.info("spk_pool") == SPK_POOL[pool]
    _check(model, eng, d, 11)
    eng.close()


def test_engine_dpccn_ecapa_mhastp_matches_python(tmp_path):
    from tests.test_engine_gpu import _cuda
    from tests.test_zz_engine_pooling_gpu import _check, _randomise_buffers
    from wesep_amd.models import get_model
    d = _cuda()
    torch.manual_seed(31)
    model = get_model("DPCCN")(tcn_blocks=2, tcn_layers=2, spk_emb_dim=192, joint_training=True,
                               spk_model="ECAPA_TDNN_c512", spk_feat=True,
                               spk_args=dict(feat_dim=80, embed_dim=192, pooling_func="MHASTP"))
    _randomise_buffers(model)
    path = str(tmp_path / "d.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    assert eng.info("arch") == 2 and eng.info("spk_kind") == 1 and eng.info("spk_pool") == SPK_POOL["MHASTP"]
    _check(model.to(d).eval(), eng, d, 12)
    eng.close()
