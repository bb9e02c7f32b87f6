"""GPU: the native runtime's ResNet launch plan with MHASTP / MQMHASTP pooling (runtime/speaker.cc, meta spk_pool) against
the Python module tree in eval mode on the same device: a pBSRNN with ResNet34-MQMHASTP and a DPCCN with ResNet50-MHASTP."""
import numpy as np
import pytest
import torch

from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu


def _randomise_buffers(model):
    with torch.no_grad():                                   # non-trivial BatchNorm running statistics
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0.0, 0.2)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)


def _check(model, eng, d, seed):
    from tests.test_engine_gpu import rel
    g = torch.Generator().manual_seed(seed)
    for R, Te in ((2, 120), (3, 77)):
        wav = 0.1 * torch.randn(R, 12000, generator=g)
        fbank = torch.randn(R, Te, 80, generator=g)
        fbank = fbank - fbank.mean(1, keepdim=True)
        est = eng.separate(wav.numpy(), fbank.numpy(), E.ENROLL_FBANK)
        with torch.no_grad():
            ref = model(wav.to(d), fbank.to(d))[0]
        err = rel(est, ref)
        print(f"engine pooling R={R} Te={Te}: rel {err:.2e}")
        assert np.isfinite(est).all() and err < 1e-4, (R, Te, err)


def test_engine_bsrnn_resnet34_mqmhastp_matches_python(tmp_path):
    from tests.test_engine_gpu import _cuda, _joint
    d = _cuda()
    model, eng = _joint(tmp_path, "ResNet34", d, seed=17,
                        spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="MQMHASTP", two_emb_layer=False))
    assert eng.info("spk_pool") == 2 and eng.info("spk_pool_heads") == 8
    _check(model, eng, d, 7)
    eng.close()


def test_engine_dpccn_resnet50_mhastp_matches_python(tmp_path):
    from tests.test_engine_gpu import _cuda
    from wesep_amd.models import get_model
    d = _cuda()
    torch.manual_seed(19)
    model = get_model("DPCCN")(tcn_blocks=2, tcn_layers=2, spk_emb_dim=256, joint_training=True, spk_model="ResNet50",
                               spk_feat=True, spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="MHASTP",
                                                            two_emb_layer=False))
    _randomise_buffers(model)
    path = str(tmp_path / "d.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    assert eng.info("arch") == 2 and eng.info("spk_pool") == 1 and eng.info("spk_bottleneck") == 1
    _check(model.to(d).eval(), eng, d, 8)
    eng.close()
