"""TEST INFRASTRUCTURE ONLY -- fp64 CPU restatements for the pooling choices of the 1-D speaker encoders (ECAPA-TDNN,
CAM++; models/ecapa_tdnn.py, models/campplus.py): wespeaker's TSTP / TAP / TSDP / ASTP pooling layers (pooling_layers.py,
as recalled from the upstream source; MHASTP / MQMHASTP come from tests/pooling_ref.py), the two trunks up to the pool
(restated from oracle/ecapa_oracle.py and oracle/campplus_oracle.py, which end in their default pools), and the
state_dict of an encoder with any of the six pools.  Parity UNPINNED like the rest of the encoders.

    TSTP: mean || sqrt(var_unbiased + 1e-7)        TAP: mean        TSDP: sqrt(var_unbiased + 1e-7)
    ASTP(in_dim, bottleneck_dim=128, global_context_att=False):
        a = tanh(linear1(x or cat(x, mean, std))); alpha = softmax_T(linear2(a))
        mean = sum alpha x; out = mean || sqrt((sum alpha x^2 - mean^2).clamp(min=1e-7))
    ECAPA-TDNN: pool = getattr(pooling_layers, name)(in_dim=1536, global_context_att=...); bn and linear over
        pool.get_out_dim().  CAM++: pool = getattr(pooling_layers, name)(in_dim=512), registered as `pool` and as
        `xvector.stats` (one object: its tensors appear under both prefixes); xvector.dense over get_out_dim()."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import campplus_oracle as CO
from oracle import ecapa_oracle as EO
from tests import pooling_ref as PR

POOLS = ("TSTP", "TAP", "TSDP", "ASTP", "MHASTP", "MQMHASTP")


class TSTP(nn.Module):
    def __init__(self, in_dim=0, **kwargs):
        super().__init__()
        self.in_dim = in_dim

    def get_out_dim(self):
        return 2 * self.in_dim

    def forward(self, x):
        return torch.cat([x.mean(-1), torch.sqrt(torch.var(x, dim=-1) + 1e-7)], 1)


class TAP(TSTP):
    def get_out_dim(self):
        return self.in_dim

    def forward(self, x):
        return x.mean(-1)


class TSDP(TSTP):
    def get_out_dim(self):
        return self.in_dim

    def forward(self, x):
        return torch.sqrt(torch.var(x, dim=-1) + 1e-7)


class ASTP(nn.Module):
    def __init__(self, in_dim, bottleneck_dim=128, global_context_att=False, **kwargs):
        super().__init__()
        self.in_dim, self.global_context_att = in_dim, global_context_att
        self.linear1 = nn.Conv1d(in_dim * 3 if global_context_att else in_dim, bottleneck_dim, kernel_size=1)
        self.linear2 = nn.Conv1d(bottleneck_dim, in_dim, kernel_size=1)

    def get_out_dim(self):
        return 2 * self.in_dim

    def forward(self, x):
        if self.global_context_att:
            mean = x.mean(-1, keepdim=True).expand_as(x)
            std = torch.sqrt(torch.var(x, dim=-1, keepdim=True) + 1e-7).expand_as(x)
            a_in = torch.cat((x, mean, std), 1)
        else:
            a_in = x
        alpha = torch.softmax(self.linear2(torch.tanh(self.linear1(a_in))), dim=2)
        mean = torch.sum(alpha * x, dim=2)
        var = torch.sum(alpha * x ** 2, dim=2) - mean ** 2
        return torch.cat([mean, torch.sqrt(var.clamp(min=1e-7))], 1)


def make_pool(name, in_dim, seed=0, **kwargs):
    """The restated pooling layer with seeded weights (fan-in scaled; biases small), fp64."""
    cls = {"TSTP": TSTP, "TAP": TAP, "TSDP": TSDP, "ASTP": ASTP, "MHASTP": PR.MHASTP, "MQMHASTP": PR.MQMHASTP}[name]
    pool = cls(in_dim=in_dim, **kwargs).double()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in pool.named_parameters():
            p.copy_(0.05 * torch.randn(p.shape, generator=g, dtype=torch.float64) if k.endswith("bias") else
                    torch.randn(p.shape, generator=g, dtype=torch.float64) * (1.0 / p.shape[1]) ** 0.5)
    return pool


def ecapa_state_dict(pool_name, channels=512, embed_dim=192, glob=False, seed=0):
    """(state_dict of ECAPA_TDNN with `pool_name`, the restated pool): the trunk from ecapa_oracle.synth_params, pool.*
    from the restatement, bn / linear sized by the pool's output."""
    pool = make_pool(pool_name, 1536, seed + 1, global_context_att=glob)
    D = pool.get_out_dim()
    sd = {k: v for k, v in EO.synth_params(seed, channels=channels, embed_dim=embed_dim, global_context_att=glob).items()
          if not k.startswith(("pool.", "bn.", "linear."))}
    g = torch.Generator().manual_seed(seed + 2)
    sd.update({"bn.weight": 1.0 + 0.1 * torch.randn(D, generator=g), "bn.bias": 0.1 * torch.randn(D, generator=g),
               "bn.running_mean": torch.zeros(D), "bn.running_var": torch.ones(D),
               "bn.num_batches_tracked": torch.zeros((), dtype=torch.long),
               "linear.weight": torch.randn(embed_dim, D, generator=g) * (1.0 / D) ** 0.5,
               "linear.bias": 0.05 * torch.randn(embed_dim, generator=g)})
    for k, v in pool.state_dict().items():
        sd["pool." + k] = v.float()
    return sd, pool


def campplus_state_dict(pool_name, embed_dim=512, seed=0, **kw):
    """(state_dict of CAMPPlus with `pool_name`, the restated pool): pool tensors under pool.* AND xvector.stats.*."""
    sd = CO.synth_params(seed, embed_dim=embed_dim, **kw)
    c = sd["xvector.out_nonlinear.batchnorm.running_mean"].shape[0]
    pool = make_pool(pool_name, c, seed + 1)
    D = pool.get_out_dim()
    g = torch.Generator().manual_seed(seed + 2)
    sd["xvector.dense.linear.weight"] = torch.randn(embed_dim, D, 1, generator=g) * (2.0 / D) ** 0.5
    for k, v in pool.state_dict().items():
        sd["pool." + k] = v.float()
        sd["xvector.stats." + k] = v.float()
    return sd, pool


def ecapa_trunk(p, x, scale=8, training=True):
    """oracle.ecapa_oracle.ecapa_forward up to the pooling: x [B, T, F] -> h [B, 1536, T]."""
    def bn(name, y):
        return F.batch_norm(y, p[name + ".running_mean"].clone(), p[name + ".running_var"].clone(), p[name + ".weight"],
                            p[name + ".bias"], training, EO.BN_MOMENTUM, EO.BN_EPS)

    def crb(name, y, dil=1):
        w = p[name + ".conv.weight"]
        k = w.shape[2]
        return bn(name + ".bn", F.relu(F.conv1d(y, w, p[name + ".conv.bias"], padding=dil * (k // 2), dilation=dil)))

    cur = crb("layer1", x.permute(0, 2, 1))
    outs = []
    for li, dil in ((2, 2), (3, 3), (4, 4)):
        q = f"layer{li}.se_res2block."
        h = crb(q + "0", cur)
        width = h.shape[1] // scale
        spx = torch.split(h, width, 1)
        parts, sp = [], None
        for i in range(scale - 1):
            sp = spx[i] if i == 0 else sp + spx[i]
            sp = F.conv1d(sp, p[q + f"1.convs.{i}.weight"], p[q + f"1.convs.{i}.bias"], padding=dil, dilation=dil)
            sp = bn(q + f"1.bns.{i}", F.relu(sp))
            parts.append(sp)
        parts.append(spx[scale - 1])
        h = crb(q + "2", torch.cat(parts, 1))
        g = F.relu(F.linear(h.mean(2), p[q + "3.linear1.weight"], p[q + "3.linear1.bias"]))
        g = torch.sigmoid(F.linear(g, p[q + "3.linear2.weight"], p[q + "3.linear2.bias"]))
        cur = cur + h * g.unsqueeze(2)
        outs.append(cur)
    return F.relu(F.conv1d(torch.cat(outs, 1), p["conv.weight"], p["conv.bias"]))


def ecapa_forward(p, pool, x, training=True):
    """The whole ECAPA-TDNN with `pool` (emb_bn False): x [B, T, F] -> [B, embed_dim]."""
    stats = pool(ecapa_trunk(p, x, training=training))
    stats = F.batch_norm(stats, p["bn.running_mean"].clone(), p["bn.running_var"].clone(), p["bn.weight"], p["bn.bias"],
                         training, EO.BN_MOMENTUM, EO.BN_EPS)
    return F.linear(stats, p["linear.weight"], p["linear.bias"])


def campplus_trunk(p, x, blocks=CO.BLOCKS, training=True, relu_masks=None):
    """oracle.campplus_oracle.campplus_forward up to the pooling: x [B, T, F] -> y [B, 512, T'] (relu_masks as there)."""
    masks = list(relu_masks) if relu_masks is not None else None

    def relu(z):
        if masks is None:
            return F.relu(z)
        mk = masks.pop(0)
        assert mk.shape == z.shape, (mk.shape, z.shape)
        return z * mk.to(z.dtype)

    def bn(name, y):
        return F.batch_norm(y, p[name + ".running_mean"].clone(), p[name + ".running_var"].clone(), p[name + ".weight"],
                            p[name + ".bias"], training, CO.BN_MOMENTUM, CO.BN_EPS)

    y = x.permute(0, 2, 1).unsqueeze(1)
    y = relu(bn("head.bn1", F.conv2d(y, p["head.conv1.weight"], padding=1)))
    for li in (1, 2):
        for bi in (0, 1):
            q = f"head.layer{li}.{bi}."
            stride = (2, 1) if bi == 0 else (1, 1)
            o = relu(bn(q + "bn1", F.conv2d(y, p[q + "conv1.weight"], stride=stride, padding=1)))
            o = bn(q + "bn2", F.conv2d(o, p[q + "conv2.weight"], padding=1))
            sc = bn(q + "shortcut.1", F.conv2d(y, p[q + "shortcut.0.weight"], stride=stride)) if bi == 0 else y
            y = relu(o + sc)
    y = relu(bn("head.bn2", F.conv2d(y, p["head.conv2.weight"], stride=(2, 1), padding=1)))
    y = y.reshape(y.shape[0], y.shape[1] * y.shape[2], y.shape[3])
    y = relu(bn("xvector.tdnn.nonlinear.batchnorm", F.conv1d(y, p["xvector.tdnn.linear.weight"], stride=2, padding=2)))
    for bi, (layers, k, dil) in enumerate(blocks):
        for i in range(layers):
            q = f"xvector.block{bi + 1}.tdnnd{i + 1}."
            h = F.conv1d(relu(bn(q + "nonlinear1.batchnorm", y)), p[q + "linear1.weight"])
            h = relu(bn(q + "nonlinear2.batchnorm", h))
            local = F.conv1d(h, p[q + "cam_layer.linear_local.weight"], padding=(k - 1) // 2 * dil, dilation=dil)
            ctx = h.mean(-1, keepdim=True) + CO.seg_pooling(h)
            ctx = F.relu(F.conv1d(ctx, p[q + "cam_layer.linear1.weight"], p[q + "cam_layer.linear1.bias"]))
            mask = torch.sigmoid(F.conv1d(ctx, p[q + "cam_layer.linear2.weight"], p[q + "cam_layer.linear2.bias"]))
            y = torch.cat([y, local * mask], 1)
        q = f"xvector.transit{bi + 1}."
        y = F.conv1d(relu(bn(q + "nonlinear.batchnorm", y)), p[q + "linear.weight"])
    return relu(bn("xvector.out_nonlinear.batchnorm", y))


def campplus_forward(p, pool, x, blocks=CO.BLOCKS, training=True, relu_masks=None):
    """The whole CAM++ with `pool` in place of TSTP: x [B, T, F] -> [B, embed_dim]."""
    stats = pool(campplus_trunk(p, x, blocks, training, relu_masks))
    emb = F.conv1d(stats.unsqueeze(-1), p["xvector.dense.linear.weight"]).squeeze(-1)
    name = "xvector.dense.nonlinear.batchnorm"
    return F.batch_norm(emb, p[name + ".running_mean"].clone(), p[name + ".running_var"].clone(), None, None, training,
                        CO.BN_MOMENTUM, CO.BN_EPS)


def small_campplus(MC, blocks, pooling_func, feat_dim, embed_dim):
    """CAMPPlus with fewer dense layers per block (the constructor's (12, 24, 16) replaced) and the given pool."""
    import builtins
    real_zip = builtins.zip

    def fake_zip(*a):
        if a and a[0] == (12, 24, 16):
            return real_zip(*real_zip(*blocks))
        return real_zip(*a)
    MC.zip = fake_zip
    try:
        return MC.CAMPPlus(feat_dim=feat_dim, embed_dim=embed_dim, pooling_func=pooling_func)
    finally:
        del MC.zip
