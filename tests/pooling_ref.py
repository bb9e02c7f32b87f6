"""TEST INFRASTRUCTURE ONLY -- CPU restatements of wespeaker's MHASTP / MQMHASTP pooling layers (pooling_layers.py, as
recalled from the upstream source; parity UNPINNED like the rest of the encoder) and of a wespeaker
ResNet that ends in either of them, built from oracle.resnet_oracle's pieces.

    MHASTP(in_dim, layer_num=2, head_num=2, d_s=1, bottleneck_dim=64)
        d_model = in_dim / head_num; d_s = d_model if d_s > 1 else 1
        per head: att = Conv1d(d_model, 64, 1) - Tanh - Conv1d(64, d_s, 1)   (layer_num 1: Conv1d(d_model, d_s, 1))
        alpha = softmax_T(att(chunk)); mean = sum alpha x; var = sum alpha x^2 - mean^2
        out = cat over heads of (mean || sqrt(var.clamp(min=1e-7)))
    MQMHASTP(in_dim, layer_num=2, query_num=2, head_num=8, d_s=2, bottleneck_dim=64)
        cat over n_query.{q} = MHASTP(in_dim, layer_num, head_num, d_s, bottleneck_dim)"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import resnet_oracle as RO


class MHASTP(nn.Module):
    def __init__(self, in_dim, layer_num=2, head_num=2, d_s=1, bottleneck_dim=64, **kwargs):
        super().__init__()
        assert in_dim % head_num == 0
        self.in_dim, self.head_num = in_dim, head_num
        d_model = in_dim // head_num
        dims = [bottleneck_dim] * (layer_num + 1)
        d_s = d_model if d_s > 1 else 1
        self.d_s = d_s
        dims[0], dims[-1] = d_model, d_s
        heads = []
        for _ in range(head_num):
            att = nn.Sequential()
            for i in range(layer_num - 1):
                att.add_module("att_" + str(i), nn.Conv1d(dims[i], dims[i + 1], 1, 1))
                att.add_module("tanh" + str(i), nn.Tanh())
            att.add_module("att_" + str(layer_num - 1), nn.Conv1d(dims[layer_num - 1], dims[layer_num], 1, 1))
            heads.append(att)
        self.heads_att_trans = nn.ModuleList(heads)

    def get_out_dim(self):
        return 2 * self.in_dim

    def forward(self, x):
        """x [B, in_dim, T] (or [B, C, F, T], flattened to the [B, C*F, T] view) -> [B, 2 * in_dim]."""
        if x.dim() == 4:
            x = x.reshape(x.shape[0], x.shape[1] * x.shape[2], x.shape[3])
        outs = []
        for chunk, att in zip(torch.chunk(x, self.head_num, dim=1), self.heads_att_trans):
            alpha = torch.softmax(att(chunk), dim=2)
            mean = torch.sum(alpha * chunk, dim=2)
            var = torch.sum(alpha * chunk ** 2, dim=2) - mean ** 2
            outs.append(torch.cat([mean, torch.sqrt(var.clamp(min=1e-7))], dim=1))
        return torch.cat(outs, dim=1)


class MQMHASTP(nn.Module):
    def __init__(self, in_dim, layer_num=2, query_num=2, head_num=8, d_s=2, bottleneck_dim=64, **kwargs):
        super().__init__()
        self.in_dim, self.query_num = in_dim, query_num
        self.n_query = nn.ModuleList([MHASTP(in_dim, layer_num=layer_num, head_num=head_num, d_s=d_s,
                                             bottleneck_dim=bottleneck_dim) for _ in range(query_num)])

    def get_out_dim(self):
        return self.query_num * 2 * self.in_dim

    def forward(self, x):
        return torch.cat([q(x) for q in self.n_query], dim=-1)


POOLS = {"MHASTP": MHASTP, "MQMHASTP": MQMHASTP}


class ResNetPooled(nn.Module):
    """Parameter container of a wespeaker ResNet whose pooling is MHASTP / MQMHASTP: the trunk's names and shapes come
    from oracle.resnet_oracle.param_shapes (as buffers-or-parameters), the pool is the restatement above, seg_1 a Linear
    of get_out_dim() inputs.  state_dict() is the encoder's."""

    def __init__(self, name="ResNet34", feat_dim=80, embed_dim=256, pooling_func="MQMHASTP", m=32, seed=0):
        super().__init__()
        self.num_blocks, self.bottleneck = RO.NUM_BLOCKS[name], name in RO.BOTTLENECK
        ex = 4 if self.bottleneck else 1
        shapes = RO.param_shapes(num_blocks=self.num_blocks, m=m, feat_dim=feat_dim, embed_dim=embed_dim,
                                 bottleneck=self.bottleneck)
        trunk = RO.synth_params(seed, num_blocks=self.num_blocks, m=m, feat_dim=feat_dim, embed_dim=embed_dim,
                                bottleneck=self.bottleneck)
        self.m = m
        self.trunk_names = [k for k in shapes if not k.startswith("seg_1.")]
        for k in self.trunk_names:
            v = trunk[k]
            if RO.is_buffer(k):
                self.register_buffer(_flat(k), v.clone())
            else:
                self.register_parameter(_flat(k), nn.Parameter(v.clone()))
        in_dim = (feat_dim // 8) * m * 8 * ex
        self.pool = POOLS[pooling_func](in_dim=in_dim)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for k, p in self.pool.named_parameters():
                if k.endswith("bias"):
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p.shape[1]) ** 0.5)
        self.seg_1 = nn.Linear(self.pool.get_out_dim(), embed_dim)

    def state_dict_encoder(self):
        """The encoder's state_dict keys (the trunk's dotted names, then pool.* and seg_1.*)."""
        sd = {k: getattr(self, _flat(k)).detach() for k in self.trunk_names}
        for k, v in self.pool.state_dict().items():
            sd["pool." + k] = v
        for k, v in self.seg_1.state_dict().items():
            sd["seg_1." + k] = v
        return sd

    def trunk_params(self):
        return {k: getattr(self, _flat(k)) for k in self.trunk_names}

    def forward(self, x, relu_masks=None, training=True):
        """x [B, T, F] fbank -> embed_a [B, embed_dim] (two_emb_layer False)."""
        y = trunk_forward(self.trunk_params(), x, self.num_blocks, self.m, self.bottleneck, relu_masks, training)
        return self.seg_1(self.pool(y))


def _flat(k):
    return k.replace(".", "__")


def trunk_forward(p, x, num_blocks, m=32, bottleneck=False, relu_masks=None, training=True):
    """The ResNet trunk of oracle.resnet_oracle.resnet_forward up to the pooling: x [B, T, F] -> [B, C, F', T']."""
    masks = list(relu_masks) if relu_masks is not None else None

    def relu(z):
        if masks is None:
            return F.relu(z)
        mk = masks.pop(0)
        assert mk.shape == z.shape, (mk.shape, z.shape)
        return z * mk.to(z.dtype)

    def bn(name, y):
        return F.batch_norm(y, p[name + ".running_mean"].clone(), p[name + ".running_var"].clone(), p[name + ".weight"],
                            p[name + ".bias"], training, RO.BN_MOMENTUM, RO.BN_EPS)
    y = x.permute(0, 2, 1).unsqueeze(1)
    y = relu(bn("bn1", F.conv2d(y, p["conv1.weight"], padding=1)))
    for q, inp, planes, stride in RO._blocks(num_blocks, m, 4 if bottleneck else 1):
        if bottleneck:
            o = relu(bn(q + "bn1", F.conv2d(y, p[q + "conv1.weight"])))
            o = relu(bn(q + "bn2", F.conv2d(o, p[q + "conv2.weight"], stride=stride, padding=1)))
            o = bn(q + "bn3", F.conv2d(o, p[q + "conv3.weight"]))
        else:
            o = relu(bn(q + "bn1", F.conv2d(y, p[q + "conv1.weight"], stride=stride, padding=1)))
            o = bn(q + "bn2", F.conv2d(o, p[q + "conv2.weight"], padding=1))
        sc = y
        if (q + "shortcut.0.weight") in p:
            sc = bn(q + "shortcut.1", F.conv2d(y, p[q + "shortcut.0.weight"], stride=stride))
        y = relu(o + sc)
    return y
