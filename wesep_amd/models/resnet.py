"""wespeaker ResNet speaker encoder on MI355X: module tree and `state_dict` keys of
`wespeaker.models.resnet.ResNet` (BasicBlock variants: ResNet18 / ResNet34), so `spk_model_init` checkpoints load.
The package itself is a third-party dependency absent from the reference tree: parity is against the restatement in
oracle/resnet_oracle.py and is UNPINNED.  nn.Conv2d / nn.BatchNorm2d / nn.Linear objects are parameter
containers only; forward is a chain of C-ABI launches (wesep_amd/functional_resnet.py).  Pooling: TSTP / TAP / TSDP,
ASTP, and wespeaker's MHASTP / MQMHASTP (restated in tests/pooling_ref.py; one launch each way, csrc/mhastp.hip)."""
import torch
import torch.nn as nn

from .. import functional_resnet as FR
from ..functional import LinearFn, PackCache


class TSTP(nn.Module):
    """Temporal statistics pooling (no parameters): mean || std."""

    def __init__(self, in_dim=0, **kwargs):
        super().__init__()
        self.in_dim = in_dim

    def get_out_dim(self):
        return self.in_dim * 2


class TAP(TSTP):
    """Temporal average pooling: the mean half of TSTP."""

    def get_out_dim(self):
        return self.in_dim


class TSDP(TSTP):
    """Temporal standard-deviation pooling: the std half of TSTP."""

    def get_out_dim(self):
        return self.in_dim


MHASTP_LDS_FLOATS = 16384 - 64        # csrc/mhastp.hip: one frame of the head (x, dx, attention rows) per 64 KiB of LDS


class MHASTP(nn.Module):
    """wespeaker `pooling_layers.MHASTP` (multi-head attentive statistics pooling): the [R, C*F', T'] view splits into
    head_num heads of d_model = in_dim / head_num features; per head alpha = softmax_T(att(chunk)) with att = Conv1d(d_model,
    64, 1) - Tanh - Conv1d(64, d_s, 1) (layer_num 2) or Conv1d(d_model, d_s, 1) (layer_num 1), d_s = d_model if d_s > 1
    else 1; out = cat over heads of (mean || sqrt(clamp(var, 1e-7))).  Module tree and names as upstream
    (heads_att_trans.{h}.att_{i}); forward is one HIP launch (functional_resnet.MhastpFn)."""

    def __init__(self, in_dim, layer_num=2, head_num=2, d_s=1, bottleneck_dim=64, **kwargs):
        super().__init__()
        assert in_dim % head_num == 0, (in_dim, head_num)
        if layer_num not in (1, 2):
            raise NotImplementedError(f"MHASTP layer_num {layer_num}: the HIP kernels are built for 1 and 2")
        if layer_num == 2 and bottleneck_dim != 64:
            raise NotImplementedError(f"MHASTP bottleneck_dim {bottleneck_dim}: the HIP kernels are built for 64")
        self.in_dim, self.head_num, self.layer_num = in_dim, head_num, layer_num
        d_model = in_dim // head_num
        self.d_model = d_model
        self.d_s = d_model if d_s > 1 else 1
        dims = [bottleneck_dim] * (layer_num + 1)
        dims[0], dims[-1] = d_model, self.d_s
        heads = []
        for _ in range(head_num):
            att = nn.Sequential()
            for i in range(layer_num - 1):
                att.add_module(f"att_{i}", nn.Conv1d(dims[i], dims[i + 1], 1, 1))
                att.add_module(f"tanh{i}", nn.Tanh())
            att.add_module(f"att_{layer_num - 1}", nn.Conv1d(dims[layer_num - 1], dims[layer_num], 1, 1))
            heads.append(att)
        self.heads_att_trans = nn.ModuleList(heads)
        self.cache = PackCache()

    def get_out_dim(self):
        return 2 * self.in_dim

    def att_params(self):
        out = []
        for att in self.heads_att_trans:
            for i in range(self.layer_num):
                conv = getattr(att, f"att_{i}")
                out += [conv.weight, conv.bias]
        return out

    def check_channels(self, C):
        """The kernels' geometry: a head is a channel range of the [R, F', T', C] activation (C*F' = in_dim)."""
        if C % self.head_num:
            raise NotImplementedError(f"MHASTP head_num {self.head_num} does not divide the {C} channels: a head must be "
                                      "a channel range of the encoder's activation")
        n1 = 64 if self.layer_num == 2 else self.d_s
        if 2 * self.d_model + n1 + (self.d_s if self.layer_num == 2 else 0) > MHASTP_LDS_FLOATS:
            raise NotImplementedError(f"MHASTP d_model {self.d_model}: one frame of a head exceeds the kernels' LDS "
                                      "tile; use more heads")

    def run(self, y, R, Fq, T, split=False):
        """y [R*F'*T', C] (the last block's channels-last output) -> [R, 2 * in_dim].  split: the grid split over T
        (the 1-D encoders, F' = 1, which pool at the full frame rate)."""
        return _mhastp_run([self], self.cache, y, R, Fq, T, split)


class MQMHASTP(nn.Module):
    """wespeaker `pooling_layers.MQMHASTP`: query_num independent MHASTP layers (n_query.{q}) on the same input,
    concatenated; one HIP launch serves all queries (each (row, head) chunk is staged once)."""

    def __init__(self, in_dim, layer_num=2, query_num=2, head_num=8, d_s=2, bottleneck_dim=64, **kwargs):
        super().__init__()
        self.in_dim, self.query_num = in_dim, query_num
        self.n_query = nn.ModuleList([MHASTP(in_dim, layer_num=layer_num, head_num=head_num, d_s=d_s,
                                             bottleneck_dim=bottleneck_dim) for _ in range(query_num)])
        self.cache = PackCache()

    def get_out_dim(self):
        return self.query_num * 2 * self.in_dim

    def check_channels(self, C):
        self.n_query[0].check_channels(C)

    def run(self, y, R, Fq, T, split=False):
        return _mhastp_run(list(self.n_query), self.cache, y, R, Fq, T, split)


def _mhastp_run(queries, cache, y, R, Fq, T, split=False):
    q0 = queries[0]
    params = [p for q in queries for p in q.att_params()]
    geo = (R, Fq, T, len(queries), q0.head_num, q0.layer_num, q0.d_s) + ((True,) if split else ())
    return FR.MhastpFn.apply(y, geo, cache, *params)


POOLING_FUNCS = ("TSTP", "TAP", "TSDP", "ASTP", "MHASTP", "MQMHASTP")
RAGGED_POOLING_FUNCS = ("TSTP", "TAP", "TSDP", "ASTP")      # the pools with a length-aware kernel (csrc/ragged_spk.hip)


def ragged_guard(module, who, pooling_func, lengths):
    """`lengths=` of a speaker encoder's forward: inference only (batch statistics over ragged rows are out of scope),
    and only with a pool that has a length-aware kernel."""
    if lengths is None:
        return
    from .._lib import WesepHipError
    if module.training or torch.is_grad_enabled():
        raise WesepHipError(f"{who}: lengths= is built for inference (eval mode under torch.no_grad()); ragged training "
                            "and BatchNorm statistics over ragged rows are out of scope")
    if pooling_func not in RAGGED_POOLING_FUNCS:
        raise NotImplementedError(f"{who}: lengths= with pooling_func {pooling_func}: {', '.join(RAGGED_POOLING_FUNCS)} "
                                  "have a length-aware kernel")


def _pooling_layer(name, in_dim, **kwargs):
    """wespeaker.models.pooling_layers by name: TSTP / TAP / TSDP (one statistics kernel), ASTP (attentive statistics,
    the ECAPA-TDNN module of models/ecapa_tdnn.py on the [R, C * F', T] view), MHASTP and MQMHASTP (csrc/mhastp.hip) --
    each with the constructor defaults wespeaker builds it with (`in_dim` only); kwargs (ECAPA-TDNN's
    global_context_att) go to every class, and only ASTP uses them."""
    if name in ("TSTP", "TAP", "TSDP"):
        return {"TSTP": TSTP, "TAP": TAP, "TSDP": TSDP}[name](in_dim=in_dim, **kwargs)
    if name == "ASTP":
        from .ecapa_tdnn import ASTP
        return ASTP(in_dim=in_dim, **kwargs)
    if name in ("MHASTP", "MQMHASTP"):
        return {"MHASTP": MHASTP, "MQMHASTP": MQMHASTP}[name](in_dim=in_dim, **kwargs)
    raise NotImplementedError(f"pooling_func {name!r}: TSTP, TAP, TSDP, ASTP, MHASTP and MQMHASTP are built")


def run_pool(pool, name, y, R, T, tl=None):
    """A pooling layer of _pooling_layer on the channels-last frames y [R*T, C] of a 1-D encoder (F' = 1) ->
    [R, pool.get_out_dim()]; MHASTP / MQMHASTP on the grid split over T.  tl: the int32 device table of the rows' valid
    frames (ragged batches; RAGGED_POOLING_FUNCS)."""
    if name == "ASTP":
        return pool.run(y, R, T, tl)
    if name in ("MHASTP", "MQMHASTP"):
        if tl is not None:
            raise NotImplementedError(f"lengths= with pooling_func {name}")
        return pool.run(y, R, 1, T, split=True)
    stats = FR.TstpFn.apply(y, (R, 1, T, tl))                               # mean || sqrt(var + 1e-7), each [C]
    half = stats.shape[1] // 2
    if name == "TAP":
        return stats[:, :half].contiguous()
    if name == "TSDP":
        return stats[:, half:].contiguous()
    return stats


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.shortcut = nn.Sequential()
        if stride != 1 or in_planes != self.expansion * planes:
            self.shortcut = nn.Sequential(
                nn.Conv2d(in_planes, self.expansion * planes, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(self.expansion * planes))
        self.stride = stride


class Bottleneck(nn.Module):
    """wespeaker Bottleneck (ResNet50 / 101 / 152): 1x1 - 3x3(stride) - 1x1, expansion 4."""
    expansion = 4

    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, self.expansion * planes, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(self.expansion * planes)
        self.shortcut = nn.Sequential()
        if stride != 1 or in_planes != self.expansion * planes:
            self.shortcut = nn.Sequential(
                nn.Conv2d(in_planes, self.expansion * planes, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(self.expansion * planes))
        self.stride = stride


def _cba(x, res, R, H, W, stride, relu, conv, bn, training):
    if training:
        bn.num_batches_tracked += 1
    return FR.ConvBnActFn.apply(x, res, (R, H, W, stride, relu, training), conv.weight, bn.weight, bn.bias,
                                bn.running_mean, bn.running_var)


def _cba_len(x, res, R, H, W, stride, relu, conv, bn, wlen):
    """_cba of a ragged inference pass: the masked epilogue writes zeros behind the rows' valid output widths `wlen`."""
    return FR.ConvBnActFn.apply(x, res, (R, H, W, stride, relu, False, wlen), conv.weight, bn.weight, bn.bias,
                                bn.running_mean, bn.running_var)


class ResNet(nn.Module):
    def __init__(self, block, num_blocks, m_channels=32, feat_dim=40, embed_dim=128, pooling_func="TSTP",
                 two_emb_layer=True):
        super().__init__()
        self.pooling_func = pooling_func
        self.in_planes, self.feat_dim, self.embed_dim = m_channels, feat_dim, embed_dim
        self.stats_dim = int(feat_dim / 8) * m_channels * 8
        self.two_emb_layer = two_emb_layer
        self.conv1 = nn.Conv2d(1, m_channels, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(m_channels)
        self.layer1 = self._make_layer(block, m_channels, num_blocks[0], stride=1)
        self.layer2 = self._make_layer(block, m_channels * 2, num_blocks[1], stride=2)
        self.layer3 = self._make_layer(block, m_channels * 4, num_blocks[2], stride=2)
        self.layer4 = self._make_layer(block, m_channels * 8, num_blocks[3], stride=2)
        self.pool = _pooling_layer(pooling_func, self.stats_dim * block.expansion)
        if pooling_func in ("MHASTP", "MQMHASTP"):
            self.pool.check_channels(m_channels * 8 * block.expansion)
        self.pool_out_dim = self.pool.get_out_dim()
        self.seg_1 = nn.Linear(self.pool_out_dim, embed_dim)
        if two_emb_layer:
            self.seg_bn_1 = nn.BatchNorm1d(embed_dim, affine=False)
            self.seg_2 = nn.Linear(embed_dim, embed_dim)
        else:
            self.seg_bn_1 = nn.Identity()
            self.seg_2 = nn.Identity()

    def _make_layer(self, block, planes, num_blocks, stride):
        layers = []
        for s in [stride] + [1] * (num_blocks - 1):
            layers.append(block(self.in_planes, planes, s))
            self.in_planes = planes * block.expansion
        return nn.Sequential(*layers)

    def forward(self, x, lengths=None):
        """x [R, T, F] fbank -> (tensor(0.), embed_a [R, embed_dim]), or (embed_a, embed_b) with two_emb_layer.
        lengths (eval mode under torch.no_grad() only): the valid frames of every row.  One pass over the rectangle then
        gives each row the embedding it gets alone: every layer's input is exactly zero behind the row's own width, which
        follows the convolutions' geometry (ragged_widths); whatever x holds behind a row's frames is ignored."""
        ragged_guard(self, "ResNet speaker encoder", self.pooling_func, lengths)
        if not x.is_cuda:
            from .._lib import WesepHipError
            raise WesepHipError("ResNet speaker encoder: wesep_amd has no CPU path")
        R, T, Fq = x.shape
        tr = self.training
        tabs = None
        if lengths is not None:
            from .. import dev
            tl = dev.length_table(lengths, R, T, x.device, lo=1)
            xs = torch.empty(R, T, Fq, device=x.device, dtype=torch.float32)
            if Fq % 4:
                raise NotImplementedError("ResNet speaker encoder: lengths= needs feat_dim % 4 == 0")
            dev.tail_select_len(x.float().contiguous(), R, T, Fq, tl, xs)
            x = xs
            tabs = _WidthTables(lengths, x.device)
        wl = (lambda k, s, p: tabs.step(k, s, p)) if tabs is not None else (lambda k, s, p: None)

        def cba(x, res, R, H, W, stride, relu, conv, bn, wlen):
            if wlen is None:
                return _cba(x, res, R, H, W, stride, relu, conv, bn, tr)
            return _cba_len(x, res, R, H, W, stride, relu, conv, bn, wlen)
        y = x.float().transpose(1, 2).contiguous().view(R * Fq * T, 1)      # [R, F, T, 1]
        H, W = Fq, T
        y = cba(y, None, R, H, W, 1, True, self.conv1, self.bn1, wl(3, 1, 1))
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                s = blk.stride
                Ho, Wo = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
                # the rows' widths behind this block: the 3x3 stride-s convolution's, which the 1x1 stride-s shortcut
                # shares; every other convolution of the block keeps the width it is given
                w_in, w_out = wl(1, 1, 0), wl(3, s, 1)
                sc = y
                if len(blk.shortcut) > 0:
                    sc = cba(y, None, R, H, W, s, False, blk.shortcut[0], blk.shortcut[1], w_out)
                if isinstance(blk, Bottleneck):
                    o = cba(y, None, R, H, W, 1, True, blk.conv1, blk.bn1, w_in)
                    o = cba(o, None, R, H, W, s, True, blk.conv2, blk.bn2, w_out)
                    y = cba(o, sc, R, Ho, Wo, 1, True, blk.conv3, blk.bn3, w_out)
                else:
                    o = cba(y, None, R, H, W, s, True, blk.conv1, blk.bn1, w_out)
                    y = cba(o, sc, R, Ho, Wo, 1, True, blk.conv2, blk.bn2, w_out)
                H, W = Ho, Wo
        tl = wl(1, 1, 0)                                                     # the rows' frames at the pooling layer
        if self.pooling_func == "ASTP":      # [R, F', T, C] -> frames [R*T, C * F'] (feature index c * F' + f), then ASTP
            Cc = y.shape[1]
            frames = y.view(R, H, W, Cc).permute(0, 2, 3, 1).reshape(R * W, Cc * H)
            stats = self.pool.run(frames, R, W, tl)
        elif self.pooling_func in ("MHASTP", "MQMHASTP"):      # straight from the [R, F', T', C] layout
            stats = self.pool.run(y, R, H, W)
        else:
            stats = FR.TstpFn.apply(y, (R, H, W, tl))                           # mean || std, each [C * F']
            half = stats.shape[1] // 2
            if self.pooling_func == "TAP":
                stats = stats[:, :half].contiguous()
            elif self.pooling_func == "TSDP":
                stats = stats[:, half:].contiguous()
        embed_a = LinearFn.apply(stats, self.seg_1.weight, self.seg_1.bias)
        if not self.two_emb_layer:
            return torch.tensor(0.0), embed_a
        from .. import functional_ecapa as FE
        E = self.embed_dim
        if tr:
            self.seg_bn_1.num_batches_tracked += 1
        ones, zeros = torch.ones(E, device=x.device), torch.zeros(E, device=x.device)
        o = FE.BatchNormRowsFn.apply(torch.relu(embed_a), ones, zeros, self.seg_bn_1.running_mean,
                                     self.seg_bn_1.running_var, tr)          # affine=False; [R, E]: a few thousand numbers
        return embed_a, LinearFn.apply(o, self.seg_2.weight, self.seg_2.bias)


def ragged_widths(lengths, num_blocks, bottleneck=False):
    """The per-layer width tables of a ragged ResNet pass, on the host: for every conv + BN + activation of the forward, in
    launch order (stem; per block: [shortcut,] conv1, conv2 [, conv3]), the rows' valid OUTPUT widths
    W' = (W + 2p - k) // s + 1 with that layer's own k, p, s.  The last entry is what the pooling layer reduces over."""
    from ..dev import conv_widths
    w = conv_widths(lengths, 3, 1, 1)
    out = [w]
    for li, n in enumerate(num_blocks):
        for bi in range(n):
            s = 2 if (li > 0 and bi == 0) else 1
            has_sc = s != 1 or (li == 0 and bi == 0 and bottleneck)
            if has_sc:
                out.append(conv_widths(w, 1, s, 0))
            if bottleneck:
                w1 = conv_widths(w, 1, 1, 0)
                w2 = conv_widths(w1, 3, s, 1)
                w = conv_widths(w2, 1, 1, 0)
                out += [w1, w2, w]
            else:
                w1 = conv_widths(w, 3, s, 1)
                w = conv_widths(w1, 3, 1, 1)
                out += [w1, w]
    return out


class _WidthTables:
    """The rows' current widths on the host and one small int32 device table per distinct width set."""

    def __init__(self, lengths, device):
        self.w = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
        self.device, self.tabs = device, {}

    def step(self, k, s, p):
        """The table of the widths behind a convolution (k, stride s, padding p) of the current ones; s > 1 advances."""
        from ..dev import conv_widths
        w = conv_widths(self.w, k, s, p)
        if s > 1:
            self.w = w
        key = tuple(w)
        if key not in self.tabs:
            self.tabs[key] = torch.tensor(w, dtype=torch.int32).to(self.device)
        return self.tabs[key]


def ResNet18(feat_dim, embed_dim, pooling_func="TSTP", two_emb_layer=True):
    return ResNet(BasicBlock, [2, 2, 2, 2], feat_dim=feat_dim, embed_dim=embed_dim, pooling_func=pooling_func,
                  two_emb_layer=two_emb_layer)


def ResNet34(feat_dim, embed_dim, pooling_func="TSTP", two_emb_layer=True):
    return ResNet(BasicBlock, [3, 4, 6, 3], feat_dim=feat_dim, embed_dim=embed_dim, pooling_func=pooling_func,
                  two_emb_layer=two_emb_layer)


def _bottleneck_resnet(num_blocks):
    def make(feat_dim, embed_dim, pooling_func="TSTP", two_emb_layer=True):
        return ResNet(Bottleneck, num_blocks, feat_dim=feat_dim, embed_dim=embed_dim, pooling_func=pooling_func,
                      two_emb_layer=two_emb_layer)
    return make


ResNet50, ResNet101, ResNet152 = (_bottleneck_resnet(n) for n in ([3, 4, 6, 3], [3, 4, 23, 3], [3, 8, 36, 3]))


def get_speaker_model(model_name: str):
    """`wespeaker.models.speaker_model.get_speaker_model` for the encoders built here."""
    table = {"ResNet18": ResNet18, "ResNet34": ResNet34, "ResNet50": ResNet50, "ResNet101": ResNet101,
             "ResNet152": ResNet152}
    if model_name in table:
        return table[model_name]
    from .ecapa_tdnn import ECAPA_MODELS
    if model_name in ECAPA_MODELS:
        return ECAPA_MODELS[model_name]
    if model_name == "CAMPPlus":
        from .campplus import CAMPPlus
        return CAMPPlus
    raise NotImplementedError(f"speaker model {model_name!r}: the wespeaker ResNets (18 / 34 / 50 / 101 / 152), "
                              "ECAPA-TDNN (c512 / c1024, with or without global context) and CAM++ (CAMPPlus) are built "
                              "(SURVEY.md section 8 row a12)")
