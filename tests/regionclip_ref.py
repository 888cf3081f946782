"""Float64 restatement of RegionCLIP's ModifiedResNet tower (P/src/regionclip/clip_backbone.py:14-300), written from the
reference's description, on the ENGINE's weights (weights.regionclip_to_engine: FrozenBN as scale / shift, q | k | v concatenated).

    tokens64(eng_sd, imgs, layers, heads, spatial_attn=True) -> [B, 1 + HW, out] float64, L2-normalised rows

``rnd`` (optional: torch.float16 / torch.bfloat16) rounds where the fp16 tower rounds -- every conv output, BN output, residual sum,
pool and the attnpool's input rows -- so that the same function states the GPU's fp16 / bf16 arithmetic up to the order of its sums.
The helpers (conv_ref, avgpool_ref, attnpool_in_ref) are the single-kernel references of tests/test_gpu_regionclip.py."""
import torch
import torch.nn.functional as F


def _r(x, rnd):
    return x if rnd is None else x.to(rnd).to(torch.float64)


def conv_ref(x, w, scale, shift, stride, res=None, relu=True, rnd=None):
    """x [B][C][H][W], w [Cout][Cin][k][k] -> relu(rnd(rnd(rnd(conv) * scale + shift) (+ res))): the BN's affine map rounded once,
    as the reference's eval F.batch_norm and resnet.hip round it"""
    k = w.shape[-1]
    y = F.conv2d(x.double(), w.double(), stride=stride, padding=k // 2)
    y = _r(y, rnd)
    y = _r(y * scale.double()[None, :, None, None] + shift.double()[None, :, None, None], rnd)
    if res is not None:
        y = _r(y + res, rnd)
    return y.clamp_min(0) if relu else y


def avgpool_ref(x, rnd=None):
    return _r(F.avg_pool2d(x.double(), 2), rnd)


def attnpool_in_ref(x, pos, rnd=None):
    """x [B][C][h][w] -> rows [B][1 + hw][C]: mean row, then the pixels, + pos (each rounded as the fp16 tower rounds)"""
    B, C = x.shape[:2]
    t = x.reshape(B, C, -1).permute(0, 2, 1)
    t = torch.cat([_r(t.mean(1, keepdim=True), rnd), t], 1)
    return _r(t + _r(pos.double(), rnd)[None], rnd)


def _mha(x, qkv_w, qkv_b, heads, rnd):
    B, T, C = x.shape
    qkv = _r(x @ qkv_w.double().t() + qkv_b.double(), rnd)
    q, k, v = qkv.split(C, -1)
    sh = lambda t: t.reshape(B, T, heads, C // heads).transpose(1, 2)
    a = torch.softmax((sh(q) @ sh(k).transpose(-1, -2)) / (C // heads) ** 0.5, -1)
    return _r((a @ sh(v)).transpose(1, 2).reshape(B, T, C), rnd)


def tokens64(sd, imgs, layers, heads, spatial_attn=True, rnd=None):
    g = lambda k: sd["rn." + k]

    def cbn(x, conv, bn, stride=1, res=None, relu=True):
        return conv_ref(x, g(conv + ".weight"), g(bn + ".scale"), g(bn + ".shift"), stride, res, relu, rnd)

    x = _r(imgs.double(), rnd)
    x = cbn(x, "conv1", "bn1", 2)
    x = cbn(x, "conv2", "bn2")
    x = cbn(x, "conv3", "bn3")
    x = avgpool_ref(x, rnd)
    for L in range(4):
        for i in range(layers[L]):
            p = "layer%d.%d." % (L + 1, i)
            stride = 2 if (L > 0 and i == 0) else 1
            o = cbn(x, p + "conv1", p + "bn1")
            o = cbn(o, p + "conv2", p + "bn2")
            if stride > 1:
                o = avgpool_ref(o, rnd)
            idn = x
            if i == 0:
                idn = cbn(avgpool_ref(x, rnd) if stride > 1 else x, p + "downsample.0", p + "downsample.1", relu=False)
            x = cbn(o, p + "conv3", p + "bn3", res=idn)
    B, C = x.shape[:2]
    rows = attnpool_in_ref(x, g("attnpool.positional_embedding"), rnd)
    att = _mha(rows, g("attnpool.qkv.weight"), g("attnpool.qkv.bias"), heads, rnd)
    cw, cb = g("attnpool.c_proj.weight").double(), g("attnpool.c_proj.bias").double()
    out = _r(att @ cw.t() + cb, rnd)
    if not spatial_attn:
        pix = x.reshape(B, C, -1).permute(0, 2, 1)
        out = torch.cat([out[:, :1], _r(pix @ cw.t() + cb, rnd)], 1)
    return F.normalize(out, dim=-1)
