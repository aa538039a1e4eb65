"""Host logic of DepthNet_Fusion's eval-mode plan (plugin/depth_net.py) without a GPU: the folded, padded,
permuted layers of ``depth_net_plan`` are applied with plain F.conv2d / F.conv_transpose2d in the order and with the
epilogues ``_forward_hip`` uses, and must reproduce the module's own eval output on the golden inputs."""
import numpy as np
import os
import torch
import torch.nn.functional as F

from golden_util import load, img_meta, max_err, fill_by_name


def _apply(x, L, residual=None, relu=True, relu_after_add=False):
    """One planned layer on an NCHW tensor whose channel count is the layer's PADDED input width."""
    k = L.k
    taps, coutp, cinp = L.w.shape
    assert x.shape[1] == cinp
    w = L.w.reshape(k, k, coutp, cinp)
    if L.transposed:
        y = F.conv_transpose2d(x, w.permute(3, 2, 0, 1), stride=2, padding=1, output_padding=1)
    else:
        y = F.conv2d(x, w.permute(2, 3, 0, 1), stride=L.stride, padding=k // 2)
    y = y * L.scale.view(1, -1, 1, 1) + L.shift.view(1, -1, 1, 1)
    if relu:
        y = F.relu(y)
    if residual is not None:
        y = y + residual
    if relu_after_add:
        y = F.relu(y)
    return y


def _unet(x, U):
    c2 = _apply(_apply(x, U["conv1"]), U["conv2"])
    c4 = _apply(_apply(c2, U["conv3"]), U["conv4"])
    return _apply(_apply(c4, U["conv9"], residual=c2), U["conv11"], residual=x)


def _build():
    import sgcdet_amd.plugin as P
    d, _ = load("depth_net")
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_net.npz"))
    stride, dbound = int(z["stride"]), [float(v) for v in z["dbound"]]
    net = P.DepthNet_Fusion(neighbor_img_num=2, downsample_factor=stride, dbound=dbound, mono_channels=d["xs"].shape[2],
                            loss_weight=0.5, max_tol=0, init_weight="none").eval()
    fill_by_name(net, base_seed=7, scale=0.15)
    return net, d, stride


def test_plan_applied_with_torch_convolutions_reproduces_the_eval_forward():
    from sgcdet_amd.plugin.depth_net import depth_net_plan
    net, d, stride = _build()
    meta = img_meta(d)
    with torch.no_grad():
        want = net(d["xs"], d["imgs"], [meta], stride)
        assert max_err(want, d["pred"]) < 5e-5                      # the torch formulation is the reference's
        P = depth_net_plan(net)
        D = net.depth_channels
        img, xs = d["imgs"][0], d["xs"][0]
        # stem: [64, 160] rows (ci*7 + kh)*7 + kw
        st = P["stem"]
        assert st.w.shape == (64, 160) and st.w[:, 147:].abs().max() == 0
        x = F.conv2d(img, st.w[:, :147].reshape(64, 3, 7, 7), stride=2, padding=3)
        x = F.relu(x * st.scale.view(1, -1, 1, 1) + st.shift.view(1, -1, 1, 1))
        for B in P["blocks"]:
            y = _apply(x, B["conv1"])
            if "down" in B:
                y = _apply(y, B["conv2"])
                x = _apply(x, B["down"], residual=y, relu=False, relu_after_add=True)
            else:
                x = _apply(y, B["conv2"], residual=x)
        f_mvs = _apply(x, P["final"], relu=False)
        assert max_err(f_mvs, net.fnet_mvs(img)) < 1e-5 * max(1.0, f_mvs.abs().max().item())
        corr = net.correlation(f_mvs, meta, stride)
        cost = _unet(F.pad(corr, (0, 0, 0, 0, 0, 32 - D)), P["corr"])
        assert cost[:, D:].abs().max() == 0                          # padded columns stay exactly 0
        mono = _unet(_apply(xs, P["fnet_mono"]), P["mono"])
        cat = torch.cat([mono, cost], 1)                              # the buffer's column order: mono | cost | zeros
        assert cat.shape[1] == P["fusion"]["conv1"].w.shape[2]
        fused = _unet(cat, P["fusion"])
        assert fused[:, 128 + D:].abs().max() == 0
        got = F.softmax(_apply(fused, P["depth_reg"], relu=False), dim=1)
    assert got.shape == want[0].shape
    assert max_err(got, want[0]) < 1e-5


def test_plan_pads_both_channel_dimensions_and_folds_the_shared_batchnorm_once():
    from sgcdet_amd.plugin.conv_plan import Conv2dSpec
    from sgcdet_amd.plugin.depth_net import depth_net_plan
    net, d, _ = _build()
    P = depth_net_plan(net)
    D = net.depth_channels

    def layers(p):
        if isinstance(p, Conv2dSpec):
            yield p
        elif isinstance(p, dict):
            for v in p.values():
                yield from layers(v)
        elif isinstance(p, list):
            for v in p:
                yield from layers(v)
    n = 0
    for L in layers({k: v for k, v in P.items() if k not in ("stem", "depth_reg")}):
        taps, coutp, cinp = L.w.shape
        assert coutp % 32 == 0 and cinp % 32 == 0 and coutp >= L.cout and cinp >= L.cin
        assert L.w[:, L.cout:].abs().sum() == 0 and L.w[:, :, L.cin:].abs().sum() == 0
        assert (L.shift[L.cout:] == 0).all() and (L.scale[L.cout:] == 1).all()
        n += 1
    assert n == 8 + 1 + 1 + 1 + 18                                   # BasicBlock convs, projection, final 1x1, fnet_mono, 3 U-Nets
    assert P["fusion"]["conv1"].w.shape[2] == 160 and P["fusion"]["conv3"].w.shape[1:] == (576, 288)
    assert P["depth_reg"].w.shape == (9, D, 160)
    blk = net.fnet_mvs.layer2[0]
    assert blk.downsample[1] is blk.bn3                              # one BatchNorm under two keys ...
    down = P["blocks"][2]["down"]
    want = blk.bn3.weight / torch.sqrt(blk.bn3.running_var + blk.bn3.eps)
    assert torch.allclose(down.scale, want.detach())                 # ... folded once: scale is gamma / sigma, not its square
    # the permuted concatenation: new column j < 128 is module channel D + j (mono_reg), 128 + i is channel i (cost_reg)
    w_mod = net.depth_reg.weight.detach()
    assert torch.equal(P["depth_reg"].w[4, :, :128], w_mod[:, D:, 1, 1]) and torch.equal(P["depth_reg"].w[4, :, 128:128 + D], w_mod[:, :D, 1, 1])
