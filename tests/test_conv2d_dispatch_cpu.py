"""``conv_plan.conv2d_rows``: the one rule that sends a 2-D layer to ``sgc_conv2d_nhwc_bf16x3`` / ``_ex`` / ``_strided``
(DESIGN.md 4.11, 4.12), driven with a recording stand-in for ``ops`` on CPU tensors -- no kernel runs.  The table below is written
by hand; the second test shows that ``Conv2dSpec.__call__`` and ``FrozenNormConv2dFunction`` (forward and input gradients)
reach the entries only through that rule, so a layer takes the same entry in eval and in training."""
import pytest
import torch

C = 32


class RecordingOps:
    """Stands in for ``ext.ops()``: records (entry, arguments that select the kernel form) and returns zeros of the output shape."""

    def __init__(self):
        self.calls = []
        self.inside = []           # non-empty while conv2d_rows runs (second test)

    def _log(self, entry, **kw):
        self.calls.append((entry, kw, bool(self.inside)))

    def conv2d_nhwc_bf16x3(self, x, w_hi, w_lo, nhw, ksize, scale=None, shift=None, residual=None, relu=False, out=None):
        assert x.shape[0] == nhw[0] * nhw[1] * nhw[2] and out is None
        self._log("nhwc", mode=relu, k=ksize, residual=residual is not None)
        return torch.zeros(x.shape[0], w_hi.shape[1])

    def _ex(self, entry, x, w_hi, nhw, ksize, stride, transposed, residual, relu, relu_after_add, out, col0, softmax_cols):
        N, H, W = nhw
        assert x.shape[0] == N * H * W
        OH, OW = (2 * H, 2 * W) if transposed else ((H + stride - 1) // stride, (W + stride - 1) // stride)
        self._log(entry, k=ksize, stride=stride, transposed=transposed, residual=residual is not None, relu=relu,
                  relu_after_add=relu_after_add, col0=col0, softmax_cols=softmax_cols, out=out is not None)
        return out if out is not None else torch.zeros(N * OH * OW, w_hi.shape[1])

    def conv2d_nhwc_ex_bf16x3(self, x, w_hi, w_lo, nhw, ksize, stride=1, transposed=False, scale=None, shift=None, residual=None,
                              relu=False, relu_after_add=False, out=None, col0=0, softmax_cols=0):
        assert transposed or stride == 1 or (nhw[1] % 2 == 0 and nhw[2] % 2 == 0)          # the entry refuses odd maps at stride 2
        return self._ex("ex", x, w_hi, nhw, ksize, stride, transposed, residual, relu, relu_after_add, out, col0, softmax_cols)

    def conv2d_nhwc_strided_bf16x3(self, x, w_hi, w_lo, nhw, ksize, stride=2, scale=None, shift=None, residual=None, relu=False,
                                   relu_after_add=False, out=None, col0=0, softmax_cols=0):
        return self._ex("strided", x, w_hi, nhw, ksize, stride, False, residual, relu, relu_after_add, out, col0, softmax_cols)

    def pack_conv_weight(self, w, transpose=False, flip=False, pad_rows=1, pad_cols=1, out=None):
        co, ci, k = w.shape[0], w.shape[1], w.shape[2]
        p = torch.zeros((k * k, ci, co) if transpose else (k * k, co, ci), dtype=torch.bfloat16)
        return p, p

    def frozen_norm_act_backward(self, dy, y, scale, relu=False, want_gres=False):
        return dy.clone(), (dy.clone() if want_gres else None)


def _planes(k, cout=C, cin=C):
    p = torch.zeros(k * k, cout, cin, dtype=torch.bfloat16)
    return p, p


def _rows(nhw, c=C):
    return torch.zeros(nhw[0] * nhw[1] * nhw[2], c)


EX = dict(stride=1, transposed=False, residual=False, relu=True, relu_after_add=False, col0=0, softmax_cols=0, out=False)
# name -> (k, nhw, conv2d_rows keywords, (entry, what the entry must have been told))
TABLE = {
    "a": (3, (2, 6, 7), dict(), ("nhwc", dict(mode=1, k=3, residual=False))),
    "b": (1, (2, 6, 7), dict(relu=False), ("nhwc", dict(mode=0, k=1, residual=False))),
    "c": (3, (2, 6, 7), dict(residual=C), ("nhwc", dict(mode=2, k=3, residual=True))),
    "d": (1, (2, 6, 7), dict(relu=False, residual=C), ("nhwc", dict(mode=0, k=1, residual=True))),
    "e": (1, (2, 6, 7), dict(relu=False, residual=C, relu_after_add=True),
          ("ex", dict(EX, k=1, residual=True, relu=False, relu_after_add=True))),
    "f": (3, (2, 6, 7), dict(residual=2 * C), ("ex", dict(EX, k=3, residual=True))),
    "g": (3, (2, 6, 7), dict(out=2 * C, col0=C), ("ex", dict(EX, k=3, col0=C, out=True))),
    "h": (3, (2, 6, 7), dict(relu=False, softmax_cols=12), ("ex", dict(EX, k=3, relu=False, softmax_cols=12))),
    "i": (3, (2, 8, 8), dict(stride=2), ("ex", dict(EX, k=3, stride=2))),
    "j": (3, (2, 5, 8), dict(stride=2), ("strided", dict(EX, k=3, stride=2))),
    "k": (1, (2, 5, 7), dict(stride=2), ("strided", dict(EX, k=1, stride=2))),
    "l": (3, (2, 5, 7), dict(stride=2, transposed=True), ("ex", dict(EX, k=3, stride=2, transposed=True))),
}


def _out_nhw(nhw, stride, transposed):
    N, H, W = nhw
    return (N, 2 * H, 2 * W) if transposed else (N, (H + stride - 1) // stride, (W + stride - 1) // stride)


@pytest.mark.parametrize("case", sorted(TABLE))
def test_conv2d_rows_follows_the_table(monkeypatch, case):
    from sgcdet_amd import ext
    from sgcdet_amd.plugin.conv_plan import conv2d_rows
    rec = RecordingOps()
    monkeypatch.setattr(ext, "ops", lambda: rec)
    k, nhw, kw, want = TABLE[case]
    kw = dict(kw)
    onhw = _out_nhw(nhw, kw.get("stride", 1), kw.get("transposed", False))
    for name in ("residual", "out"):                             # the table gives their widths
        if name in kw:
            kw[name] = _rows(onhw, kw[name])
    y = conv2d_rows(_rows(nhw), *_planes(k), nhw, k, **kw)
    assert [(e, a) for e, a, _ in rec.calls] == [want]
    assert y.shape == (onhw[0] * onhw[1] * onhw[2], 2 * C if "out" in kw else C)
    assert "out" not in kw or y is kw["out"]


def _conv_bn(k, stride):
    torch.manual_seed(k + stride)
    conv, bn = torch.nn.Conv2d(C, C, k, stride=stride, padding=k // 2, bias=False), torch.nn.BatchNorm2d(C).eval()
    conv.weight.requires_grad_(False)                            # the input gradient alone: the weight gradient has an entry of its own
    return conv, bn


# the layer forms of the ResNet blocks: (k, stride, nhw, call keywords) -> forward entry, input-gradient entry
CALLERS = {
    "a": (3, 1, (2, 6, 7), dict(), ("nhwc", dict(mode=1, k=3, residual=False)), ("nhwc", dict(mode=0, k=3, residual=False))),
    "e": (1, 1, (2, 6, 7), dict(relu=False, residual=True, relu_after_add=True),
          ("ex", dict(EX, k=1, residual=True, relu=False, relu_after_add=True)), ("nhwc", dict(mode=0, k=1, residual=False))),
    "i": (3, 2, (2, 8, 8), dict(), ("ex", dict(EX, k=3, stride=2)), ("ex", dict(EX, k=3, stride=2, transposed=True, relu=False))),
    "j": (3, 2, (2, 5, 8), dict(), ("strided", dict(EX, k=3, stride=2)), ("ex", dict(EX, k=3, stride=2, transposed=True, relu=False))),
    "k": (1, 2, (2, 5, 7), dict(relu=False), ("strided", dict(EX, k=1, stride=2, relu=False)), ("nhwc", dict(mode=0, k=1, residual=False))),
}


@pytest.mark.parametrize("case", sorted(CALLERS))
def test_both_callers_reach_the_entries_only_through_conv2d_rows(monkeypatch, case):
    """``Conv2dSpec.__call__`` and ``FrozenConv2d`` (``FrozenNormConv2dFunction``: forward and the three input-gradient forms) on
    the same layer: every entry call happens inside ``conv2d_rows``, one per call of it, and both forwards take the same entry."""
    from sgcdet_amd import ext
    from sgcdet_amd.plugin import conv_plan
    rec = RecordingOps()
    monkeypatch.setattr(ext, "ops", lambda: rec)
    real, n_rule = conv_plan.conv2d_rows, []

    def spy(*a, **kw):
        n_rule.append(1)
        rec.inside.append(1)
        try:
            return real(*a, **kw)
        finally:
            rec.inside.pop()
    monkeypatch.setattr(conv_plan, "conv2d_rows", spy)
    k, stride, nhw, kw, want_fwd, want_dx = CALLERS[case]
    onhw = _out_nhw(nhw, stride, False)
    kw = dict(kw)
    if kw.get("residual"):
        kw["residual"] = _rows(onhw)
    conv, bn = _conv_bn(k, stride)

    spec = conv_plan.Conv2dSpec(conv, bn)
    spec.w_hi = spec.w_lo = spec.w.to(torch.bfloat16)            # the planes are split where the kernels run; the rule reads their shape
    y, got_nhw = spec(_rows(nhw), nhw, **kw)
    assert got_nhw == onhw and y.shape == (onhw[0] * onhw[1] * onhw[2], C)
    assert [(e, a) for e, a, _ in rec.calls] == [want_fwd]

    x = _rows(nhw).requires_grad_(True)
    y, got_nhw = conv_plan.FrozenConv2d(conv, bn)(x, nhw, **kw)
    assert got_nhw == onhw and y.shape == (onhw[0] * onhw[1] * onhw[2], C)
    assert [(e, a) for e, a, _ in rec.calls] == [want_fwd, want_fwd]
    y.sum().backward()
    assert x.grad.shape == x.shape
    assert [(e, a) for e, a, _ in rec.calls] == [want_fwd, want_fwd, want_dx]
    assert all(inside for _, _, inside in rec.calls) and len(n_rule) == len(rec.calls) == 3
