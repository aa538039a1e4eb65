"""The non-finite contract on the CPU (tests/nonfinite_contract.py, DESIGN.md "Non-finite values"): the helpers themselves, and -- for
every operation that has both an oracle twin and a float64 torch formulation -- that the two yardsticks agree class for class on
poisoned input, before a GPU is involved."""
import pytest
import torch

import nonfinite_contract as nf
from nonfinite_contract import FINITE, NAN, NEG_INF, POS_INF

KINDS = ("nan", "+inf", "-inf")


# ---- the helpers -----------------------------------------------------------------------------------------------------------------------
def test_classes():
    t = torch.tensor([[0.0, float("nan"), float("inf")], [float("-inf"), -0.0, 3.4e38]])
    assert nf.classes(t).tolist() == [[FINITE, NAN, POS_INF], [NEG_INF, FINITE, FINITE]]
    assert nf.classes(t.double()).dtype == torch.int8


def test_poison_sites_and_values():
    assert nf.poison_sites(60, 8) == [(30, 7), (59, 7)]                                      # one image: its last row is the tensor's
    assert nf.poison_sites(60, 8, image_rows=20, live=5) == [(10, 4), (19, 4), (59, 4)]      # interior, end of image 0, end of the tensor
    assert nf.poison_sites(1, 4) == [(0, 3)]
    t = torch.zeros(60, 8)
    for kind, cls in (("nan", NAN), ("+inf", POS_INF), ("-inf", NEG_INF)):
        p = nf.poison(t, kind, image_rows=20, live=5)
        c = nf.classes(p)
        assert int((c != FINITE).sum()) == 3 and c[10, 4] == c[19, 4] == c[59, 4] == cls
    assert not t.any()                                                                       # a copy: the input is untouched


def test_poison_refuses_small_tensors():
    with pytest.raises(ValueError, match="too small"):
        nf.poison(torch.zeros(3, 8), "nan")                                                  # two of three rows
    with pytest.raises(ValueError, match="too small"):
        nf.poison(torch.zeros(6, 1), "nan", spread="column")                                 # the only column
    nf.poison(torch.zeros(1, 4), "nan", spread="element")                                    # one of four elements
    nf.poison(torch.zeros(6, 4), "nan", spread="column")
    with pytest.raises(ValueError):
        nf.poison(torch.zeros(4, 4, 4), "nan")
    with pytest.raises(ValueError):
        nf.poison_sites(60, 8, image_rows=25)


def test_widen_z_pairs():
    F = torch.zeros(2 * 3 * 4, 5, dtype=torch.bool)
    F.view(2, 3, 4, 5)[1, 2, 1, 3] = True                                                    # z = 1 -> the pair (0, 1)
    F.view(2, 3, 4, 5)[0, 0, 2, 0] = True                                                    # z = 2 -> the pair (2, 3)
    W = nf.widen_z_pairs(F, (2, 3, 4)).view(2, 3, 4, 5)
    assert int(W.sum()) == 4 and W[1, 2, 0, 3] and W[1, 2, 1, 3] and W[0, 0, 2, 0] and W[0, 0, 3, 0]
    with pytest.raises(ValueError):
        nf.widen_z_pairs(F[:20], (2, 3, 4))
    with pytest.raises(ValueError):
        nf.widen_z_pairs(torch.zeros(2 * 3 * 3, 5, dtype=torch.bool), (2, 3, 3))


def _ref(n=40, c=6):
    r = torch.arange(n * c, dtype=torch.float32).view(n, c) / 7
    r[3, 2] = r[4, 2] = float("nan")
    return r


def test_preconditions_fire_on_constructed_bad_cases():
    ref = _ref()
    nf.compare_exact(ref.clone(), ref, 1e-6, "ok")
    nf.compare_traced(ref.clone(), ref, 1e-6, "ok")
    clean = torch.nan_to_num(ref, nan=1.0)
    with pytest.raises(AssertionError, match="is empty"):
        nf.compare_exact(clean, clean, 1e-6, "empty F")
    with pytest.raises(AssertionError, match="is empty"):
        nf.compare_traced(clean, clean, 1e-6, "empty F")
    most = ref.clone()
    most[:20] = float("nan")
    with pytest.raises(AssertionError, match="half"):
        nf.compare_exact(most, most, 1e-6, "half")
    with pytest.raises(AssertionError, match="half"):
        nf.compare_traced(most, most, 1e-6, "half")
    # an Inf case in which no infinity survives and nothing was removed: the reference under Inf is NaN wherever it read the poison
    with pytest.raises(AssertionError, match="no infinity survives"):
        nf.compare_traced(ref.clone(), ref, 1e-6, "inf", kind="+inf", ref_kind=ref.clone())
    # all finite elements of the kernel's output fall inside the reference's non-finite set: nothing finite to compare
    got = torch.full_like(ref, float("nan"))
    with pytest.raises(AssertionError):
        nf.compare_exact(got, ref, 1e-6, "nothing finite")


def test_comparisons_catch_what_they_are_for():
    ref = _ref()
    swallowed = ref.clone()
    swallowed[3, 2] = 0.0                                                                   # the fmaxf(NaN, 0) case
    with pytest.raises(AssertionError, match="class"):
        nf.compare_exact(swallowed, ref, 1e-6, "swallowed")
    with pytest.raises(AssertionError, match="came out finite"):
        nf.compare_traced(swallowed, ref, 1e-6, "swallowed")
    leaked = ref.clone()
    leaked[30, 0] = float("nan")                                                            # a tile that read across a boundary
    with pytest.raises(AssertionError, match="outside the receptive field"):
        nf.compare_traced(leaked, ref, 1e-6, "leaked")
    off = ref.clone()
    off[10, 1] += 1.0
    with pytest.raises(AssertionError, match="finite elements off"):
        nf.compare_traced(off, ref, 1e-6, "off")
    # Inf poison: the reference keeps +Inf at one place and a ReLU removed the other; the kernel may give NaN at both, never finite at the first
    ref_inf = torch.nan_to_num(ref, nan=0.0)
    ref_inf[3, 2] = float("inf")
    nf.compare_traced(ref.clone(), ref, 1e-6, "inf as nan", kind="+inf", ref_kind=ref_inf)
    nf.compare_traced(ref_inf.clone(), ref, 1e-6, "inf kept", kind="+inf", ref_kind=ref_inf)
    with pytest.raises(AssertionError, match="came out finite"):
        nf.compare_traced(torch.nan_to_num(ref, nan=0.0), ref, 1e-6, "inf lost", kind="+inf", ref_kind=ref_inf)
    # the Winograd-z rule: the other plane of a pair may be non-finite, a third plane may not
    grid = (2, 5, 4)
    r = torch.ones(40, 6)
    r.view(2, 5, 4, 6)[1, 1, 2, 0] = float("nan")
    g = r.clone()
    g.view(2, 5, 4, 6)[1, 1, 3, 0] = float("nan")
    nf.compare_traced(g, r, 1e-6, "pair", z_pair_grid=grid)
    with pytest.raises(AssertionError, match="outside the receptive field"):
        nf.compare_traced(g, r, 1e-6, "pair")
    g.view(2, 5, 4, 6)[1, 1, 1, 0] = float("nan")
    with pytest.raises(AssertionError, match="outside the receptive field"):
        nf.compare_traced(g, r, 1e-6, "pair", z_pair_grid=grid)


# ---- the oracle and float64 torch agree class for class ------------------------------------------------------------------------------
# rows of CASES in tests/test_gpu_conv3d.py: every relu mode, a residual, a stride, the transposed form, ragged grids
CONV3D = [
    (32, 128, (10, 10, 4), 3, 1, False, True, True),
    (64, 128, (8, 6, 4), 3, 2, False, False, True),
    (64, 256, (5, 5, 2), 3, 1, False, True, True),
    (32, 32, (7, 5, 3), 3, 1, False, False, False),
    (64, 128, (5, 4, 3), 2, 2, True, False, True),
    (64, 128, (9, 7, 4), 3, 1, False, True, 2),
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CONV3D)
def test_conv3d_oracle_and_float64_torch_agree(case, kind, oracle_ops):
    for where in ("x", "shift") + (("residual",) if case[6] else ()):
        i = nf.conv3d_inputs(case, kind, where)
        got, og = oracle_ops.conv3d_cl(i["x"], i["wt"], i["grid"], i["k"], i["s"], i["tr"], i["sc"], i["sh"], i["res"], i["relu"])
        assert tuple(og) == tuple(i["og"])
        nf.compare_exact(got, nf.conv3d_torch64(i), 2e-5, f"conv3d {case} {kind} in {where}", need_nonfinite=kind == "nan")   # a ReLU may remove every -Inf


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nhw,cin,cout,k,relu,res", [((3, 15, 20), 64, 96, 3, 1, True), ((2, 8, 10), 256, 32, 1, 0, False), ((1, 7, 5), 96, 28, 3, 2, True)])
def test_conv2d_oracle_and_float64_torch_agree(nhw, cin, cout, k, relu, res, kind, oracle_ops):
    for where in ("x", "shift") + (("residual",) if res else ()):
        i = nf.conv2d_inputs(nhw, cin, cout, k, relu, res, kind, where)
        hi, lo = oracle_ops.split_bf16(i["wt"])
        got = oracle_ops.conv2d_nhwc_bf16x3(i["x"], hi, lo, nhw, k, i["sc"], i["sh"], i["res"], i["relu"])
        i["wt"] = hi.float() + lo.float()
        nf.compare_exact(got, nf.conv2d_torch64(i), 1e-4, f"conv2d {nhw} {cin}->{cout} k{k} {kind} in {where}", need_nonfinite=kind == "nan")


BN_OUTPUTS = ("y", "mean", "invstd", "rm", "rv", "dx", "dw", "db", "dres")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("rows,C", [(77, 1040), (6, 4)])
def test_bn_rows_oracle_and_float64_torch_agree(rows, C, tail, kind, oracle_ops):
    for where in ("x", "dy") + (("residual",) if tail else ()):
        d = nf.bn_inputs(rows, C, kind, where)
        got, ref = nf.bn_run(oracle_ops, d, tail), nf.bn_torch64(d, tail)
        for name in BN_OUTPUTS:
            if ref[name] is not None:
                nf.compare_exact(got[name], ref[name], 2e-4, f"bn_rows {rows}x{C} tail {tail} {kind} in {where}: {name}", need_nonfinite=False)
        if kind == "nan":                                  # the poison reached something (an infinity may leave in the ReLU or its gate)
            assert any(bool((nf.classes(ref[n]) != FINITE).any()) for n in BN_OUTPUTS if ref[n] is not None)


@pytest.mark.parametrize("kind", KINDS)
def test_layer_norm_rows_oracle_and_float64_torch_agree(kind, oracle_ops):
    rows, C = 100, 96
    g = torch.Generator().manual_seed(rows + C)
    x = nf.poison(torch.randn(rows, C, generator=g) * 3 + 0.7, kind)
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    want = torch.nn.functional.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5)
    nf.compare_exact(oracle_ops.layer_norm_rows(x, w, b, 1e-5), want, 2e-6, f"layer_norm_rows {kind}")
