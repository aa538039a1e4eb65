"""CPU checks of SyncBatchNorm on the row kernels (include/sgcdet_amd_syncbn.h, ``functions.SyncBatchNormRowsFunction``,
``conv_plan.SYNCBN_ROWS_HIP``): the new header equals its binding table, stays apart from the others and is exported;
every new entry has a buffer case with a finite float64 reference; the merge the kernels evaluate (Chan's step on [mean | M2 | count]
in rank order) and the local-sum backward hold in float64 against the concatenation; CPU rows do not see the switch; the count limit
sends an oversized call to the torch formulation."""
import copy
import os
import re
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgc_bn_rows_sync_stats", "sgc_bn_rows_sync_apply", "sgc_bn_rows_sync_backward_sums", "sgc_bn_rows_sync_backward_apply")
HEADER = "sgcdet_amd_syncbn.h"


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sgc_[a-z0-9_]+)\s*\(", text)))


def test_header_equals_its_table_and_the_library_exports_it():
    from sgcdet_amd import _abi, build
    new = set(_abi.SYNCBN_SIGNATURES) | set(_abi.SYNCBN_INTROSPECTION)
    assert _declared(HEADER) == sorted(new) == sorted(NEW) and not _abi.SYNCBN_INTROSPECTION
    old = set()
    for table in (_abi.SIGNATURES, _abi.INTROSPECTION, _abi.TRAIN_SIGNATURES, _abi.TRAIN_INTROSPECTION, _abi.IMAGE_SIGNATURES,
                  _abi.IMAGE_INTROSPECTION, _abi.DEPTH_TRAIN_SIGNATURES, _abi.DEPTH_TRAIN_INTROSPECTION, _abi.LEVEL_TRAIN_SIGNATURES,
                  _abi.LEVEL_TRAIN_INTROSPECTION, _abi.SCENE_BATCH_SIGNATURES, _abi.SCENE_BATCH_INTROSPECTION):
        old |= set(table)
    assert not new & old
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header != HEADER:
            assert not new & set(_declared(header)), header
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "sgcdet_amd.h"' in text
    # the prototypes, argument for argument (the stream included): pointers, ints, floats, int64 in the header's order
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    kinds = {"p": _abi.C.c_void_p, "i": _abi.C.c_int, "f": _abi.C.c_float, "l": _abi.C.c_int64}
    for name in NEW:
        args = re.search(r"int " + name + r"\((.*?)\);", flat).group(1).split(",")
        want = [kinds["p" if "*" in a or "sgc_stream_t" in a else "l" if "int64_t" in a else "f" if "float" in a else "i"] for a in args]
        assert _abi.SYNCBN_SIGNATURES[name] == want, name
    assert f"#define SGC_SYNCBN_MAX_WORLD {_abi.SYNCBN_MAX_WORLD}" in text and _abi.SYNCBN_MAX_COUNT == 2 ** 24
    assert _abi.ABI_VERSION == 4                                  # no existing argument list changed
    lib = _abi.Library(build.build(), train=True)                 # raises ImportError on a missing symbol
    assert all(hasattr(lib._dll, n) for n in NEW)
    plain = _abi.Library(build.build())._dll
    assert all(getattr(plain, n).argtypes is None for n in NEW)   # bound with the training tables only


def test_every_new_entry_point_has_a_buffer_case_with_a_finite_float64_reference():
    from sgcdet_amd import _abi
    from buffer_cases import CASES as OLD
    from buffer_cases_depth_train import CASES as OLD_DEPTH
    from buffer_cases_level_train import CASES as OLD_LEVEL
    from buffer_cases_syncbn import CASES
    names = set(_abi.SYNCBN_SIGNATURES)
    covered = set()
    for case in CASES:
        assert case.entries and set(case.entries) <= names, case
        assert case.only == "cuda" and case.ref is not None and case.extent is None       # the header: every output fully written
        covered |= set(case.entries)
        ref = case.reference(None)
        assert ref and all(v.dtype == torch.float64 and bool(torch.isfinite(v).all()) for v in ref.values()), case.name
    assert covered == names
    ids = [c.name for cs in (CASES, OLD, OLD_DEPTH, OLD_LEVEL) for c in cs]
    assert len(ids) == len(set(ids))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert text.count("fully written") >= 2                                               # stats and sums; y, dx, dresidual are [rows, C]


# ---- the formulas of include/sgcdet_amd_syncbn.h in float64 ---------------------------------------------------------------------------
def test_rank_order_chan_merge_and_local_sums_are_the_batch_norm_of_the_concatenation():
    from buffer_cases_syncbn import EPS, sync_inputs, sync_reference
    i = sync_inputs((77, 5, 1), 12, 1, True, 3)
    want = sync_reference(i)
    C = 12
    n = m = M2 = None
    for r in range(3):                                            # the merge kernel's loop: rank 0's values, then Chan's step per rank
        s = want[f"stats{r}"]
        mb, Mb, nb = s[:C], s[C:2 * C], float(s[2 * C])
        if n is None:
            n, m, M2 = nb, mb.clone(), Mb.clone()
            continue
        tot, d = n + nb, mb - m
        m = m + d * (nb / tot)
        M2 = M2 + Mb + d * d * n * (nb / tot)
        n = tot
    assert bool((want["stats2"][C:2 * C] == 0).all())             # a rank of one row: M2 = 0
    assert (m - want["mean"]).abs().max() < 1e-13 and (1.0 / torch.sqrt(M2 / n + EPS) - want["invstd"]).abs().max() < 1e-13
    assert abs(1.0 / n - float(want["inv_count"])) < 1e-18
    # dx of a rank from the summed local sums
    total = sum(want[f"sums{r}"] for r in range(3))
    w = i["w"].double()
    pre = want["pre"].split([77, 5, 1])
    for r in range(3):
        g = i["dys"][r].double() * (pre[r] > 0)
        xhat = (i["xs"][r].double() - want["mean"]) * want["invstd"]
        dx = w * want["invstd"] * (g - total[:C] / n - xhat * total[C:] / n)
        assert (dx - want[f"dx{r}"]).abs().max() < 1e-12 * max(1.0, float(want[f"dx{r}"].abs().max()))
        assert (g - want[f"dres{r}"]).abs().max() == 0


# ---- the switch ------------------------------------------------------------------------------------------------------------------------
def test_cpu_rows_do_not_see_the_switch(monkeypatch):
    from sgcdet_amd import dist as sd
    from sgcdet_amd.plugin import conv_plan
    assert conv_plan.SYNCBN_ROWS_HIP == (os.environ.get("SGC_SYNCBN_ROWS_HIP", "0") == "1")
    grid, C = (4, 3, 2), 8
    g = torch.Generator().manual_seed(4)
    bn0 = sd.SyncBatchNorm3d(C).train()
    rows, res, dy = (torch.randn(24, C, generator=g) for _ in range(3))
    results = []
    for flag in (False, True):
        monkeypatch.setattr(conv_plan, "SYNCBN_ROWS_HIP", flag)
        bn = copy.deepcopy(bn0)
        x = rows.clone().requires_grad_(True)
        assert not conv_plan._syncbn_on_kernels(bn, x)
        y = conv_plan.bn_rows(bn, x, grid, residual=res, relu=True)
        y.backward(dy)
        results.append((y.detach(), x.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var, bn.num_batches_tracked))
    for a, b in zip(*results):
        assert torch.equal(a, b)
    assert int(results[0][6]) == 1


def test_the_count_limit_sends_an_oversized_call_to_the_torch_formulation(monkeypatch):
    from sgcdet_amd import dist as sd
    from sgcdet_amd.plugin import conv_plan
    fits = conv_plan.syncbn_counts_fit
    assert fits(1, 1) and fits(2 ** 24 - 1, 1) and not fits(2 ** 24, 1) and not fits(0, 1)
    assert fits(2 ** 23 - 1, 2) and not fits(2 ** 23, 2) and not fits(2 ** 22, 4) and fits(2 ** 22 - 1, 4)
    assert fits(1, 1024) and not fits(1, 1025) and not fits(1, 0)
    # the dispatch asks exactly this predicate: stand-ins for CUDA rows of 2^24 - 1 and of 2^24 rows
    monkeypatch.setattr(conv_plan, "SYNCBN_ROWS_HIP", True)
    bn = sd.SyncBatchNorm3d(8).train()
    rows = lambda n, **kw: types.SimpleNamespace(**dict(dict(is_cuda=True, dtype=torch.float32, shape=(n, 8)), **kw))      # noqa: E731
    assert conv_plan._syncbn_on_kernels(bn, rows(2 ** 24 - 1))
    assert not conv_plan._syncbn_on_kernels(bn, rows(2 ** 24))
    # and the other conditions of the branch, one at a time
    assert not conv_plan._syncbn_on_kernels(bn, rows(100, is_cuda=False)) and not conv_plan._syncbn_on_kernels(bn, rows(100, dtype=torch.float16))
    assert not conv_plan._syncbn_on_kernels(bn, rows(100, shape=(100, 6)))
    assert not conv_plan._syncbn_on_kernels(copy.deepcopy(bn).eval(), rows(100))
    assert not conv_plan._syncbn_on_kernels(sd.SyncBatchNorm3d(8, momentum=None).train(), rows(100))
    assert not conv_plan._syncbn_on_kernels(sd.SyncBatchNorm3d(8, affine=False).train(), rows(100))
    assert not conv_plan._syncbn_on_kernels(torch.nn.BatchNorm3d(8).train(), rows(100))
    monkeypatch.setattr(conv_plan, "SYNCBN_ROWS_HIP", False)
    assert not conv_plan._syncbn_on_kernels(bn, rows(100))
