"""The buffer harness on the CPU (tests/buffer_contract.py, DESIGN.md "Buffers"): stand-in "kernels" with one fault each must make
``run_case`` fail for that fault's own reason; the allocator patch is undone after an exception; the case table covers every entry
point of sgcdet_amd/_abi.py that writes device memory; and the whole table runs against the oracle, which checks the table's builders,
references and defined extents -- and the oracle's own loops for the same faults -- before anything goes to a GPU."""
import pytest
import torch

import buffer_contract as bc
from buffer_contract import Case, run_case

ROWS, C, CP = 5, 6, 8          # the stand-in: y[ROWS, CP] = 2 x + 1 in the first C columns, 0 in the padded ones


def _build():
    return dict(x=torch.randn(ROWS, C, generator=torch.Generator().manual_seed(1)))


def _ref(i):
    return dict(y=torch.nn.functional.pad(2 * i["x"].double() + 1, (0, CP - C)))


def _correct(ops, t):
    y = torch.empty(ROWS, CP)
    ws = torch.empty(ROWS, C)
    ws.copy_(t["x"])                      # the workspace is written before it is read
    y[:, :C] = 2 * ws + 1
    y[:, C:] = 0
    return dict(y=y)


def _last_row_unwritten(ops, t):
    y = _correct(ops, t)["y"]
    y[ROWS - 1] = torch.empty(CP)         # as left by the allocator
    return dict(y=y)


def _padded_column_unwritten(ops, t):
    y = _correct(ops, t)["y"]
    y[:, CP - 1] = torch.empty(ROWS)
    return dict(y=y)


def _workspace_read_before_written(ops, t):
    y = _correct(ops, t)["y"]
    ws = torch.empty(ROWS, C)
    y[:, :C] += (ws > 1.0).float() * 1e-7      # garbage consumed and compared away: NaN > 1 is false, 3e30 > 1 is true
    return dict(y=y)


def _past(y, offset):
    return torch.as_strided(y, (1,), (1,), y.storage_offset() + offset)


def _writes_past_the_end(ops, t):
    y = _correct(ops, t)["y"]
    _past(y, y.numel()).fill_(1.0)
    return dict(y=y)


def _writes_before_the_start(ops, t):
    y = _correct(ops, t)["y"]
    _past(y, -1).fill_(1.0)
    return dict(y=y)


def _reads_past_the_input(ops, t):
    y = _correct(ops, t)["y"]
    x = t["x"]
    y[ROWS - 1, :C] += 0.0 * torch.as_strided(x, (C,), (1,), x.storage_offset() + ROWS * C)       # the row behind the last, weight 0
    return dict(y=y)


def _not_allocated_through_the_patch(ops, t):
    torch.empty(ROWS, C).copy_(t["x"])           # a workspace through the patch, the result through torch.zeros
    return dict(y=torch.nn.functional.pad(2 * t["x"] + 1, (0, CP - C)))


def _returns_its_input(ops, t):
    torch.empty(ROWS, C).copy_(t["x"])
    return dict(y=t["x"])                        # a guarded input is not an allocation of the wrapper's


def _nothing_allocated_through_the_patch(ops, t):
    return dict(y=torch.nn.functional.pad(2 * t["x"] + 1, (0, CP - C)))


MUTANTS = [
    (_last_row_unwritten, r"'y': 8 elements of the defined extent were not written .* first at \(4, 0\)"),
    (_padded_column_unwritten, r"'y': 5 elements of the defined extent were not written .* first at \(0, 7\)"),
    (_workspace_read_before_written, r"differs between the sentinel kinds .* depends on what the memory held"),
    (_writes_past_the_end, r"guard band damaged: allocation 1 .* byte 2 of the guard after it"),       # 1.0f and the NaN differ from their third byte on
    (_writes_before_the_start, r"guard band damaged: allocation 1 .* byte 4094 of the guard before it"),
    (_reads_past_the_input, r"non-finite under BOTH sentinel kinds, first at \(4, 0\): an input was read beyond its extent"),
    (_not_allocated_through_the_patch, r"vacuous: output 'y' was not allocated through the patched functions"),
    (_returns_its_input, r"vacuous: output 'y' was not allocated through the patched functions"),
    (_nothing_allocated_through_the_patch, r"vacuous: nothing was allocated through the patched functions"),
]


def test_a_correct_stand_in_passes():
    got = run_case(Case("stand-in", (), _build, _correct, ref=_ref, tol=1e-6), None, "cpu")
    assert torch.equal(got["A"]["y"], got["B"]["y"])


@pytest.mark.parametrize("kernel,message", MUTANTS, ids=[m[0].__name__.strip("_") for m in MUTANTS])
def test_every_fault_class_fails_for_its_own_reason(kernel, message):
    with pytest.raises(AssertionError, match=message):
        run_case(Case("stand-in", (), _build, kernel, ref=_ref, tol=1e-6), None, "cpu")


def test_a_write_into_the_neighbours_of_a_caller_range_is_seen():
    """The caller-provided form: the launch owns columns [2, 2 + C) of a wider buffer."""
    def run(spill):
        def f(ops, t):
            buf = torch.empty(ROWS, 12)
            buf[:, 2:2 + C + spill] = torch.nn.functional.pad(2 * t["x"] + 1, (0, spill))
            return dict(buf=buf)
        return f
    cols = torch.zeros(ROWS, 12, dtype=torch.bool)
    cols[:, 2:2 + C] = True
    kw = dict(ref=lambda i: dict(buf=torch.nn.functional.pad(2 * i["x"].double() + 1, (2, 12 - 2 - C))), tol=1e-6,
              extent=lambda r, i: dict(buf=cols), keep=lambda r, i: dict(buf=~cols))
    run_case(Case("range", (), _build, run(0), **kw), None, "cpu")
    with pytest.raises(AssertionError, match=r"5 elements outside the range the launch owns were written, first at \(0, 8\)"):
        run_case(Case("range", (), _build, run(1), **kw), None, "cpu")


def test_an_empty_extent_is_refused():
    with pytest.raises(AssertionError, match="empty defined extent"):
        run_case(Case("stand-in", (), _build, _correct, ref=_ref, extent=lambda r, i: dict(y=torch.zeros(ROWS, CP, dtype=torch.bool))), None, "cpu")


def test_the_allocators_are_restored_after_an_exception_and_every_form_is_guarded():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with pytest.raises(ZeroDivisionError):
        with bc.prefilled("A") as ledger:
            assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[3]
            a = torch.empty(3, 4)
            b = torch.empty((2, 5), dtype=torch.int32)
            c = torch.empty_like(a.t())
            d = torch.empty_strided((3, 2), (1, 4), dtype=torch.float16)
            e = a.new_empty((7,), dtype=torch.uint8)
            f = torch.empty_like(b, dtype=torch.bfloat16)
            assert ledger.n_allocations == 6 and all(ledger.owns(t) for t in (a, b, c, d, e, f)) and not ledger.owns(torch.zeros(3))
            assert not a._is_view() and not c._is_view()            # tensors of their own: a Function may return them, ReLU may work in place
            assert a.is_contiguous() and c.stride() == torch.empty_like(a.t()).stride() == (1, 4) and d.stride() == (1, 4)
            assert bool(torch.isnan(a).all()) and bool(torch.isnan(d).all()) and bool(torch.isnan(f).all()) and f.shape == (2, 5)
            assert bool((b.view(torch.uint8) == 0xA5).all()) and bool((e == 0xA5).all())
            assert all(t.data_ptr() % 64 == 0 for t in (a, b, c, d, e, f))
            assert ledger.guards_intact()
            d.fill_(1.0)                                            # every element of a strided interior, nothing else
            assert ledger.guards_intact()
            torch.as_strided(e, (1,), (1,), e.storage_offset() + 7).fill_(0)
            assert not ledger.guards_intact() and ledger.damaged()[0][:3] == (4, "after", 0)
            1 / 0
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before
    with bc.prefilled("B") as ledger:
        assert float(torch.empty(2)[0]) == pytest.approx(3e30, rel=1e-6) and float(torch.empty(2, dtype=torch.float16)[1]) == 6e4
        assert bool((torch.empty(2, dtype=torch.int64).view(torch.uint8) == 0x5A).all())
    g = bc.guarded_input(torch.arange(6, dtype=torch.float32).view(2, 3))
    assert g.tolist() == [[0, 1, 2], [3, 4, 5]] and bool(torch.isnan(torch.as_strided(g, (2,), (7,), g.storage_offset() - 1)).all())


# ---- the case table ---------------------------------------------------------------------------------------------------------------
NO_DEVICE_OUTPUT = {"sgc_abi_version", "sgc_backend", "sgc_last_error", "sgc_set_tuning", "sgc_set_conv_products", "sgc_get_conv_products",
                    "sgc_tile_window", "sgc_dfa3d_backward_binned_lds_bytes"}


def test_every_entry_point_that_writes_device_memory_has_a_case():
    from sgcdet_amd import _abi
    from buffer_cases import CASES
    names = set()
    for table in (_abi.SIGNATURES, _abi.INTROSPECTION, _abi.TRAIN_SIGNATURES, _abi.TRAIN_INTROSPECTION, _abi.IMAGE_SIGNATURES,
                  _abi.IMAGE_INTROSPECTION):
        names |= set(table)
    assert NO_DEVICE_OUTPUT <= names
    excluded = {n for n in names if n in NO_DEVICE_OUTPUT or n.endswith(("_supported", "_workspace_floats", "_workspace_bytes"))}
    covered = set()
    for case in CASES:
        assert case.entries, f"{case}: names no entry point"
        assert set(case.entries) <= names, f"{case}: unknown entry point {set(case.entries) - names}"
        covered |= set(case.entries)
    assert not (covered & excluded)
    uncovered = sorted(names - excluded - covered)
    assert not uncovered, f"{len(uncovered)} entry points that write device memory have no case: {uncovered}"
    ids = [c.name for c in CASES]
    assert len(ids) == len(set(ids))


def test_every_region_left_unasserted_names_the_header_sentence_that_declares_it():
    """Undefined regions are named, not guessed: a case that restricts an output's extent says where the public headers declare the rest
    undefined, and that header holds the entry's name."""
    import os
    from buffer_cases import CASES
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    text = {f: open(os.path.join(inc, f)).read() for f in os.listdir(inc)}
    n = 0
    for case in CASES:
        if case.extent is None:
            continue
        n += 1
        assert case.undefined, f"{case}: restricts an extent without naming the header sentence"
        header = case.undefined.split(",")[0].split(":")[0].strip()
        assert header in text, f"{case}: {header} is no public header"
        assert any(e in text[header] for e in case.entries), f"{case}: {header} does not declare {case.entries}"
    assert n >= 12
    tails = text["sgcdet_amd.h"]
    for phrase in ("Capacity tails", "pair_cam / pair_q beyond totals[0]", "valid_index beyond totals[1]", "keep beyond n_keep[0]", "keep[c] beyond n_keep[c]",
                   "NOT written: allocate them zeroed"):
        assert phrase in tails, phrase
    assert "grad is NOT written" in text["sgcdet_amd_train.h"]


def _cpu_cases():
    from buffer_cases import CASES
    return [c for c in CASES if c.only is None]


@pytest.mark.parametrize("case", _cpu_cases(), ids=lambda c: c.name)
def test_case_table_against_the_oracle(case, oracle_ops):
    """Every case with an oracle twin through the oracle: builders, references and extents of the table, and the oracle's own loops.
    A case whose reference IS the oracle is held to points 1, 3, 4 and 5 and to finiteness here (its values are pinned to torch by
    tests/test_oracle_*.py); one with a float64 formulation to all five."""
    run_case(case, oracle_ops, "cpu", ref_ops=None)


def test_gpu_only_cases_build_their_inputs_and_float64_references():
    """The training-only and image-side cases have no oracle twin to run here: their builders and float64 formulations at least run,
    and every reference tensor is finite."""
    from buffer_cases import CASES
    n = 0
    for case in CASES:
        if case.only == "cuda" and case.ref is not None:
            ref = case.reference(None)
            assert all(bool(torch.isfinite(v.double()).all()) for v in ref.values()), case.name
            n += 1
    assert n > 30


def test_mask_kernels_of_the_oracle_against_torch(oracle_ops):
    from buffer_cases import check_mask_kernels
    check_mask_kernels(oracle_ops, "cpu")
