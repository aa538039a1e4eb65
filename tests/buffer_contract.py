"""Shared pieces of the buffer tests (tests/test_buffers_cpu.py, tests/test_gpu_buffers.py; DESIGN.md "Buffers"): what a kernel
finds in its output and workspace memory before the launch, and what lies next to its buffers, is controlled here.

``prefilled(kind)`` replaces torch.empty / empty_like / empty_strided / Tensor.new_empty for its duration: every allocation becomes
the interior of a sentinel-filled parent with GUARD_BYTES of guard on each side, recorded in a ledger.  GUARD_BYTES = 4096 is a design
constant: a multiple of the allocator's 512-byte alignment (interior pointers keep the alignment the vector stores assume) and four
times the widest store of one wave (64 lanes x 16 B).  Two sentinel kinds: "A" = NaN (floats) / the byte 0xA5 (integers), which shows
an unwritten or read-before-written float; "B" = a large finite value (3e30; 6e4 for fp16) / the byte 0x5A, which shows garbage that
is consumed but masked, clamped or compared away.  ``guarded_input`` puts an input into the interior of a NaN- (0xA5-) filled parent:
a read past either end that reaches an output shows as a NaN under BOTH kinds.

``run_case`` runs one ``Case`` under both kinds and asserts
  1. the check is not vacuous: the ledger recorded an allocation and every returned tensor is the ledger's, or is named in
     ``Case.accumulated`` (a caller-provided tensor the kernel accumulates into or updates in place: torch.zeros / an in-out input);
  2. inside the output's defined extent the result is finite where the reference is and within the bound of the existing test the
     case is lifted from (the reference is float64 torch or the oracle, never the code under test);
  3. the defined extent is bit-identical between the kinds (``bits``; float-atomic kernels are exempt and meet 2 under each kind);
  4. every guard band of every allocation -- outputs, workspaces, guarded inputs -- still holds its sentinel;
  5. the inputs went in guarded and 2 still holds.
The harness only observes: a damaged guard is read from the ledger after the launch completed.  The case table lives in
tests/buffer_cases.py."""
import contextlib

import torch

GUARD_BYTES = 4096
KINDS = ("A", "B")
_BYTE = {"A": 0xA5, "B": 0x5A}


def sentinel(kind, dtype):
    """The fill of ``kind`` for ``dtype``: a float value, or None for the byte pattern (integers, bool)."""
    if not dtype.is_floating_point:
        return None
    if kind == "A":
        return float("nan")
    return 6e4 if dtype == torch.float16 else 3e30


_ORIG_EMPTY = torch.empty          # guarded_input allocates with the original also inside ``prefilled``


def _itemsize(dtype):
    return torch.tensor([], dtype=dtype).element_size()


def _parent(orig_empty, numel, dtype, device, kind):
    """(raw uint8 parent, typed view of it, guard in elements): 4096 B | numel elements | 4096 B, all sentinel."""
    item = _itemsize(dtype)
    raw = orig_empty(2 * GUARD_BYTES + numel * item, dtype=torch.uint8, device=device)
    typed = raw.view(dtype)
    v = sentinel(kind, dtype)
    if v is None:
        raw.fill_(_BYTE[kind])
    else:
        typed.fill_(v)
    return raw, typed, GUARD_BYTES // item


def _interior(orig_empty, raw, guard, size, stride, dtype):
    """The tensor of ``size`` / ``stride`` (None: contiguous) that starts ``guard`` elements into ``raw``'s storage.  It is a tensor of
    its own on that storage, not a view of the parent: autograd treats it as it treats any freshly allocated output (a custom Function
    may return it and a later in-place operation may modify it)."""
    if stride is None:
        stride, n = [], 1
        for s in reversed(size):
            stride.insert(0, n)
            n *= max(int(s), 1)
    t = orig_empty(0, dtype=dtype, device=raw.device)
    t.set_(raw.untyped_storage(), guard, tuple(size), tuple(stride))
    return t


class Ledger:
    def __init__(self, kind):
        self.kind = kind
        self.records = []          # (raw parent, guard elements, numel, dtype, kind of its fill)
        self._ptrs = set()
        self._expect = {}

    def add(self, raw, guard, numel, dtype, kind=None, is_input=False):
        """``is_input``: the parent of a guarded input -- its guards are checked, but ``owns`` does not count it: a wrapper that returns
        (a view of) one of its inputs has allocated nothing through the patched functions."""
        self.records.append((raw, guard, numel, dtype, kind or self.kind))
        if not is_input:
            self._ptrs.add(raw.untyped_storage().data_ptr())

    @property
    def n_allocations(self):
        return len(self.records)

    def owns(self, t):
        return t.untyped_storage().data_ptr() in self._ptrs

    def _expected(self, dtype, device, kind):
        key = (dtype, str(device), kind)
        if key not in self._expect:
            e = torch.full((GUARD_BYTES,), _BYTE[kind], dtype=torch.uint8)
            v = sentinel(kind, dtype)
            if v is not None:
                e = torch.full((GUARD_BYTES // _itemsize(dtype),), v, dtype=dtype).view(torch.uint8)
            self._expect[key] = e.to(device)
        return self._expect[key]

    def damaged(self):
        """[(allocation number, "before" | "after", first damaged byte offset into that guard)] of every damaged guard band."""
        bad = []
        for i, (raw, guard, numel, dtype, kind) in enumerate(self.records):
            e = self._expected(dtype, raw.device, kind)
            for side, band in (("before", raw[:GUARD_BYTES]), ("after", raw[raw.numel() - GUARD_BYTES:])):
                if not torch.equal(band, e):
                    bad.append((i, side, int((band != e).nonzero()[0]), numel, dtype))
        return bad

    def guards_intact(self):
        return not self.damaged()


def _strided_extent(size, stride):
    if any(s == 0 for s in size):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(size, stride))


def _size_of(args, kw):
    size = kw.pop("size", None)
    if size is None:
        size = args[0] if len(args) == 1 and not isinstance(args[0], int) else args
    return tuple(int(s) for s in size)


@contextlib.contextmanager
def prefilled(kind):
    """Sentinel-filled, guarded allocations for the duration of the block; yields the ledger.  The originals are back afterwards,
    also after an exception.  Not for use inside a graph capture."""
    assert kind in KINDS
    ledger = Ledger(kind)
    o_empty, o_like, o_strided = torch.empty, torch.empty_like, torch.empty_strided
    own_new_empty = torch.Tensor.__dict__.get("new_empty")
    plain = (None, torch.strided)

    def make(size, stride, dtype, device):
        dtype = dtype or torch.get_default_dtype()
        device = torch.device(device) if device is not None else torch.tensor([]).device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        numel = _strided_extent(size, stride) if stride is not None else int(torch.Size(size).numel())
        raw, typed, guard = _parent(o_empty, numel, dtype, device, kind)
        ledger.add(raw, guard, numel, dtype)
        return _interior(o_empty, raw, guard, size, stride, dtype)

    def empty(*args, dtype=None, device=None, requires_grad=False, **kw):
        if kw.get("out") is not None or kw.get("pin_memory") or kw.get("layout") not in plain or kw.get("names") is not None \
                or kw.get("memory_format") not in (None, torch.contiguous_format):
            return o_empty(*args, dtype=dtype, device=device, requires_grad=requires_grad, **kw)
        t = make(_size_of(args, kw), None, dtype, device)
        return t.requires_grad_() if requires_grad else t

    def empty_like(x, *, dtype=None, device=None, requires_grad=False, memory_format=None, **kw):
        if kw.get("pin_memory") or kw.get("layout") not in plain or x.layout != torch.strided or x.is_quantized:
            return o_like(x, dtype=dtype, device=device, requires_grad=requires_grad, memory_format=memory_format or torch.preserve_format, **kw)
        size, stride = tuple(x.shape), None
        if memory_format in (None, torch.preserve_format) and not x.is_contiguous() and x.numel():
            probe = o_like(x, device="meta")                       # the strides torch itself would choose
            stride = tuple(probe.stride())
        elif memory_format not in (None, torch.preserve_format, torch.contiguous_format):
            stride = tuple(o_empty(size, device="meta", memory_format=memory_format).stride())
        t = make(size, stride, dtype or x.dtype, device if device is not None else x.device)
        return t.requires_grad_() if requires_grad else t

    def empty_strided(size, stride, *, dtype=None, device=None, requires_grad=False, **kw):
        if kw.get("pin_memory") or kw.get("layout") not in plain:
            return o_strided(size, stride, dtype=dtype, device=device, requires_grad=requires_grad, **kw)
        t = make(tuple(int(s) for s in size), tuple(int(s) for s in stride), dtype, device)
        return t.requires_grad_() if requires_grad else t

    def new_empty(self, *args, dtype=None, device=None, requires_grad=False, **kw):
        if kw.get("pin_memory") or kw.get("layout") not in plain:
            return torch._C.TensorBase.new_empty(self, *args, dtype=dtype, device=device, requires_grad=requires_grad, **kw)
        t = make(_size_of(args, kw), None, dtype or self.dtype, device if device is not None else self.device)
        return t.requires_grad_() if requires_grad else t

    torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty = empty, empty_like, empty_strided, new_empty
    try:
        yield ledger
    finally:
        torch.empty, torch.empty_like, torch.empty_strided = o_empty, o_like, o_strided
        if own_new_empty is None:
            del torch.Tensor.new_empty
        else:
            torch.Tensor.new_empty = own_new_empty


def guarded_input(t, ledger=None):
    """A copy of ``t`` in the interior of a NaN-filled (integers: 0xA5-filled) parent; recorded in ``ledger`` when given."""
    if not t.is_contiguous():
        t = t.contiguous()
    raw, typed, guard = _parent(_ORIG_EMPTY, t.numel(), t.dtype, t.device, "A")
    if ledger is not None:
        ledger.add(raw, guard, t.numel(), t.dtype, "A", is_input=True)
    inner = _interior(_ORIG_EMPTY, raw, guard, tuple(t.shape), None, t.dtype)
    inner.copy_(t)
    return inner


def _map(obj, f):
    if isinstance(obj, torch.Tensor):
        return f(obj)
    if isinstance(obj, dict):
        return {k: _map(v, f) for k, v in obj.items()}
    if isinstance(obj, (tuple, list)):
        return type(obj)(_map(v, f) for v in obj)
    return obj


class Case:
    """One kernel family at the smallest shape that reaches it.

    name         id of the case
    entries      the entry points of sgcdet_amd/_abi.py the case launches (the coverage rule reads these)
    build()      -> dict of inputs on the CPU (tensors, nested tuples / dicts of tensors, plain values), seeded
    run(ops, t)  -> dict name -> output tensor; ``t`` = the inputs on ``ops``' device, every tensor guarded
    ref          None: the reference is ``run(oracle_ops, inputs)``; else ref(inputs) -> dict name -> tensor (float64 torch)
    ref_run      None, or the function to run through the oracle in place of ``run`` (the existing test compares with another entry's twin)
    tol          bound of the existing test the case is lifted from (a float, or a dict per output): max |got - ref| over the extent
                 <= tol * max(1, max |ref|) (``unit_floor`` False: * max |ref|; "abs": tol is absolute).  Integer and bool outputs are
                 compared exactly.
    nan_values   outputs in which a NaN is a value the operation defines (only consulted where there is no reference to say where)
    check        None, or check(got, inputs): the comparison of an existing test that is not of that form, on the outputs of each kind
    extent       None, or extent(ref, inputs) -> dict name -> bool mask (or a slice / tuple of slices) of the DEFINED part of that
                 output; what it leaves out must be a region the public header declares undefined (``undefined`` names the sentence)
    keep         None, or keep(ref, inputs) -> dict name -> bool mask of elements of a caller-provided buffer the launch must NOT touch
    bits         True: the defined extent is bit-identical between the sentinel kinds; False: float atomics (the header says so)
    accumulated  outputs the caller provides: torch.zeros the kernel accumulates into, or in-out inputs
    needs        precondition(ops) run before the case (proves the family is reached), or None
    only         None, "cuda": the case has no oracle twin to run on the CPU (training-only / image-side entry points)"""

    def __init__(self, name, entries, build, run, ref=None, tol=1e-5, unit_floor=True, extent=None, keep=None, bits=True, accumulated=(),
                 needs=None, only=None, undefined=None, ref_run=None, check=None, nan_values=()):
        self.name, self.entries, self.build, self.run, self.ref = name, tuple(entries), build, run, ref
        self.tol, self.unit_floor, self.extent, self.keep, self.bits = tol, unit_floor, extent, keep, bits
        self.accumulated, self.needs, self.only, self.undefined, self.ref_run = tuple(accumulated), needs, only, undefined, ref_run
        self.check, self.nan_values = check, tuple(nan_values)
        self._inputs = self._ref = None

    def inputs(self):
        if self._inputs is None:
            self._inputs = self.build()
        return self._inputs

    def reference(self, ref_ops):
        """Computed once and shared; None when there is neither a float64 formulation nor a reference library."""
        if self._ref is None:
            if self.ref is not None:
                self._ref = _map(self.ref(self.inputs()), lambda t: t.detach().cpu())
            elif ref_ops is not None:
                self._ref = _map((self.ref_run or self.run)(ref_ops, _map(self.inputs(), lambda t: t.clone())), lambda t: t.detach().cpu())
        return self._ref

    def __repr__(self):
        return self.name


def _as_mask(sel, like):
    if sel is None:
        return torch.ones(like.shape, dtype=torch.bool)
    if isinstance(sel, torch.Tensor):
        return sel.cpu().bool().expand(like.shape) if sel.shape != like.shape else sel.cpu().bool()
    m = torch.zeros(like.shape, dtype=torch.bool)
    m[sel] = True
    return m


def _is_sentinel(t, kind):
    """Per element of the CPU tensor ``t``: does it still hold the fill of ``kind``?"""
    v = sentinel(kind, t.dtype)
    if v is None:
        raw = t.contiguous().view(torch.uint8).view(*t.shape, -1) if t.dtype != torch.bool else t.contiguous().view(torch.uint8).unsqueeze(-1)
        return (raw == _BYTE[kind]).all(-1)
    return torch.isnan(t) if kind == "A" else t == torch.tensor(v, dtype=t.dtype)


def run_case(case, ops, device, ref_ops=None):
    """Runs ``case`` through ``ops`` on ``device`` once under each sentinel kind and asserts the five points of the module docstring.
    ``ref_ops``: the reference library for cases without a float64 formulation (the oracle); None on the CPU, where the oracle is
    the code under test -- the values of such a case are then held to finiteness and to the bit identity alone."""
    if case.needs is not None:
        case.needs(ops)
    inputs = case.inputs()
    ref = case.reference(ref_ops)
    got = {}
    for kind in KINDS:
        with prefilled(kind) as ledger:
            n_before = ledger.n_allocations
            t = _map(inputs, lambda x: guarded_input(x.to(device), ledger))
            n_inputs = ledger.n_allocations - n_before
            out = case.run(ops, t)
            if device != "cpu":
                torch.cuda.synchronize()
        out = {k: v for k, v in out.items() if v is not None}
        assert out, f"{case}: the case returns no output"
        # 1. not vacuous
        assert ledger.n_allocations > n_inputs, f"{case}: vacuous: nothing was allocated through the patched functions"
        for name, v in out.items():
            assert ledger.owns(v) or name in case.accumulated, \
                f"{case}: vacuous: output '{name}' was not allocated through the patched functions (and is not declared as accumulated)"
        # 4. guards
        bad = ledger.damaged()
        assert not bad, (f"{case}, kind {kind}: guard band damaged: " + "; ".join(
            f"allocation {i} ({'input' if i < n_inputs else 'output / workspace'}, {numel} x {dtype}): byte {off} of the guard {side} it"
            for i, side, off, numel, dtype in bad))
        got[kind] = {k: v.detach().cpu().clone() for k, v in out.items()}
    if case.check is not None:
        for kind in KINDS:
            case.check(got[kind], inputs)
    names = list(got["A"])
    exts = case.extent(ref if ref is not None else got["A"], inputs) if case.extent is not None else {}
    keeps = case.keep(ref if ref is not None else got["A"], inputs) if case.keep is not None else {}
    for name in names:
        a, b = got["A"][name], got["B"][name]
        m = _as_mask(exts.get(name), a)
        assert bool(m.any()), f"{case}: output '{name}' has an empty defined extent"
        r = ref.get(name) if ref is not None else None
        if r is not None:
            assert r.shape == a.shape, f"{case}: output '{name}': shape {tuple(a.shape)} != the reference's {tuple(r.shape)}"
        # 2. written ...
        if a.dtype.is_floating_point:
            fin_ref = torch.isfinite(r.double()) if r is not None else torch.ones_like(m)
            if r is None and name in case.nan_values:
                fin_ref = ~(torch.isnan(a) & torch.isnan(b))
            na, nb = m & fin_ref & ~torch.isfinite(a), m & fin_ref & ~torch.isfinite(b)
            if bool(na.any()):
                first = tuple(int(i) for i in na.nonzero()[0])
                if bool((na & nb).any()):
                    assert False, (f"{case}: output '{name}': {int((na & nb).sum())} elements of the defined extent are non-finite under "
                                   f"BOTH sentinel kinds, first at {tuple(int(i) for i in (na & nb).nonzero()[0])}: an input was read beyond "
                                   f"its extent (a NaN of an input guard reached the output)")
                assert False, (f"{case}: output '{name}': {int(na.sum())} elements of the defined extent were not written (or were computed "
                               f"from unwritten memory): NaN under kind A, first at {first}, {float(b[first]):.6g} there under kind B")
            assert not bool(nb.any()), f"{case}: output '{name}': non-finite under kind B alone, first at {tuple(int(i) for i in nb.nonzero()[0])}"
        # ... and right
        if r is not None:
            for kind, g in (("A", a), ("B", b)):
                if a.dtype.is_floating_point:
                    cmp = m & torch.isfinite(r.double())
                    if not bool(cmp.any()):
                        continue
                    tol = case.tol[name] if isinstance(case.tol, dict) else case.tol
                    scale = float(r.double()[cmp].abs().max())
                    scale = 1.0 if case.unit_floor == "abs" else (max(1.0, scale) if case.unit_floor else scale)
                    err = float((g.double()[cmp] - r.double()[cmp]).abs().max())
                    print(f"{case} '{name}' kind {kind}: {int(cmp.sum())} of {r.numel()} elements, max|err| {err:.3e}, bound {tol * scale:.3e}")
                    assert err <= tol * scale, f"{case}: output '{name}', kind {kind}: off by {err:.3e} > {tol:.1e} * {scale:.3e}"
                else:
                    ne = m & (g != r.to(g.dtype))
                    assert not bool(ne.any()), (f"{case}: output '{name}', kind {kind}: {int(ne.sum())} elements of the defined extent differ "
                                                f"from the reference (unwritten or wrong), first at {tuple(int(i) for i in ne.nonzero()[0])}")
        # 3. independent of what the memory held
        bits = case.bits[name] if isinstance(case.bits, dict) else case.bits
        if bits:
            av, bv = (x.contiguous().view(torch.uint8 if x.dtype == torch.bool else x.dtype) for x in (a, b))
            same = ((av == bv) | ((av != av) & (bv != bv))) if a.dtype.is_floating_point else (av == bv)
            diff = m & ~same
            assert not bool(diff.any()), (f"{case}: output '{name}' differs between the sentinel kinds at {int(diff.sum())} elements of the defined "
                                          f"extent, first at {tuple(int(i) for i in diff.nonzero()[0])}: the result depends on what the memory held")
        # caller-provided buffers: the neighbours of the written range still hold the sentinel
        if name in keeps:
            k = _as_mask(keeps[name], a)
            assert bool(k.any()) and not bool((k & m).any()), f"{case}: output '{name}': bad keep mask"
            for kind, g in (("A", a), ("B", b)):
                hit = k & ~_is_sentinel(g, kind)
                assert not bool(hit.any()), (f"{case}: output '{name}', kind {kind}: {int(hit.sum())} elements outside the range the launch owns were "
                                             f"written, first at {tuple(int(i) for i in hit.nonzero()[0])}")
    return got
