"""The cases of the scene-batched 3-D convolution passes (include/sgcdet_amd_scene_batch.h): one table for the value tests
(tests/test_gpu_conv3d_batched.py) and for the buffer contract (tests/buffer_contract.py).  Per kernel family the smallest per-scene
grid that still reaches it; the float64 references are computed once per case for three scenes and shared (two scenes = the first
two of them: the scenes are independent)."""
import functools

import torch
import torch.nn.functional as F

from buffer_contract import Case

ENTRIES = ("sgc_conv3d_cl_bf16x3_batched", "sgc_conv3d_wgrad_bf16x3_batched")
MAX_SCENES = 3


class Conv:
    """One forward case: Cin -> Cout on ``grid`` per scene, (k, s) or the transposed k2 s2 form; ``epi``: scale, shift, residual and
    the ReLU mode are set; ``ws``: the launch gets a workspace of the queried size (False: none -- a split launch then accumulates
    with float atomics)."""

    def __init__(self, name, cin, cout, grid, k=3, s=1, tr=False, epi=0, ws=True):
        self.name, self.cin, self.cout, self.grid, self.k, self.s, self.tr, self.epi, self.ws = name, cin, cout, grid, k, s, tr, epi, ws

    def __repr__(self):
        return self.name

    @property
    def out_grid(self):
        if self.tr:
            return tuple(2 * d for d in self.grid)
        pad = 0 if self.k == 2 else self.k // 2
        return tuple((d + 2 * pad - self.k) // self.s + 1 for d in self.grid)

    @property
    def taps(self):
        return 8 if self.tr else self.k ** 3


def _halo(tag, grid):
    """Cout 32 / 64 / 160: the 32-, 64- and 128-column tiles with a ragged last tile; Cin 128: channel splits, with the workspace and
    without."""
    out = []
    for cout in (32, 64, 160):
        out.append(Conv(f"halo_{tag}_32to{cout}", 32, cout, grid, epi=cout // 32 % 3))
        out.append(Conv(f"halo_{tag}_128to{cout}_ws", 128, cout, grid, epi=1))
    out.append(Conv(f"halo_{tag}_128to160_atomics", 128, 160, grid, epi=2, ws=False))
    return out


# k1 s1: 32 -> 64 is the issue's size and runs the tile kernel with one tap; the weight-stationary row GEMM takes Cin in {128, 256} with
# Cout % 128 == 0 (rows_gemm_supported), so 128 -> 128 is the case that reaches it
FWD = [Conv("tile_k1s1", 32, 64, (3, 5, 7), k=1, epi=1), Conv("rows_gemm_k1s1", 128, 128, (3, 5, 7), k=1, epi=1),
       Conv("rows_gemm_k1s1_plain", 256, 128, (3, 5, 7), k=1, epi=0)]
FWD += _halo("4x8x8", (16, 16, 8))          # exactly halo_min_m = 2048 voxels
FWD += _halo("8x8x4", (8, 8, 32))
FWD += _halo("4x4x16", (12, 12, 16))
FWD += _halo("ragged", (17, 9, 15))
FWD += [Conv("grid_10x10x4", 32, 512, (10, 10, 4), epi=1), Conv("grid_12x12x4", 32, 512, (12, 12, 4), epi=2)]
for _ws in (True, False):
    _t = "ws" if _ws else "atomics"
    FWD += [Conv(f"tile_k3s1_span_{_t}", 64, 96, (6, 5, 3), epi=1, ws=_ws),          # 90 rows per scene: a 128-row tile spans scenes
            Conv(f"tile_k3s2_10x10x4_{_t}", 64, 64, (10, 10, 4), s=2, epi=2, ws=_ws),
            Conv(f"tile_k3s2_7x5x3_{_t}", 64, 128, (7, 5, 3), s=2, epi=0, ws=_ws),
            Conv(f"tile_k1s2_{_t}", 64, 128, (6, 4, 4), k=1, s=2, epi=1, ws=_ws),
            Conv(f"tile_transposed_{_t}", 64, 96, (5, 5, 2), k=2, s=2, tr=True, epi=1, ws=_ws)]

# weight gradients: the same grids and (k, s) pairs (k2 s2: the transposed layers, x := the fine-grid tensor)
WGRAD = [Conv("wgrad_rows_k1s1", 32, 64, (3, 5, 7), k=1), Conv("wgrad_rows_k1s1_128", 128, 128, (3, 5, 7), k=1)]
for _tag, _grid in (("4x8x8", (16, 16, 8)), ("8x8x4", (8, 8, 32)), ("4x4x16", (12, 12, 16)), ("ragged", (17, 9, 15))):
    WGRAD += [Conv(f"wgrad_halo_{_tag}_32to64", 32, 64, _grid), Conv(f"wgrad_halo_{_tag}_128to160", 128, 160, _grid),
              Conv(f"wgrad_halo_{_tag}_32to32_nows", 32, 32, _grid, ws=False)]
WGRAD += [Conv("wgrad_grid_10x10x4", 32, 512, (10, 10, 4)), Conv("wgrad_grid_12x12x4", 32, 512, (12, 12, 4)),
          Conv("wgrad_tile_k3s1_span", 64, 96, (6, 5, 3)), Conv("wgrad_tile_k3s1_span_nows", 64, 96, (6, 5, 3), ws=False),
          Conv("wgrad_tile_k3s2_10x10x4", 64, 64, (10, 10, 4), s=2), Conv("wgrad_tile_k3s2_7x5x3", 64, 128, (7, 5, 3), s=2),
          Conv("wgrad_tile_k1s2", 64, 128, (6, 4, 4), k=1, s=2), Conv("wgrad_k2s2", 96, 64, (10, 10, 4), k=2, s=2)]


def _seed(c):
    return sum(ord(ch) for ch in c.name)


@functools.lru_cache(maxsize=None)
def fwd_inputs(c):
    """x [3 V, Cin], wt [taps, Cout, Cin], scale / shift [Cout], residual [3 OV, Cout] on the CPU, seeded."""
    g = torch.Generator().manual_seed(_seed(c))
    V = c.grid[0] * c.grid[1] * c.grid[2]
    og = c.out_grid
    x = torch.randn(MAX_SCENES * V, c.cin, generator=g)
    wt = torch.randn(c.taps, c.cout, c.cin, generator=g) * (1.0 / (c.taps * c.cin) ** 0.5)
    scale = torch.rand(c.cout, generator=g) + 0.5
    shift = torch.randn(c.cout, generator=g)
    res = torch.randn(MAX_SCENES * og[0] * og[1] * og[2], c.cout, generator=g)
    return dict(x=x, wt=wt, scale=scale, shift=shift, residual=res)


def _volume(rows, scenes, grid):
    return rows.view(scenes, *grid, rows.shape[1]).permute(0, 4, 1, 2, 3)


def _rows(vol):
    return vol.permute(0, 2, 3, 4, 1).reshape(-1, vol.shape[1])


def _weight(c, wt):
    if c.tr:
        return wt.view(2, 2, 2, c.cout, c.cin).permute(4, 3, 0, 1, 2)           # ConvTranspose3d [Cin, Cout, 2, 2, 2]
    return wt.view(c.k, c.k, c.k, c.cout, c.cin).permute(3, 4, 0, 1, 2)        # Conv3d [Cout, Cin, k, k, k]


def _conv64(c, x_rows, wt, scenes):
    x = _volume(x_rows.double(), scenes, c.grid)
    w = _weight(c, wt.double())
    if c.tr:
        return _rows(F.conv_transpose3d(x, w, stride=2))
    return _rows(F.conv3d(x, w, stride=c.s, padding=0 if c.k == 2 else c.k // 2))


@functools.lru_cache(maxsize=None)
def fwd_reference(c):
    """float64: the convolution of every scene on its own (the batch form of F.conv3d), then the epilogue of the case -- [3 OV, Cout]."""
    t = fwd_inputs(c)
    y = _conv64(c, t["x"], t["wt"], MAX_SCENES)
    if c.epi:
        y = y * t["scale"].double() + t["shift"].double()
        if c.epi == 2:
            y = torch.relu(y)
        y = y + t["residual"].double()
        if c.epi == 1:
            y = torch.relu(y)
    return y


def launch_fwd(ops, c, t, scenes, x=None, entry="sgc_conv3d_cl_bf16x3_batched"):
    """One launch of the case on ``scenes`` scenes through the raw entry (outputs and workspace allocated here with torch.empty, so
    that the buffer harness sees them).  ``t``: the inputs on the device, hi / lo planes included.  ``entry`` = the scene-less entry
    for the scenes = 1 comparison."""
    V = c.grid[0] * c.grid[1] * c.grid[2]
    og = c.out_grid
    OV = og[0] * og[1] * og[2]
    x = t["x"][:scenes * V] if x is None else x
    y = torch.empty((scenes * OV, c.cout), dtype=torch.float32, device=x.device)
    dll = ops.lib._dll
    n = int(dll.sgc_conv3d_batched_workspace_floats(*c.grid, c.cin, c.cout, c.k, c.s, int(c.tr), 1, scenes))
    ws = torch.empty(n, dtype=torch.float32, device=x.device) if (c.ws and n > 0) else None
    epi = (t["scale"], t["shift"], t["residual"][:scenes * OV]) if c.epi else (None, None, None)
    args = (x, t["hi"], t["lo"], *epi, y, *c.grid, c.cin, c.cout, c.k, c.s, int(c.tr), int(c.epi))
    if entry == "sgc_conv3d_cl_bf16x3_batched":
        ops._call(entry, *args, scenes, ws, n if ws is not None else 0)
    else:
        assert scenes == 1
        ops._call(entry, *args, ws, n if ws is not None else 0)
    return y


def fwd_is_atomic(ops, c, scenes):
    """Does the launch accumulate with float atomics (a split plan and no workspace)?  Then it is not bit-reproducible: the header says so."""
    n = int(ops.lib._dll.sgc_conv3d_batched_workspace_floats(*c.grid, c.cin, c.cout, c.k, c.s, int(c.tr), 1, scenes))
    return n > 0 and not c.ws


@functools.lru_cache(maxsize=None)
def wgrad_inputs(c):
    g = torch.Generator().manual_seed(_seed(c))
    V = c.grid[0] * c.grid[1] * c.grid[2]
    og = c.out_grid
    x = torch.randn(MAX_SCENES * V, c.cin, generator=g)
    dy = torch.randn(MAX_SCENES * og[0] * og[1] * og[2], c.cout, generator=g)
    return dict(x=x, dy=dy)


@functools.lru_cache(maxsize=None)
def wgrad_reference(c, scenes):
    """float64 dW [taps, Cout, Cin]: the gradient of sum(conv(x) * dy) over the first ``scenes`` scenes, i.e. the SUM of the scenes' gradients."""
    t = wgrad_inputs(c)
    V = c.grid[0] * c.grid[1] * c.grid[2]
    og = c.out_grid
    OV = og[0] * og[1] * og[2]
    w = torch.zeros(c.cout, c.cin, c.k, c.k, c.k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(_volume(t["x"][:scenes * V].double(), scenes, c.grid), w, stride=c.s, padding=0 if c.k == 2 else c.k // 2)
    (_rows(y) * t["dy"][:scenes * OV].double()).sum().backward()
    return w.grad.permute(2, 3, 4, 0, 1).reshape(c.taps, c.cout, c.cin)


def launch_wgrad(ops, c, t, scenes, x=None, entry="sgc_conv3d_wgrad_bf16x3_batched"):
    V = c.grid[0] * c.grid[1] * c.grid[2]
    og = c.out_grid
    OV = og[0] * og[1] * og[2]
    x = t["x"][:scenes * V] if x is None else x
    dy = t["dy"][:scenes * OV]
    dw = torch.empty((c.taps, c.cout, c.cin), dtype=torch.float32, device=x.device)
    n = int(ops.lib._dll.sgc_conv3d_wgrad_batched_workspace_floats(*c.grid, c.cin, c.cout, c.k, c.s, scenes))
    assert n >= 0, ops.lib.last_error()
    ws = torch.empty(n, dtype=torch.float32, device=x.device) if (c.ws and n > 0) else None
    if entry == "sgc_conv3d_wgrad_bf16x3_batched":
        ops._call(entry, x, dy, dw, *c.grid, c.cin, c.cout, c.k, c.s, scenes, ws, n if ws is not None else 0)
    else:
        assert scenes == 1
        ops._call(entry, x, dy, dw, *c.grid, c.cin, c.cout, c.k, c.s, ws, n if ws is not None else 0)
    return dw


# ---- the buffer contract -------------------------------------------------------------------------------------------------------------
TOL = 1e-4      # tests/test_gpu_conv3d.py: a bf16x3 convolution pass against the oracle / float64, in units of the tensor scale


def _fwd_case(c, scenes, atomic):
    def build():
        t = dict(fwd_inputs(c))
        t["hi"], t["lo"] = t["wt"].to(torch.bfloat16), (t["wt"] - t["wt"].to(torch.bfloat16).float()).to(torch.bfloat16)
        return t

    def ref(t):
        og = c.out_grid
        return dict(y=fwd_reference(c)[:scenes * og[0] * og[1] * og[2]])
    return Case(f"{c.name}_B{scenes}", ENTRIES[:1], build, lambda ops, t: dict(y=launch_fwd(ops, c, t, scenes)), ref=ref, tol=TOL,
                bits=not atomic, only="cuda")


def _wgrad_case(c, scenes):
    return Case(f"{c.name}_B{scenes}", ENTRIES[1:], lambda: dict(wgrad_inputs(c)), lambda ops, t: dict(dw=launch_wgrad(ops, c, t, scenes)),
                ref=lambda t: dict(dw=wgrad_reference(c, scenes)), tol=TOL, only="cuda")


def buffer_case(ops, c, scenes):
    """The ``Case`` of a table row (``ops`` answers whether the launch accumulates with float atomics)."""
    return _wgrad_case(c, scenes) if c.name.startswith("wgrad") else _fwd_case(c, scenes, fwd_is_atomic(ops, c, scenes))
