"""Decision edges of the plane sweep (``sgc_plane_sweep_corr``, csrc/plane_sweep.hip; ``sgc_plane_sweep_corr_backward``,
csrc/plane_sweep_bwd.hip): case builders, a float64 reference written from the definition, and deliberately wrong variants of it.

The position rule (``plane_sweep_corners``, csrc/sample_geom.hpp), in fp32 and in this order:

    (px, py, pz) = rot @ (x, y, 1) * depth + trans;  u = px / pz;  gx = u / ((W - 1) / 2) - 1;  ix = ((gx + 1) * W - 1) / 2

    a sample contributes iff -1 < ix < W and -1 < iy < H (false for NaN / inf; there is NO gate on pz);  x0 = floor(ix);
    each of the four corners (x0 | x0 + 1, y0 | y0 + 1) counts iff it lies on the map, with its bilinear weight;
    corr[n, d, p] = (1 / K) sum_k sum_c S[c] * f[n, p, c] / sqrt(C),   S = the weighted corner rows of view nbr[n, k].

The lattice: for T a power of two and q a multiple of a quarter pixel, u = (T - 1)(2 q + 1) / (2 T) is a short binary fraction and
every intermediate (u / half = (2 q + 1) / T, gx, ix = q) is exact in fp32 in whatever order a compiler fuses the operations -- a
kernel, the C oracle and this reference must take the same branch at every gate, and no sample has to be excused.
``assert_exact`` checks that on the fp32 tensors the kernels read.

The positions of every case come from ``walk_f32`` (the rule above, op for op in fp32); weights, sums and gradients are float64 with
plain indexing and autograd.  ``list_walk`` is the same walk as the backward's count / fill passes: list lengths, chunk counts and scan
sizes are asserted from it, never assumed.  Nothing here calls into ``oracle/`` or ``TensorOps``."""
import functools
import math

import torch

F64 = torch.float64
FWD_TOL = 2e-5        # of max(1, max |want|): test_plane_sweep_cost_volume_matches_reference_golden_and_oracle
BWD_TOL = 1e-5        # of max |ref|: test_plane_sweep_backward_* (tests/test_gpu_plane_sweep_grad.py)
VARIANTS = ("border", "trunc", "align_corners", "half_w", "pz_gate")     # deliberately wrong rules (the teeth of the tests)
PSB_CHUNK, PSB_SCAN, PSB_LONG_WAVES = 512, 2048, 4096                    # csrc/plane_sweep_bwd.hip


# --------------------------------------------------------------------------------------------------------------------
# positions
# --------------------------------------------------------------------------------------------------------------------
def walk_f32(rel, depth, H, W, variant=None):
    """The sample positions in fp32, op for op as plane_sweep_corners computes them.  rel [N, K, 3, 4], depth [D]
    -> dict(ix, iy, pz) of [N, K, D, H*W] fp32.  ``variant``: "align_corners" / "half_w" change the arithmetic."""
    N, K = rel.shape[:2]
    m = rel.float().reshape(N, K, 12)
    c = lambda i: m[:, :, i].reshape(N, K, 1, 1)                                                     # noqa: E731
    p = torch.arange(H * W)
    fx, fy = (p % W).float().view(1, 1, 1, -1), (p // W).float().view(1, 1, 1, -1)
    dep = depth.float().view(1, 1, -1, 1)
    rx, ry, rz = c(0) * fx + c(1) * fy + c(2), c(4) * fx + c(5) * fy + c(6), c(8) * fx + c(9) * fy + c(10)
    px, py, pz = rx * dep + c(3), ry * dep + c(7), rz * dep + c(11)
    u, v = px / pz, py / pz
    out = []
    for t, T in ((u, W), (v, H)):
        half = (T / 2.0) if variant == "half_w" else (T - 1) / 2.0
        g = t / torch.full_like(t, half) - 1.0                         # a tensor divisor: a true fp32 division
        if variant == "align_corners":
            out.append((g + 1.0) / 2.0 * float(T - 1))
        else:
            out.append(((g + 1.0) * float(T) - 1.0) / 2.0)
    return dict(ix=out[0], iy=out[1], pz=pz.expand_as(out[0]))


def _corners(pos, H, W, variant=None):
    """float64 corner rule -> [(pixel index clamped into the map, weight (0 where the corner does not count), counts)] x 4."""
    ix, iy = pos["ix"].double(), pos["iy"].double()
    if variant == "border":                                            # padding_mode = "border": the position is clamped
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    gate = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)                 # open on both sides; false for NaN and +-inf
    if variant == "pz_gate":
        gate = gate & (pos["pz"] > 0)
    sx, sy = torch.where(gate, ix, torch.zeros_like(ix)), torch.where(gate, iy, torch.zeros_like(iy))
    rnd = torch.trunc if variant == "trunc" else torch.floor
    x0, y0 = rnd(sx), rnd(sy)
    lx, ly = sx - x0, sy - y0
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0.long() + dx, y0.long() + dy
            ok = gate & (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            w = (lx if dx else 1 - lx) * (ly if dy else 1 - ly)
            out.append((yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1), w * ok, ok))
    return out


# --------------------------------------------------------------------------------------------------------------------
# the float64 reference
# --------------------------------------------------------------------------------------------------------------------
def correlation_f64(rows, nbr, rel, depth, H, W, variant=None, role=None):
    """corr [N, D, H, W] of rows [N, H*W, C] (float64; may require grad) from the definition.  A pair whose id lies outside [0, N)
    adds nothing and leaves the 1 / K scale alone (the guard of the backward; the forward is never given such an id).
    ``role``: "reference" / "neighbour" keep the gradient of that role of the features only."""
    N, HW, C = rows.shape
    K, D = nbr.shape[1], depth.numel()
    corners = _corners(walk_f32(rel, depth, H, W, variant), H, W, variant)
    own = rows.detach() if role == "neighbour" else rows
    views = torch.arange(N).view(N, 1, 1)
    corr = 0
    for k in range(K):
        valid = ((nbr[:, k] >= 0) & (nbr[:, k] < N)).view(N, 1, 1, 1)
        src = rows[nbr[:, k].clamp(0, N - 1).long()]                   # [N, HW, C]
        if role == "reference":
            src = src.detach()
        S = 0
        for idx, w, _ in corners:
            S = S + (w[:, k] * valid[..., 0]).unsqueeze(-1) * src[views, idx[:, k]]          # [N, D, HW, C]
        corr = corr + (S * own.view(N, 1, HW, C)).sum(-1) / math.sqrt(C)
    return (corr / K).view(N, D, H, W)


def grad_f64(rows, nbr, rel, depth, grad_corr, H, W, variant=None, role=None):
    """-> (corr, d (sum corr * grad_corr) / d rows) by float64 autograd of ``correlation_f64``."""
    f = rows.double().detach().requires_grad_(True)
    corr = correlation_f64(f, nbr, rel, depth, H, W, variant, role)
    g, = torch.autograd.grad(corr, f, grad_corr.double())
    return corr.detach(), g


# --------------------------------------------------------------------------------------------------------------------
# the backward's lists, from the same walk
# --------------------------------------------------------------------------------------------------------------------
def list_walk(nbr, rel, depth, H, W, grad_corr=None):
    """What passes 1 and 3 of the backward produce: one entry per on-image corner of every (n, k, d, p) whose id is in [0, N).
    -> dict(count [N*H*W] entries per destination row, and with ``grad_corr``: dst, src rows and the fp32 coefficient g * w)."""
    N, K = nbr.shape
    HW, D = H * W, depth.numel()
    pos = walk_f32(rel, depth, H, W)
    ix, iy = pos["ix"], pos["iy"]
    inside = (ix > -1) & (iy > -1) & (ix < W) & (iy < H)
    x0f, y0f = torch.where(inside, ix.floor(), torch.zeros_like(ix)), torch.where(inside, iy.floor(), torch.zeros_like(iy))
    lx, ly = ix - x0f, iy - y0f
    hx, hy = 1.0 - lx, 1.0 - ly
    x0, y0 = x0f.long(), y0f.long()
    valid = ((nbr >= 0) & (nbr < N)).view(N, K, 1, 1)
    base = nbr.clamp(0, N - 1).long().view(N, K, 1, 1) * HW
    src = (torch.arange(N).view(N, 1, 1, 1) * HW + torch.arange(HW).view(1, 1, 1, HW)).expand(N, K, D, HW)
    dsts, srcs, coefs = [], [], []
    for dy, wy in ((0, hy), (1, ly)):
        for dx, wx in ((0, hx), (1, lx)):
            xx, yy = x0 + dx, y0 + dy
            ok = inside & valid & (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            dsts.append((base + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1))[ok])
            if grad_corr is not None:
                g = grad_corr.float().reshape(N, 1, D, HW).expand(N, K, D, HW)
                srcs.append(src[ok])
                coefs.append((g * (wx * wy))[ok])
    dst = torch.cat(dsts)
    out = dict(count=torch.bincount(dst, minlength=N * HW), dst=dst)
    if grad_corr is not None:
        out.update(src=torch.cat(srcs), coef=torch.cat(coefs))
    return out


def chunk_count(count):
    """Work items of psb_long_kernel: a list longer than PSB_CHUNK is split into ceil(len / PSB_CHUNK) chunks."""
    long = count[count > PSB_CHUNK]
    return int(((long + PSB_CHUNK - 1) // PSB_CHUNK).sum())


def scan_blocks(n_rows):
    """Workgroup totals that psb_scan_top_kernel scans, 256 per iteration."""
    return (n_rows + PSB_SCAN - 1) // PSB_SCAN


def identical_entries(walk):
    """Entries of ``list_walk`` that have at least one twin: the same destination row, source row and coefficient bits."""
    key = torch.stack([walk["dst"], walk["src"], walk["coef"].view(torch.int32).long()], 1)
    _, counts = torch.unique(key, dim=0, return_counts=True)
    return int(counts[counts > 1].sum())


# --------------------------------------------------------------------------------------------------------------------
# warps with prescribed positions
# --------------------------------------------------------------------------------------------------------------------
def axis_row(T, a_x=0.0, a_y=0.0, b=0.0, cst=0.0, pz=1.0):
    """One row (4 numbers) of a warp with pz = ``pz`` everywhere whose position on an axis of size T is
    (a_x * x + a_y * y + b) * depth + cst pixels:  u = (2 position + 1)(T - 1) / (2 T) inverts the rule above."""
    s = (T - 1) / T
    return [pz * a_x * s, pz * a_y * s, pz * b * s, pz * (2 * cst + 1) * (T - 1) / (2 * T)]


def warp(H, W, x, y, pz=1.0):
    """[3, 4] float64: x, y = (a_x, a_y, b, cst) of ``axis_row``; the third rotation row is zero and m[11] = pz."""
    return torch.tensor([axis_row(W, *x, pz=pz), axis_row(H, *y, pz=pz), [0.0, 0.0, 0.0, pz]], dtype=F64)


def _case(name, H, W, C, nbr, rel, depth, seed, grad_corr=None, **extra):
    g = torch.Generator().manual_seed(seed)
    N, D = nbr.shape[0], len(depth)
    rows = torch.randn(N, H * W, C, generator=g)
    if grad_corr is None:
        grad_corr = torch.randn(N, D, H, W, generator=g)
    return dict(name=name, H=H, W=W, C=C, N=N, K=nbr.shape[1], D=D, rows=rows, nbr=nbr, rel=rel.float().contiguous(), rel64=rel,
                depth=torch.tensor(depth, dtype=torch.float32), grad_corr=grad_corr.contiguous(), **extra)


def _ring(N, K, own_every=None):
    """nbr[n, k] = n + 1 + k (mod N); with ``own_every``, every such view (view 0 first) is its own last neighbour."""
    nbr = (torch.arange(N).view(N, 1) + 1 + torch.arange(K).view(1, K)) % N
    if own_every:
        nbr[::own_every, K - 1] = torch.arange(N)[::own_every]
    return nbr


# --------------------------------------------------------------------------------------------------------------------
# 1. the lattice and the cases beside it
# --------------------------------------------------------------------------------------------------------------------
LATTICE_D = 25                                                        # planes per pair: 6 quarter-pixel steps short of 8 pixels


def fixed_values(T):
    """One fractional interior point, 0, T - 1, -0.5, T - 0.75."""
    return (T / 2 - 0.75, 0.0, T - 1.0, -0.5, T - 0.75)


def sweep_values(T):
    """Every quarter pixel from -1.5 to T + 0.5."""
    return [k / 4.0 for k in range(-6, 4 * T + 3)]


def lattice_case(name, H, W, K, C, seed, pz=1.0, own_every=4):
    """Every (n, k) pair sweeps one axis in quarter-pixel steps over its LATTICE_D planes (depths 1, 2, 3, ...: the position does not
    depend on the pixel) from its own start, the other axis at one of the fixed values.  ``pz`` = -1: the same positions from points
    behind the neighbour camera (px, py and pz negated)."""
    starts = []                                                       # (x of plane 0, y of plane 0, x step, y step)
    for axis, T, To in ((0, W, H), (1, H, W)):
        sweep = sweep_values(T)
        for c0 in range(0, len(sweep), LATTICE_D):
            for fv in fixed_values(To):
                starts.append((sweep[c0], fv, 0.25, 0.0) if axis == 0 else (fv, sweep[c0], 0.0, 0.25))
    while len(starts) % K:
        starts.append(starts[len(starts) % 7])
    N = len(starts) // K
    rel = torch.stack([warp(H, W, (0, 0, sx, x0 - sx), (0, 0, sy, y0 - sy), pz) for x0, y0, sx, sy in starts]).view(N, K, 3, 4)
    j = torch.arange(LATTICE_D, dtype=F64)
    st = torch.tensor(starts, dtype=F64).view(N, K, 4, 1)
    want = dict(ix=st[:, :, 0] + st[:, :, 2] * j, iy=st[:, :, 1] + st[:, :, 3] * j)                  # [N, K, D]
    return _case(name, H, W, C, _ring(N, K, own_every), rel, [float(d + 1) for d in range(LATTICE_D)], seed, want=want, pz=pz)


def assert_exact(case):
    """The warp is held exactly by fp32 and the positions recomputed op for op in fp32 ARE the intended quarter-pixel values."""
    assert torch.equal(case["rel"].double(), case["rel64"]), case["name"]
    pos = walk_f32(case["rel"], case["depth"], case["H"], case["W"])
    for a in ("ix", "iy"):
        want = case["want"][a].unsqueeze(-1).expand_as(pos[a])
        assert torch.equal(pos[a].double(), want), (case["name"], a)
    assert bool((pos["pz"] == case["pz"]).all())


def assert_lattice_coverage(case):
    """Each axis takes every quarter pixel from -1.5 to T + 0.5 against every fixed value of the other axis."""
    H, W = case["H"], case["W"]
    pts = torch.stack([case["want"]["ix"].reshape(-1), case["want"]["iy"].reshape(-1)], 1)
    seen = {(float(x), float(y)) for x, y in pts}
    for q in sweep_values(W):
        for fv in fixed_values(H):
            assert (q, fv) in seen, (case["name"], "x", q, fv)
    for q in sweep_values(H):
        for fv in fixed_values(W):
            assert (fv, q) in seen, (case["name"], "y", fv, q)


# (name, H, W, K, C, pz): K = 1, a tail of every channel template, points behind the camera; own neighbours in each
LATTICE_CASES = (("4x8-k1", 4, 8, 1, 20, 1.0), ("8x16-k2", 8, 16, 2, 65, 1.0), ("4x8-k3-behind", 4, 8, 3, 3, -1.0))

NONFINITE_KINDS = ("+inf", "-inf", "nan", "nan-x-inf-y", "huge-x", "huge-y", "one-plane")


@functools.lru_cache(maxsize=None)
def lattice(name):
    i = [c[0] for c in LATTICE_CASES].index(name)
    _, H, W, K, C, pz = LATTICE_CASES[i]
    return lattice_case(name, H, W, K, C, 40 + i, pz)


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """4 x 8 maps, K = 2.  Pair k = 0 of view n is of NONFINITE_KINDS[n]: pz == 0 with px > 0, < 0, == 0 (+inf, -inf, NaN), a finite
    position near +-1e30, and "one-plane": pz = depth - 3, zero on the third plane only, the other planes at (2.25, 1.25) from
    behind (planes 1, 2) and from the front (4, 5).  Pair k = 1 is an ordinary on-image sweep."""
    H, W, D = 4, 8, 5
    on = lambda i: warp(H, W, (0, 0, 0.25, 0.5 + i), (0, 0, 0.0, 0.75 + 0.25 * (i % 4)))              # noqa: E731
    zero = lambda px, py: torch.tensor([[0, 0, 0, px], [0, 0, 0, py], [0, 0, 0, 0]], dtype=F64)      # noqa: E731
    huge_x, huge_y = on(0).clone(), on(1).clone()
    huge_x[0, 3], huge_y[1, 3] = 1e30, -1e30
    cx, cy = axis_row(W, cst=2.25)[3], axis_row(H, cst=1.25)[3]
    one = torch.tensor([[0, 0, cx, -3 * cx], [0, 0, cy, -3 * cy], [0, 0, 1, -3]], dtype=F64)
    first = [zero(1, 1), zero(-1, 0.5), zero(0, 0), zero(0, 1), huge_x, huge_y, one]
    N = len(first)
    rel = torch.stack([torch.stack([first[n], on(n % 5)]) for n in range(N)])
    rel = rel.float().double()                                        # 1e30 is not an fp32 number: the case is its rounding
    return _case("nonfinite", H, W, 20, _ring(N, 2, 3), rel, [1.0, 2.0, 3.0, 4.0, 5.0], 47)


def assert_nonfinite_classes(case):
    """The fp32 walk puts every k = 0 pair into the class its name says."""
    pos = walk_f32(case["rel"], case["depth"], case["H"], case["W"])
    ix, iy = pos["ix"][:, 0], pos["iy"][:, 0]
    pinf, ninf = (lambda t: bool((t == math.inf).all())), (lambda t: bool((t == -math.inf).all()))
    assert pinf(ix[0]) and pinf(iy[0]) and ninf(ix[1]) and pinf(iy[1])
    assert bool(ix[2].isnan().all() and iy[2].isnan().all()) and bool(ix[3].isnan().all()) and pinf(iy[3])
    assert bool(ix[4].isfinite().all() and (ix[4] > 1e29).all()) and bool(iy[5].isfinite().all() and (iy[5] < -1e29).all())
    assert bool((iy[4] > -1).all() and (iy[4] < case["H"]).all() and (ix[5] > -1).all() and (ix[5] < case["W"]).all())
    assert bool(ix[6][2].isnan().all() and iy[6][2].isnan().all())
    others = [0, 1, 3, 4]
    assert bool((ix[6][others] == 2.25).all() and (iy[6][others] == 1.25).all())
    assert bool((pos["pz"][6, 0, :2] < 0).all() and (pos["pz"][6, 0, 3:] > 0).all())
    on = pos["ix"][:, 1]
    assert bool(((on > -1) & (on < case["W"])).any())


# --------------------------------------------------------------------------------------------------------------------
# 2. ragged shapes on real geometry (make_img_meta, as tests/test_gpu_plane_sweep_grad.py)
# --------------------------------------------------------------------------------------------------------------------
def _ragged():
    out = {}
    for C in (1, 3, 63, 64, 65, 100, 129, 200, 256):                  # every channel template (64 per lane step) and its tails
        out[f"C{C}"] = (5, C, 9, 13, 2, 5)
    for D in (1, 2, 3, 4, 5, 31, 32):                                 # plane groups of 4
        out[f"D{D}"] = (5, 65, 9, 13, 2, D)
    # pixel tiles: 64 per workgroup forward, 4 rows per workgroup backward.  257 pixels cannot be had (a prime, and H = 1 or
    # W = 1 is no case: the normalisation divides by zero there): 256 and 258 stand on both sides of it, 260 is four tiles and
    # four pixels on a map of ordinary proportions
    for H, W in ((7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (6, 43), (13, 20)):
        out[f"HW{H * W}"] = (5, 65, H, W, 2, 3)
    out["K1"] = (5, 65, 9, 13, 1, 5)
    out["K4"] = (7, 65, 9, 13, 4, 5)                                  # K = 4 needs 7 views
    return out


RAGGED = _ragged()                                                    # name -> (N, C, H, W, K, D)


@functools.lru_cache(maxsize=None)
def ragged_inputs(name):
    """-> (f_mvs [N,C,H,W], nbr [N,K], rel [N,K,3,4], depth [D], grad_corr [N,D,H,W]).  K = 1: the first neighbour of the K = 2 case
    (closest_frame_ids takes even counts only)."""
    from test_gpu_plane_sweep_grad import _random_case
    N, C, H, W, K, D = RAGGED[name]
    f_mvs, nbr, rel, depth, grad_corr = _random_case(N, C, H, W, max(K, 2), D, seed=sorted(RAGGED).index(name) + 100)
    return f_mvs, nbr[:, :K].contiguous(), rel[:, :K].contiguous(), depth, grad_corr


@functools.lru_cache(maxsize=None)
def ragged_reference(name):
    """-> (corr [N,D,H,W], grad rows [N,H*W,C]) float64: reference_correlation with warp_f64 and its autograd (reference_grad_f64)."""
    from plane_sweep_grad_contract import reference_correlation, to_rows, warp_f64
    f_mvs, nbr, rel, depth, grad_corr = ragged_inputs(name)
    f = f_mvs.double().detach().requires_grad_(True)
    corr = reference_correlation(f, nbr, rel, depth, warp=warp_f64)
    corr.backward(grad_corr.double())
    return corr.detach(), to_rows(f.grad)


# --------------------------------------------------------------------------------------------------------------------
# 3. scan and list edges of the backward
# --------------------------------------------------------------------------------------------------------------------
OFF = ((0, 0, 0, -30.5), (0, 0, 0, -30.5))                            # a warp that puts every sample off the image


def _ordinary(i):
    """On-image warps whose corners stay clear of pixel column 0: ix >= 1.125."""
    return ((0.75, 0.0, 0.0, 1.125 + 0.25 * (i % 3)), (0.0, 0.5 + 0.125 * (i % 2), 0.25, 0.375 + 0.5 * (i % 4)))


@functools.lru_cache(maxsize=None)
def list_edge_case():
    """8 x 8 maps, depths (1 x 7, 2), K = 2.  Pixel 0 of views 0 .. 4 receives exactly 511, 512, 513, 1024 and 1025 entries; the other
    rows receive the short lists of the ordinary pairs, which name views 5 .. 7 only.  Every position is (-0.5, -0.5) -- only the
    corner at pixel 0 is on the map, weight 0.25 -- or off the image:
      full        no rotation part: all 64 pixels x 8 planes                                                    512
      dep1_all    x = -20 depth + 19.5: -0.5 on the 7 planes of depth 1, -20.5 on the last                      448
      row0_dep1   the same, and y = -2 y depth - 0.5: image row 0 only                                           56
      px0_dep1    the same, and x = (-2 x - 20) depth + 19.5: pixel 0 only                                        7
      px0_dep2    x = (-2 x + 20) depth - 40.5: pixel 0 on the plane of depth 2 only                              1"""
    H = W = 8
    h = (0, 0, 0, -0.5)
    full, dep1_all = (h, h), ((0, 0, -20, 19.5), h)
    row0_dep1 = ((0, 0, -20, 19.5), (0, -2, 0, -0.5))
    px0_dep1, px0_dep2 = ((-2, 0, -20, 19.5), (0, -2, 0, -0.5)), ((-2, 0, 20, -40.5), (0, -2, 0, -0.5))
    pairs = [(0, dep1_all), (5, _ordinary(0)),          # view 0
             (0, row0_dep1), (1, full),                 # view 1
             (0, px0_dep1), (2, full),                  # ...
             (2, px0_dep2), (3, full),
             (3, full), (4, full),
             (4, full), (6, _ordinary(1)),
             (4, px0_dep2), (7, _ordinary(2)),
             (5, _ordinary(3)), (6, _ordinary(4))]
    nbr = torch.tensor([m for m, _ in pairs]).view(8, 2)
    rel = torch.stack([warp(H, W, x, y) for _, (x, y) in pairs]).view(8, 2, 3, 4)
    lengths = {0: 511, 1: 512, 2: 513, 3: 1024, 4: 1025}              # view -> entries of its pixel 0
    return _case("list-edges", H, W, 65, nbr, rel, [1.0] * 7 + [2.0], 51, lengths=lengths)


@functools.lru_cache(maxsize=None)
def identical_case():
    """8 x 8 maps, 8 planes of EQUAL depth and a grad_corr equal across planes: every entry has 7 twins with the same source row
    and the same coefficient bits.  Pixel 0 of views 0 and 1 holds 512 entries (64 groups of 8), the other lists are short."""
    H = W = 8
    full = ((0, 0, 0, -0.5), (0, 0, 0, -0.5))
    pairs = [(1, full), (2, _ordinary(0)), (2, _ordinary(1)), (0, full), (0, _ordinary(2)), (1, _ordinary(3))]
    nbr = torch.tensor([m for m, _ in pairs]).view(3, 2)
    rel = torch.stack([warp(H, W, x, y) for _, (x, y) in pairs]).view(3, 2, 3, 4)
    g = torch.randn(3, 1, H, W, generator=torch.Generator().manual_seed(52)).expand(3, 8, H, W)
    return _case("identical", H, W, 65, nbr, rel, [1.0] * 8, 53, grad_corr=g)


@functools.lru_cache(maxsize=None)
def work_list_case():
    """17 views of 32 x 32, K = 1, 32 planes of equal depth, a 4 x down-scaling warp (x / 4 + 0.125): 81 destination rows per view,
    49 of them with 64 pixels x 32 planes = 2048 entries (4 chunks), 28 with 1024 (2 chunks), 4 with 512 (not split)."""
    H = W = 32
    N = 17
    rel = warp(H, W, (0.25, 0, 0, 0.125), (0, 0.25, 0, 0.125)).view(1, 1, 3, 4).repeat(N, 1, 1, 1)
    return _case("work-list", H, W, 8, _ring(N, 1), rel, [1.0] * 32, 54)


# (name, N, H, W, K): N * H * W on and beside the scan's 2048-count block, and past 256 block totals (the carry of the top scan)
SCAN_CASES = (("rows2047", 1, 23, 89, 2), ("rows2048", 2, 32, 32, 2), ("rows2049", 1, 3, 683, 2), ("rows525312", 2, 512, 513, 1))


@functools.lru_cache(maxsize=None)
def scan_case(name):
    i = [c[0] for c in SCAN_CASES].index(name)
    _, N, H, W, K = SCAN_CASES[i]
    gentle = [((1.0, 0.0, 0.3, 0.1), (0.0, 1.0, -0.2, 0.35)), ((0.9, 0.05, 0.1, 0.3), (-0.04, 0.85, 0.2, -0.2))]
    rel = torch.stack([warp(H, W, *gentle[(n + k) % 2]) for n in range(N) for k in range(K)]).view(N, K, 3, 4)
    return _case(name, H, W, 4 if N * H * W > 4096 else 8, _ring(N, K), rel, [1.0, 1.25], 60 + i)


@functools.lru_cache(maxsize=None)
def empty_case(kind):
    """"unnamed": view 2 is nobody's neighbour; "off-image": every position is off the image."""
    H = W = 8
    nbr = torch.tensor([[1, 0], [0, 1], [0, 1]])
    rel = torch.stack([warp(H, W, *(_ordinary(i) if kind == "unnamed" else OFF)) for i in range(6)]).view(3, 2, 3, 4)
    return _case(f"empty-{kind}", H, W, 65, nbr, rel, [1.0, 1.5, 2.0], 70)


@functools.lru_cache(maxsize=None)
def id_guard_case():
    """Ids -1 and N in some pairs (the backward only).  View 3 has no valid neighbour at all."""
    H = W = 8
    nbr = torch.tensor([[1, -1], [4, 2], [3, 0], [-1, 4]])
    rel = torch.stack([warp(H, W, *_ordinary(i)) for i in range(8)]).view(4, 2, 3, 4)
    return _case("id-guard", H, W, 65, nbr, rel, [1.0, 1.5, 2.0], 71)


@functools.lru_cache(maxsize=None)
def reference(builder, *args):
    """(corr, grad rows) float64 of a case from one of the builders above: computed once, shared by the tests."""
    c = builder(*args)
    return grad_f64(c["rows"], c["nbr"], c["rel"], c["depth"], c["grad_corr"], c["H"], c["W"])


# --------------------------------------------------------------------------------------------------------------------
# comparisons
# --------------------------------------------------------------------------------------------------------------------
def check_forward(got, want, what):
    """|got - want| <= 2e-5 * max(1, max |want|) on every element: no sample is left out."""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, what
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err, bound = float((got - want).abs().max()), FWD_TOL * max(1.0, float(want.abs().max()))
    print(f"{what}: forward err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: forward {err:.3e} > {bound:.3e}"
    return err


def check_backward(got, ref, what):
    """|got - ref| <= 1e-5 * max |ref| on every element."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, what
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err, bound = float((got - ref).abs().max()), BWD_TOL * float(ref.abs().max())
    print(f"{what}: backward err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: backward {err:.3e} > {bound:.3e}"
    return err


def kernel_args(case, to=lambda t: t):
    """-> (feat rows, nbr int32, rt [N, K, 12], depth) as the entry points take them; ``to`` moves a tensor to the device."""
    N, K = case["nbr"].shape
    return (to(case["rows"].contiguous()), to(case["nbr"].to(torch.int32).contiguous()),
            to(case["rel"].reshape(N, K, 12).contiguous()), to(case["depth"].contiguous()))
