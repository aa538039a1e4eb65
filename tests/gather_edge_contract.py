"""Exact gate coordinates for every form of the deformable gather (DFA3D), and a float64 reference of the operator.

The lattice: map sizes are powers of two, every coordinate is a multiple of a quarter pixel, so ``ref + off / T``,
``t * T`` and ``- 0.5`` are exact in fp32 in whatever order a kernel fuses them -- a kernel, the C oracle and this float64
reference must take the same branch at every gate, and no sample has to be excused.

The reference is written from the operator's definition (one level):

    t_im = t * T - 0.5 on every axis; a sample contributes iff -1 < t_im < T on ALL three axes;
    score_k = linear interpolation along depth of the depth distribution at pixel corner k (taps outside [0, D-1] are 0);
    out    += attn * sum_k bilinear_weight_k * score_k * value[corner k], corners outside the map contribute nothing.

Gradients are float64 autograd of that code with ``floor`` and the gate masks constant: only the corners that exist carry
terms.  Nothing here calls into ``oracle/`` or ``TensorOps``."""
import itertools

import torch

F64 = torch.float64
FWD_TOL, BWD_TOL = 1e-5, 2e-5                 # of max(1, scale): the `close` helper of tests/test_gpu_kernels.py
VARIANTS = ("inclusive", "trunc", "clamp")   # deliberately wrong sampling rules (the teeth of the tests)
ROW_HI, ROW_LO = 1e3, -1e3                    # last row / first row of every camera's value map


# --------------------------------------------------------------------------------------------------------------------
# the lattice
# --------------------------------------------------------------------------------------------------------------------
def fixed_values(T):
    """One fractional interior point, 0, T - 1, -0.5, T - 0.75."""
    return (T // 2 - 0.75, 0.0, T - 1.0, -0.5, T - 0.75)


def sweep_values(T):
    """Every quarter pixel from t_im = -1.5 to T + 0.5."""
    return [k / 4.0 for k in range(-6, 4 * T + 3)]


def lattice(H, W, D):
    """[n, 3] float64 of (h_im, w_im, d_im): each axis sweeps its full range, the other two take the fixed values."""
    dims = (H, W, D)
    rows = []
    for a in range(3):
        b, c = [k for k in range(3) if k != a]
        for va in sweep_values(dims[a]):
            for vb, vc in itertools.product(fixed_values(dims[b]), fixed_values(dims[c])):
                r = [0.0, 0.0, 0.0]
                r[a], r[b], r[c] = va, vb, vc
                rows.append(r)
    return torch.tensor(rows, dtype=F64)


def lattice_items(H, W, D, M, P, seed, multiple=1):
    """The lattice dealt to items of M * P samples.  Neighbouring lattice points share an item, so that a pair-list form can
    give the item one reference pixel and reach its samples with offsets of a few pixels.
    -> t_im [n, M, P, 3] (h, w, d) float64, ref_pix [n, 3] (h, w, d) float64 (integers inside the map)."""
    t = lattice(H, W, D)
    key = torch.floor((t + 1.5) / 4)
    order = torch.argsort(key[:, 0] * 10000 + key[:, 1] * 100 + key[:, 2], stable=True)
    t = t[order]
    spi = M * P
    n = -(-t.shape[0] // spi)
    n = -(-n // multiple) * multiple
    items = t[torch.arange(n * spi) % t.shape[0]].view(n, spi, 3)
    g = torch.Generator().manual_seed(seed)
    perm = torch.stack([torch.randperm(spi, generator=g) for _ in range(n)])
    items = torch.gather(items, 1, perm[:, :, None].expand(n, spi, 3))
    hi = torch.tensor([H - 1.0, W - 1.0, D - 1.0], dtype=F64)
    ref_pix = torch.minimum(items.median(1).values.round().clamp(min=0), hi)
    return items.view(n, M, P, 3).contiguous(), ref_pix


def interior_items(H, W, D, M, P, n, seed):
    """Random interior samples, exact in fp32 and 1/128 pixel away from every integer: t_im = (k + 0.5) / 64 in (0, T - 1)."""
    g = torch.Generator().manual_seed(seed)
    cols = [(torch.randint(0, 64 * (T - 1), (n, M, P), generator=g).to(F64) + 0.5) / 64 for T in (H, W, D)]
    t = torch.stack(cols, -1)
    hi = torch.tensor([H - 1.0, W - 1.0, D - 1.0], dtype=F64)
    return t, torch.minimum(t.view(n, -1, 3).median(1).values.round().clamp(min=0), hi)


def loc_of(t_im, H, W, D):
    """(h_im, w_im, d_im) -> normalised (x, y, z) fp32 sampling locations; exact: multiples of 1 / (4 T) (1 / (128 T))."""
    x = (t_im[..., 1] + 0.5) / W
    y = (t_im[..., 0] + 0.5) / H
    z = (t_im[..., 2] + 0.5) / D
    loc = torch.stack([x, y, z], -1)
    assert torch.equal(loc.float().double(), loc)
    return loc.float().contiguous()


def t_im_of(loc, H, W, D):
    """What a kernel computes from fp32 locations, in fp32: (h_im, w_im, d_im)."""
    loc = loc.float()
    return torch.stack([loc[..., 1] * H - 0.5, loc[..., 0] * W - 0.5, loc[..., 2] * D - 0.5], -1)


def class_counts(t_im, H, W, D):
    """Occurrences of every gate class per axis, and the rarest two-axis corner combination.
    -> ({(axis, class): count}, min over axis pairs and corner value pairs of the count)."""
    t_im = t_im.reshape(-1, 3).double()
    counts = {}
    for a, (name, T) in enumerate((("h", H), ("w", W), ("d", D))):
        t = t_im[:, a]
        for cls, v in (("-1.25", -1.25), ("-1", -1.0), ("-0.75", -0.75), ("-0.5", -0.5), ("0", 0.0), ("T-1", T - 1.0),
                       ("T-0.75", T - 0.75), ("T-0.25", T - 0.25), ("T", float(T)), ("T+0.25", T + 0.25)):
            counts[(name, cls)] = int((t == v).sum())
        counts[(name, "interior integer")] = int(((t > 0) & (t < T - 1) & (t == t.floor())).sum())
    combos = []
    dims = (H, W, D)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for va, vb in itertools.product((-0.5, 0.0, dims[a] - 1.0, dims[a] - 0.75), (-0.5, 0.0, dims[b] - 1.0, dims[b] - 0.75)):
            combos.append(int(((t_im[:, a] == va) & (t_im[:, b] == vb)).sum()))
    return counts, min(combos)


def assert_coverage(t_im, H, W, D, what=""):
    counts, combo = class_counts(t_im, H, W, D)
    thin = {k: v for k, v in counts.items() if v < 8}
    assert not thin, f"{what}: gate classes seen fewer than 8 times: {thin}"
    assert combo >= 4, f"{what}: a two-axis corner combination occurs only {combo} times"
    return counts, combo


def make_maps(N, H, W, D, M, Cm, dist_heads, seed):
    """Seeded value [N, S, M, Cm] and depth [N, S, dist_heads, D] maps (softmax over D).  The last row of every camera
    holds 1e3 and the first row -1e3: a corner that leaks across a row or a camera border moves the result by hundreds."""
    g = torch.Generator().manual_seed(seed)
    value = torch.randn(N, H * W, M, Cm, generator=g)
    dist = torch.randn(N, H * W, dist_heads, D, generator=g).mul(2).softmax(-1).contiguous()
    value[:, (H - 1) * W:] = ROW_HI
    value[:, :W] = ROW_LO
    return value.contiguous(), dist


# --------------------------------------------------------------------------------------------------------------------
# the cases the GPU tests run (tests/test_gpu_gather_edges.py); the CPU file asserts the coverage of every one
# --------------------------------------------------------------------------------------------------------------------
# (name, B, M, Cm, P, D, levels [(H, W)], dist_heads == M)
FUSED_CASES = [
    ("hot", 2, 8, 32, 4, 4, [(8, 16)], False),
    ("cm16", 2, 8, 16, 4, 8, [(16, 8)], False),
    ("scalar", 2, 2, 5, 2, 8, [(8, 16)], False),
    ("two-level", 2, 8, 32, 4, 4, [(8, 16), (4, 8)], False),
    ("two-level-rep", 2, 8, 32, 4, 4, [(8, 16), (4, 8)], True),
]
# the split `_ext` operators (depth_score_* / wms_*) take a per-head depth distribution: dist_heads == M throughout.
# "hot": the float4 path; "scalar": Cm % 4 != 0, one channel per lane and per atomic; "two-level": a non-zero level start
SPLIT_CASES = [
    ("hot", 2, 8, 32, 4, 4, [(8, 16)], True),
    ("scalar", 2, 8, 5, 4, 4, [(8, 16)], True),
    ("two-level", 2, 8, 32, 4, 4, [(8, 16), (4, 8)], True),
]
# (name, Cm, (H, W), D): N = 2 cameras, M = 8, P = 4
PAIR_CASES = [("cm32", 32, (8, 16), 4), ("cm16", 16, (16, 8), 8)]
GEOMETRY_CASES = [("c256", 256, (8, 16), 4), ("c128", 128, (16, 8), 8)]
PAIR_N, PAIR_M, PAIR_P = 2, 8, 4


def fused_inputs(case, seed=0):
    """-> dict(value, dist, shapes3, lsi, loc [B,Q,M,L,P,3], attn [B,Q,M,L,P], go [B,Q,M*Cm], t_im per level)."""
    _, B, M, Cm, P, D, levels, rep = case
    L = len(levels)
    per_level = [lattice_items(h, w, D, M, P, seed + 7 * l, multiple=B)[0] for l, (h, w) in enumerate(levels)]
    n = max(t.shape[0] for t in per_level)
    per_level = [t[torch.arange(n) % t.shape[0]] for t in per_level]
    Q = n // B
    loc = torch.stack([loc_of(t, h, w, D) for t, (h, w) in zip(per_level, levels)], 2)        # [n, M, L, P, 3]
    maps = [make_maps(B, h, w, D, M, Cm, M if rep else 1, seed + 100 + l) for l, (h, w) in enumerate(levels)]
    g = torch.Generator().manual_seed(seed + 1)
    return dict(
        value=torch.cat([m[0] for m in maps], 1).contiguous(), dist=torch.cat([m[1] for m in maps], 1).contiguous(),
        shapes3=torch.tensor([[h, w, D] for h, w in levels], dtype=torch.int64),
        lsi=torch.tensor([0] + [h * w for h, w in levels], dtype=torch.int64).cumsum(0)[:-1].contiguous(),
        loc=loc.view(B, Q, M, L, P, 3).contiguous(), attn=torch.rand(B, Q, M, L, P, generator=g),
        go=torch.randn(B, Q, M * Cm, generator=g), t_im=per_level, levels=levels, D=D)


def pair_inputs(Cm, HW, D, seed=0, interior=False, loc_heads=PAIR_M):
    """Pair-list inputs: N cameras, every (camera, voxel) pair listed, pair i = camera * Nq + voxel.
    Reference points are pixel centres, offsets multiples of a quarter pixel.  ``loc_heads`` 1: one sample set per pair,
    shared by the M channel groups of the value map (the binned backward's shared form).
    -> dict(value [N,S,M,Cm], dist [N,S,D], ref_cam [N,Nq,3], raw [n, M*P*4] = [uv (m,p,xy) | dz (m,p) | logit (m,p)],
            loc [n,M,P,3] fp32 = ref + off / (W, H, D), t_im [n,M,P,3], pair_cam, pair_q, mask)."""
    H, W = HW
    N, M, P = PAIR_N, loc_heads, PAIR_P
    if interior:
        t, ref_pix = interior_items(H, W, D, M, P, 64, seed)
    else:
        t, ref_pix = lattice_items(H, W, D, M, P, seed, multiple=N)
    n = t.shape[0]
    Nq = n // N
    off = t - ref_pix.view(n, 1, 1, 3)                                    # pixels, (h, w, d)
    ref = (ref_pix + 0.5) / torch.tensor([H, W, D], dtype=F64)            # pixel centres, (y, x, z)
    ref_cam = torch.stack([ref[:, 1], ref[:, 0], ref[:, 2]], -1).float().view(N, Nq, 3).contiguous()
    g = torch.Generator().manual_seed(seed + 1)
    uv = torch.stack([off[..., 1], off[..., 0]], -1).reshape(n, M * P * 2)
    raw = torch.cat([uv, off[..., 2].reshape(n, M * P), torch.randn(n, M * P, generator=g).double()], 1).float().contiguous()
    assert torch.equal(raw[:, :M * P * 3].double(), torch.cat([uv, off[..., 2].reshape(n, M * P)], 1))
    # the locations as a kernel forms them, in fp32
    r = ref_cam.view(n, 1, 1, 3)
    loc = torch.stack([r[..., 0] + raw[:, :M * P * 2].view(n, M, P, 2)[..., 0] / W,
                       r[..., 1] + raw[:, :M * P * 2].view(n, M, P, 2)[..., 1] / H,
                       r[..., 2] + raw[:, M * P * 2:M * P * 3].view(n, M, P) / D], -1).contiguous()
    assert torch.equal(t_im_of(loc, H, W, D).double(), t)                 # exact, whatever the order of the operations
    value, dist = make_maps(N, H, W, D, PAIR_M, Cm, 1, seed + 100)
    cam = torch.arange(N, dtype=torch.int32).repeat_interleave(Nq)
    q = torch.arange(Nq, dtype=torch.int32).repeat(N)
    return dict(value=value, dist=dist.view(N, H * W, D).contiguous(), ref_cam=ref_cam, raw=raw, loc=loc, t_im=t,
                pair_cam=cam, pair_q=q, mask=torch.ones(N, Nq, dtype=torch.uint8), n=n, H=H, W=W, D=D, M=M, P=P, N=N, Nq=Nq,
                max_offset=float(off.abs().max()))


def geometry_inputs(C, HW, D, seed=0, interior=False):
    """The geometry sample reads the map AT the reference point: the lattice goes into ``ref_cam`` itself (direct locations)."""
    H, W = HW
    N = PAIR_N
    if interior:
        t = interior_items(H, W, D, 1, 1, 128, seed)[0]
    else:
        t = lattice_items(H, W, D, 1, 1, seed, multiple=N)[0]
    n = t.shape[0]
    Nq = n // N
    ref_cam = loc_of(t.view(n, 3), H, W, D).view(N, Nq, 3).contiguous()
    value, dist = make_maps(N, H, W, D, 1, C, 1, seed + 100)
    cam = torch.arange(N, dtype=torch.int32).repeat_interleave(Nq)
    q = torch.arange(Nq, dtype=torch.int32).repeat(N)
    return dict(feat=value.view(N, H * W, C), dist=dist.view(N, H * W, D).contiguous(), ref_cam=ref_cam, t_im=t, pair_cam=cam,
                pair_q=q, mask=torch.ones(N, Nq, dtype=torch.uint8), n=n, H=H, W=W, D=D, N=N, Nq=Nq)


# --------------------------------------------------------------------------------------------------------------------
# the float64 reference
# --------------------------------------------------------------------------------------------------------------------
def _axis(t, T, variant):
    """t_im [..] float64 -> (gate, integer floor, fractional weight).  The gate and the floor are constants."""
    td = t.detach()
    low = td >= -1 if variant == "inclusive" else td > -1              # the gate is the OPEN interval (-1, T)
    i0 = (torch.trunc(td) if variant == "trunc" else torch.floor(td)).long()
    return low & (td < T), i0, t - i0


def _corner(i, T, variant):
    """Corner index -> (index clamped into the map for the read, does the corner exist)."""
    if variant == "clamp":                                             # index T read from T - 1 instead of dropped
        return i.clamp(0, T - 1), (i >= 0) & (i <= T)
    return i.clamp(0, T - 1), (i >= 0) & (i <= T - 1)


def sample_level(value, dist, hwd, start, loc, attn, bidx, variant=None):
    """One level of the operator.  value [B,S,M,Cm], dist [B,S,1|M,D] float64; loc [n,M,P,3] (x, y, z) float64;
    attn [n,M,P] | None (= 1); bidx [n] long: the map each item samples; ``start``: first pixel of the level.
    -> out [n, M, Cm], score [n, M, P, 4] in the corner order (h0,w0) (h0,w1) (h1,w1) (h1,w0)."""
    H, W, D = hwd
    n, M, P, _ = loc.shape
    gh, h0, lh = _axis(loc[..., 1] * H - 0.5, H, variant)
    gw, w0, lw = _axis(loc[..., 0] * W - 0.5, W, variant)
    gd, d0, ld = _axis(loc[..., 2] * D - 0.5, D, variant)
    gate = gh & gw & gd
    b = bidx.long().view(n, 1, 1).expand(n, M, P)
    m = torch.arange(M).view(1, M, 1).expand(n, M, P)
    dm = m if dist.shape[2] == M and M > 1 else torch.zeros_like(m)
    d0i, d0ok = _corner(d0, D, variant)
    d1i, d1ok = _corner(d0 + 1, D, variant)
    out, scores = 0, []
    for dh_, dw_ in ((0, 0), (0, 1), (1, 1), (1, 0)):
        hi, hok = _corner(h0 + dh_, H, variant)
        wi, wok = _corner(w0 + dw_, W, variant)
        pix = start + hi * W + wi
        col = dist[b, pix, dm]                                         # [n, M, P, D]
        # u, v reach the score only through floor(): the uv-through-score term that oracle/sgc_oracle.c:311 zeroes never arises
        s = col.gather(-1, d0i[..., None]).squeeze(-1) * d0ok * (1 - ld) + col.gather(-1, d1i[..., None]).squeeze(-1) * d1ok * ld
        s = s * (hok & wok & gate)
        scores.append(s)
        wgt = (lh if dh_ else 1 - lh) * (lw if dw_ else 1 - lw)
        out = out + (wgt * s)[..., None] * value[b, pix, m]
    if attn is not None:
        out = out * attn[..., None]
    return out.sum(2), torch.stack(scores, -1)


def dfa3d_forward_items_ref(value, dist, shapes3, lsi, loc, attn, item_batch, variant=None):
    """Item-list form, any number of levels: loc [n,M,L,P,3], attn [n,M,L,P] | None -> out [n, M*Cm], score [n,M,L,P,4]."""
    n, M, L = loc.shape[:3]
    out, scores = 0, []
    for l in range(L):
        o, s = sample_level(value, dist, tuple(int(v) for v in shapes3[l]), int(lsi[l]), loc[:, :, l],
                            None if attn is None else attn[:, :, l], item_batch, variant)
        out = out + o
        scores.append(s)
    return out.reshape(n, -1), torch.stack(scores, 2)


def dfa3d_forward_ref(value, dist, shapes3, lsi, loc, attn, variant=None):
    """Batch form: loc [B,Q,M,L,P,3] -> out [B,Q,M*Cm], score [B,Q,M,L,P,4]."""
    B, Q = loc.shape[:2]
    bidx = torch.arange(B).repeat_interleave(Q)
    out, score = dfa3d_forward_items_ref(value, dist, shapes3, lsi, loc.flatten(0, 1), None if attn is None else attn.flatten(0, 1),
                                         bidx, variant)
    return out.view(B, Q, -1), score.view(B, Q, *score.shape[1:])


def backward_of(fn, value, dist, loc, attn, go):
    """(out, (grad_value, grad_dist, grad_loc, grad_attn)) of ``out = fn(value, dist, loc, attn)`` by float64 autograd."""
    leaves = [t.detach().double().requires_grad_() for t in (value, dist, loc, attn)]
    out = fn(*leaves)
    return out.detach(), torch.autograd.grad(out, leaves, go.double())


def dfa3d_backward_ref(value, dist, shapes3, lsi, loc, attn, go, item_batch=None, variant=None):
    """Gradients of the batch form (``item_batch`` None) or the item-list form."""
    if item_batch is None:
        fn = lambda v, d, x, a: dfa3d_forward_ref(v, d, shapes3, lsi, x, a, variant)[0]
    else:
        fn = lambda v, d, x, a: dfa3d_forward_items_ref(v, d, shapes3, lsi, x, a, item_batch, variant)[0]
    return backward_of(fn, value, dist, loc, attn, go)


def pairs_deform_gather_ref(value, dist, ref_cam, raw, pair_cam, pair_q, H, W, M, P, variant=None):
    """value [N,S,M,Cm], dist [N,S,D], ref_cam [N,Nq,3], raw [n, M*P*4] -> out [n, M*Cm]:
    loc = ref + off / (W, H, D), attention = softmax of the logits over the P points of a head."""
    value, dist, ref_cam, raw = (t.double() for t in (value, dist, ref_cam, raw))
    n, D = raw.shape[0], dist.shape[-1]
    r = ref_cam[pair_cam.long(), pair_q.long()].view(n, 1, 1, 3)
    uv = raw[:, :M * P * 2].view(n, M, P, 2)
    dz = raw[:, M * P * 2:M * P * 3].view(n, M, P)
    loc = torch.stack([r[..., 0] + uv[..., 0] / W, r[..., 1] + uv[..., 1] / H, r[..., 2] + dz / D], -1)
    attn = raw[:, M * P * 3:].view(n, M, P).softmax(-1)
    out, _ = sample_level(value, dist.view(*dist.shape[:2], 1, D), (H, W, D), 0, loc, attn, pair_cam, variant)
    return out.reshape(n, -1)


def pairs_geometry_sample_ref(feat, dist, ref_cam, pair_cam, pair_q, H, W, variant=None):
    """feat [N,S,C], dist [N,S,D] -> [n, C]: one head, one sample at the reference point, weight 1."""
    feat, dist, ref_cam = (t.double() for t in (feat, dist, ref_cam))
    D = dist.shape[-1]
    loc = ref_cam[pair_cam.long(), pair_q.long()].view(-1, 1, 1, 3)
    out, _ = sample_level(feat.view(*feat.shape[:2], 1, -1), dist.view(*dist.shape[:2], 1, D), (H, W, D), 0, loc, None, pair_cam, variant)
    return out.reshape(loc.shape[0], -1)


def split_reference(c, variant=None):
    """The fused operator's float64 results for ``fused_inputs`` -> dict(out, score [B,Q,M,L,P,4] reference corner order, grads)."""
    d = lambda k: c[k].double()
    out, score = dfa3d_forward_ref(d("value"), d("dist"), c["shapes3"], c["lsi"], d("loc"), d("attn"), variant)
    _, grads = dfa3d_backward_ref(c["value"], c["dist"], c["shapes3"], c["lsi"], c["loc"], c["attn"], c["go"], variant=variant)
    return dict(out=out, score=score, grads=grads)


def split_operators(ops, c, to=lambda t: t):
    """depth_score_forward -> wms_forward and wms_backward -> depth_score_backward of ``ops`` (the HIP library or the C oracle) on
    ``fused_inputs``; ``to`` moves a tensor to the device.  grad_loc is assembled as (gl2.x, gl2.y, gl3.z)."""
    t = {k: to(c[k]) for k in ("value", "dist", "shapes3", "lsi", "loc", "attn", "go")}
    s2, l2 = t["shapes3"][:, :2].contiguous(), t["loc"][..., :2].contiguous()
    score = ops.depth_score_forward(t["dist"], t["shapes3"], t["lsi"], t["loc"])
    out = ops.wms_forward(t["value"], s2, t["lsi"], l2, t["attn"], score)
    gv, gl2, ga, gs = (torch.zeros_like(x) for x in (t["value"], l2, t["attn"], score))
    ops.wms_backward(t["value"], s2, t["lsi"], l2, t["attn"], score, t["go"], gv, gl2, ga, gs)
    gd, gl3 = torch.zeros_like(t["dist"]), torch.zeros_like(t["loc"])
    ops.depth_score_backward(t["dist"], t["shapes3"], t["lsi"], t["loc"], gs, gd, gl3)
    return dict(out=out, score=score, grad_value=gv, grad_dist=gd, grad_loc=torch.cat([gl2, gl3[..., 2:]], -1), grad_attn=ga,
                gl3_uv=gl3[..., :2])


# --------------------------------------------------------------------------------------------------------------------
# comparisons
# --------------------------------------------------------------------------------------------------------------------
def rel_err(a, b):
    """max |a - b| / max(1, max |b|): the figure the `close` helper of tests/test_gpu_kernels.py bounds."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def check(a, b, tol, what, log=None):
    e = rel_err(a, b)
    if log is not None:
        log[what] = max(e, log.get(what, 0.0))
    print(f"{what}: err {e:.3e} of the scale (bound {tol:.0e})")
    assert e <= tol, f"{what}: {e:.3e} of the scale > {tol:.0e}"
    return e


def check_rows(a, b, mag, what, tol=FWD_TOL):
    """Element-wise form of the forward bound.  Every weight of the operator is >= 0, so ``mag`` = the reference run on |value| bounds
    the sum of the magnitudes of an element's terms; an fp32 sum of <= 64 such terms errs by well under 64 * 2^-24 = 4e-6 of it.
    The +-1e3 rows then do not loosen the bound for the elements that never touch them."""
    a, b, mag = a.detach().cpu().double(), b.detach().cpu().double(), mag.detach().cpu().double()
    e = float(((a - b).abs() / mag.clamp(min=1.0)).max())
    print(f"{what}: element-wise err {e:.3e} of max(1, sum |terms|) (bound {tol:.0e})")
    assert e <= tol, f"{what}: element-wise {e:.3e} > {tol:.0e}"
    return e


def check_split(got, ref, what, log=None):
    """``split_operators`` against ``split_reference``: forward and scores at FWD_TOL, the four gradients at BWD_TOL, and the uv
    gradient through the score (which the reference drops) exactly 0."""
    check(got["out"], ref["out"], FWD_TOL, f"{what} forward", log)
    check(got["score"], ref["score"], FWD_TOL, f"{what} score", log)
    for name, want in zip(("grad_value", "grad_dist", "grad_loc", "grad_attn"), ref["grads"]):
        check(got[name], want, BWD_TOL, f"{what} {name}", log)
    assert not got["gl3_uv"].any(), f"{what}: gl3.x / gl3.y must be exactly 0"
