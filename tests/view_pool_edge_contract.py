"""Visibility and softmax edges of the inter-view pooling kernels -- ``view_mean``, ``view_attend``, ``view_attend_pq``,
``view_attend_backward`` -- and the unit-axis / odd-channel edges of ``upsample2x_occ``, shared by the CPU (oracle) and GPU
(HIP library) test modules: every check takes a TensorOps and a device.

The kernels change behaviour on the NUMBER of cameras that see a voxel (rows prefetched ``PD`` at a time, cameras walked in
chunks of ``LG`` = 32 or 64, empty chunks skipped, at most 128 scores parked in LDS), so the visibility mask is built by
design (``patterns``): one voxel per camera count and position that matters, for every N of ``NS``.

References are plain float64 torch on dense ``[N, n_valid, .]`` slots, written here and independent of the oracle.  Bounds:
``1e-5 * max(1, |want|max)`` (forward) and ``2e-5 * max(1, |want|max)`` (gradients) are the project's existing attention
bounds; everything else is an equality, or the derived bound of ``check_exact`` for the projected-query form.

Exact cases use integer-valued data, where every product and sum is exact in fp32:
  * dominant camera: one camera's score exceeds every other by >= 110 (asserted in float64), so in fp32 its softmax weight
    is exactly 1 and the others are exactly 0 (exp(-104) < 2^-149); the score itself is ~ +-90, above the exp overflow at
    88.7, so a kernel that loses the running maximum produces inf / nan.  The result is that camera's row;
  * equal scores: all visible cameras of a voxel share one key row; every weight is 1 / count and the result is the
    correctly rounded mean (a correctly rounded fp32 division equals the float64 quotient rounded to fp32: 53 >= 2 * 24 + 2);
  * one visible camera: ctx = v, grad_v = grad_ctx, grad_q = grad_k = 0."""
import functools
import math

import torch
import torch.nn.functional as F

NS = (1, 3, 31, 32, 33, 64, 65, 100, 128)
COUNTS = (2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65)
KNOBS = ((1, 4), (1, 1), (0, 4))                       # (view_group, view_depth); the first is the default
PQ_DEPTHS = (4, 1, 2, 8)
VARIANTS = ("production", "permuted")

MEAN_GROUP_C = (256, 128)                              # reach view_mean_group_kernel
MEAN_PLAIN_C = (32, 6)                                 # view_mean_kernel<float4>, view_mean_kernel<float>
ATTEND_GROUP = ((256, 8), (128, 8), (256, 1), (256, 2), (256, 16), (128, 4))      # (C, heads): heads * G in {32, 64}
ATTEND_PLAIN = ((64, 8), (32, 8), (16, 8), (8, 8))     # view_attend_kernel<4> (64, 32) and <1> (16, 8)
PQ_C = (256, 128)
BACKWARD = ((256, 8), (128, 8), (64, 8), (32, 8), (16, 8), (8, 8), (256, 1))

UP_GRIDS = ((1, 1, 1), (1, 5, 1), (4, 1, 3), (2, 2, 1))
UP_CHANNELS = (4, 12, 512)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cuda(ops):
    return ops.device_type == "cuda"


def set_knobs(ops, group, depth):
    if _cuda(ops):
        ops.lib.call("sgc_set_tuning", b"view_group", group)
        ops.lib.call("sgc_set_tuning", b"view_depth", depth)


def tuned(ops, group, depth, fn):
    """``fn()`` under the two knobs of view_pool.hip (the oracle has one form of everything), defaults put back afterwards."""
    set_knobs(ops, group, depth)
    try:
        return fn()
    finally:
        set_knobs(ops, 1, 4)


# --------------------------------------------------------------------------------------------------------------------
# visibility patterns
# --------------------------------------------------------------------------------------------------------------------
def patterns(N):
    """name -> bool [N]: the designed visibility columns of an N-camera scene, in a fixed order"""
    cams = torch.arange(N)
    out = {"none": cams < 0, "cam0": cams == 0, "cam_last": cams == N - 1}
    for c in COUNTS:
        if c < N:                                       # c == N is "all"
            out[f"first{c}"] = cams < c
            out[f"last{c}"] = cams >= N - c
    out["alternate"] = cams % 2 == 0
    out["all"] = cams >= 0
    if N > 32:
        out["from32"] = cams >= 32
    if N > 64:
        out["from64"] = cams >= 64
    k = 0
    while sum(bool(v.any()) for v in out.values()) < 5 or sum(bool(v.any()) for v in out.values()) % 2 == 0:
        out[f"all_again{k}"] = cams >= 0                # an odd n_valid (a dead half-wave at C = 128), and > 3 rows for count
        k += 1
    return out


@functools.lru_cache(None)
def scene(N):
    """-> (mask uint8 [N, Nq], names per voxel): the patterns in a seeded order (neighbouring groups of a wave walk different
    counts), unseen voxels at the front, in the middle and at the end, Nq no multiple of 4"""
    pat = patterns(N)
    names = [n for n in pat if n != "none"]
    order = torch.randperm(len(names), generator=_gen(1000 + N)).tolist()
    names = [names[i] for i in order]
    names = ["none"] + names[: len(names) // 2] + ["none"] + names[len(names) // 2:] + ["none"]
    while len(names) % 4 == 0:
        names.append("none")
    mask = torch.stack([pat[n] for n in names], 1).to(torch.uint8).contiguous()
    return mask, tuple(names)


def check_scene(N):
    """the contract's own preconditions: every listed pattern is present for its N, n_valid is odd, Nq % 4 != 0"""
    mask, names = scene(N)
    assert mask.shape == (N, len(names)) and len(names) % 4 != 0 and len(names) <= 84
    cnt = mask.long().sum(0)
    col = {n: i for i, n in enumerate(names)}
    want = {"none": 0, "cam0": 1, "cam_last": 1, "alternate": (N + 1) // 2, "all": N}
    want.update({f"first{c}": c for c in COUNTS if c < N})
    want.update({f"last{c}": c for c in COUNTS if c < N})
    if N > 32:
        want["from32"] = N - 32
    if N > 64:
        want["from64"] = N - 64
    for name, c in want.items():
        assert name in col and int(cnt[col[name]]) == c, (N, name)
    m = mask.bool()
    assert bool(m[0, col["cam0"]]) and bool(m[N - 1, col["cam_last"]])
    for c in COUNTS:
        if c < N:
            assert bool(m[:c, col[f"first{c}"]].all()) and bool(m[N - c:, col[f"last{c}"]].all())
    assert bool(m[::2, col["alternate"]].all())
    if N > 32:
        assert not bool(m[:32, col["from32"]].any()) and bool(m[32:, col["from32"]].all())
    if N > 64:
        assert not bool(m[:64, col["from64"]].any()) and bool(m[64:, col["from64"]].all())
    n_valid = int((cnt > 0).sum())
    assert n_valid % 2 == 1 and n_valid >= 5, (N, n_valid)
    assert int(cnt.sum()) <= 4096
    return n_valid


def pair_list(ops, device, N, variant):
    """the production pair list of ``scene(N)`` (``ops.compact_pairs``), checked against the mask; ``permuted``: the same slot
    table with the pair rows renumbered by a seeded permutation (the header defines slot only as "pair index or -1").
    -> dict(slot, valid_index on the device; slot_c, vi_c, vis [N, n_valid] bool on the CPU; n_pairs, n_valid, N)"""
    mask, _ = scene(N)
    pc = ops.compact_pairs(mask.to(device))
    n_pairs, n_valid = (int(v) for v in pc["totals"][:2].cpu())
    slot = pc["slot"].cpu()
    vi = pc["valid_index"][:n_valid].cpu().contiguous()
    m = mask.bool()
    assert n_pairs == int(m.sum()) and n_valid == int(m.any(0).sum())
    assert torch.equal(slot >= 0, m), "slot >= 0 exactly where the mask is set"
    assert torch.equal(slot[m].sort().values, torch.arange(n_pairs, dtype=torch.int32)), "slot numbers the pairs"
    assert torch.equal(vi.long(), m.any(0).nonzero()[:, 0]), "valid_index: the seen voxels, ascending"
    if variant == "permuted":
        perm = torch.randperm(n_pairs, generator=_gen(2000 + N)).int()
        slot = torch.where(slot >= 0, perm[slot.clamp(min=0).long()], slot).contiguous()
    else:
        assert variant == "production"
    return dict(slot=slot.to(device), valid_index=vi.to(device), slot_c=slot, vi_c=vi, vis=m[:, vi.long()],
                n_pairs=n_pairs, n_valid=n_valid, N=N)


def to_rows(dense, pl):
    """dense [N, n_valid, D] -> pair rows [n_pairs, D]: row slot[n, valid_index[i]] = dense[n, i]"""
    sl = pl["slot_c"].long()[:, pl["vi_c"].long()]
    rows = torch.zeros((pl["n_pairs"], dense.shape[-1]), dtype=dense.dtype)
    rows[sl[pl["vis"]]] = dense[pl["vis"]]
    return rows


def to_dense(rows, pl):
    """pair rows -> (dense [N, n_valid, D] with zeros in the unseen slots, vis [N, n_valid])"""
    sl = pl["slot_c"].long()[:, pl["vi_c"].long()]
    return rows[sl.clamp(min=0)] * pl["vis"][..., None].to(rows.dtype), pl["vis"]


# --------------------------------------------------------------------------------------------------------------------
# float64 references
# --------------------------------------------------------------------------------------------------------------------
def ref_mean(feat, pl):
    d, vis = to_dense(feat.double(), pl)
    return d.sum(0) / vis.sum(0)[:, None]


def ref_attend_scores(q, kv, pl, heads):
    C = q.shape[1]
    hd = C // heads
    d, vis = to_dense(kv, pl)
    N, nv = vis.shape
    k, v = d[..., :C].reshape(N, nv, heads, hd), d[..., C:].reshape(N, nv, heads, hd)
    s = torch.einsum("ihc,nihc->nih", q.reshape(nv, heads, hd), k) * (1.0 / hd) ** 0.5
    return s.masked_fill(~vis[..., None], -math.inf), v


def ref_attend(q, kv, pl, heads):
    """per head softmax(scale q_h . k_n) over the visible cameras, times v (float64 tensors in, autograd passes through)"""
    s, v = ref_attend_scores(q, kv, pl, heads)
    return torch.einsum("nih,nihc->ihc", torch.softmax(s, 0), v).reshape(q.shape)


def ref_attend_backward(q, kv, gctx, pl, heads):
    q, kv = q.double().requires_grad_(), kv.double().requires_grad_()
    ref_attend(q, kv, pl, heads).backward(gctx.double())
    return q.grad, kv.grad


def ref_pq_scores(qp, x, pl):
    d, vis = to_dense(x.double(), pl)
    nv, C = vis.shape[1], x.shape[1]
    s = torch.einsum("ihc,nic->nih", qp.double().reshape(nv, -1, C), d)
    return s.masked_fill(~vis[..., None], -math.inf), d


def ref_pq(qp, x, pl):
    s, d = ref_pq_scores(qp, x, pl)
    return torch.einsum("nih,nic->ihc", torch.softmax(s, 0), d).reshape(qp.shape)


def _gap(s):
    """scores [N, nv, H] with -inf on unseen cameras -> the smallest (best - second best) over voxels with > 1 camera"""
    top = s.topk(min(2, s.shape[0]), 0).values
    if top.shape[0] < 2:
        return math.inf
    g = top[0] - top[1]
    return float(g[torch.isfinite(g)].min()) if bool(torch.isfinite(g).any()) else math.inf


# --------------------------------------------------------------------------------------------------------------------
# running the entry points
# --------------------------------------------------------------------------------------------------------------------
def _count(pl, device):
    return torch.tensor([pl["n_valid"] - 3], dtype=torch.int32, device=device)


def run_mean(ops, device, pl, feat, count=None):
    return ops.view_mean(feat.to(device), pl["slot"], pl["valid_index"], pl["n_valid"], count=count).cpu()


def run_attend(ops, device, pl, q, kv, heads, count=None):
    return ops.view_attend(q.to(device), kv.to(device), pl["slot"], pl["valid_index"], heads, count=count).cpu()


def run_pq(ops, device, pl, qp, x, count=None):
    return ops.view_attend_pq(qp.to(device), x.to(device), pl["slot"], pl["valid_index"], 8, count=count).cpu()


def run_backward(ops, device, pl, q, kv, heads, gctx):
    """the forward's own ctx goes into the backward, as in training"""
    qd, kvd = q.to(device), kv.to(device)
    ctx = ops.view_attend(qd, kvd, pl["slot"], pl["valid_index"], heads)
    gq, gkv = ops.view_attend_backward(qd, kvd, pl["slot"], pl["valid_index"], heads, ctx, gctx.to(device))
    return ctx.cpu(), gq.cpu(), gkv.cpu()


def close(got, want, tol, what):
    assert got.dtype == torch.float32 and got.shape == want.shape, what
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite"
    err = float((got.double() - want.double()).abs().max())
    bound = tol * max(1.0, float(want.abs().max()))
    assert err <= bound, f"{what}: |err|max {err:.3e} > {bound:.3e}"


def _twice_and_count(run, pl, device, what):
    """two launches are bit-identical; with the row count n_valid - 3 on the device the first n_valid - 3 rows are the full
    run's, bit for bit.  -> the result"""
    got, again = run(None), run(None)
    assert torch.equal(got, again), f"{what}: two launches differ"
    part = run(_count(pl, device))
    n = pl["n_valid"] - 3
    assert torch.equal(part[:n], got[:n]), f"{what}: device-side count"
    return got


# --------------------------------------------------------------------------------------------------------------------
# (a) float64 reference on seeded randn data; two launches; device-side count
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _randn_case(op, C, heads, N, n_pairs, n_valid):
    g = _gen(31 * N + C + heads + len(op))
    if op == "mean":
        return (torch.randn(n_pairs, C, generator=g),)
    if op == "pq":
        return torch.randn(n_valid, 8 * C, generator=g) * (2.0 / C ** 0.5), torch.randn(n_pairs, C, generator=g)
    return torch.randn(n_valid, C, generator=g), torch.randn(n_pairs, 2 * C, generator=g), torch.randn(n_valid, C, generator=g)


def check_mean_reference(ops, device, C, N, variant):
    pl = pair_list(ops, device, N, variant)
    feat, = _randn_case("mean", C, 0, N, pl["n_pairs"], pl["n_valid"])
    what = f"view_mean C {C} N {N} {variant}"
    got = _twice_and_count(lambda cnt: run_mean(ops, device, pl, feat, cnt), pl, device, what)
    close(got, ref_mean(feat, pl), 1e-5, what)
    return got


def check_attend_reference(ops, device, C, heads, N, variant):
    pl = pair_list(ops, device, N, variant)
    q, kv, _ = _randn_case("attend", C, heads, N, pl["n_pairs"], pl["n_valid"])
    what = f"view_attend C {C} heads {heads} N {N} {variant}"
    got = _twice_and_count(lambda cnt: run_attend(ops, device, pl, q, kv, heads, cnt), pl, device, what)
    close(got, ref_attend(q.double(), kv.double(), pl, heads), 1e-5, what)
    return got


def check_pq_reference(ops, device, C, N, variant):
    pl = pair_list(ops, device, N, variant)
    qp, x = _randn_case("pq", C, 8, N, pl["n_pairs"], pl["n_valid"])
    what = f"view_attend_pq C {C} N {N} {variant}"
    got = _twice_and_count(lambda cnt: run_pq(ops, device, pl, qp, x, cnt), pl, device, what)
    close(got, ref_pq(qp, x, pl), 1e-5, what)
    return got


def check_backward_reference(ops, device, C, heads, N, variant):
    pl = pair_list(ops, device, N, variant)
    q, kv, gctx = _randn_case("attend", C, heads, N, pl["n_pairs"], pl["n_valid"])
    what = f"view_attend_backward C {C} heads {heads} N {N} {variant}"
    ctx, gq, gkv = run_backward(ops, device, pl, q, kv, heads, gctx)
    ctx2, gq2, gkv2 = run_backward(ops, device, pl, q, kv, heads, gctx)
    assert torch.equal(gq, gq2) and torch.equal(gkv, gkv2), f"{what}: two launches differ"
    want_q, want_kv = ref_attend_backward(q, kv, gctx, pl, heads)
    close(ctx, ref_attend(q.double(), kv.double(), pl, heads), 1e-5, what + " (forward)")
    close(gq, want_q, 2e-5, what + " grad_q")
    close(gkv, want_kv, 2e-5, what + " grad_kv")
    return gq, gkv


# --------------------------------------------------------------------------------------------------------------------
# (c) exact cases on integer-valued data
# --------------------------------------------------------------------------------------------------------------------
def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


PLACEMENTS = ("first", "middle", "last", "chunk32", "chunk64", "per_head") + tuple(f"slot{k}" for k in range(1, 8)) + ("refill",)


@functools.lru_cache(None)
def dominant_cameras(N, heads, placement):
    """-> dom [n_valid, heads]: the camera (index into N) that dominates head h of voxel i.  ``first`` / ``middle`` / ``last``
    among the visible ones; ``slotK``: the K-th visible one (every prefetch slot of PD = 1, 2, 4, 8); ``refill``: the 10th
    (a row loaded by the refill inside the walk); ``chunk32`` / ``chunk64``: the first visible camera of the second chunk of
    LG = 32 / 64 cameras; ``per_head``: another camera for every head.  Where a voxel has too few cameras: its last one."""
    mask = scene(N)[0].bool()
    vis = mask[:, mask.any(0)]
    nv = vis.shape[1]
    dom = torch.zeros((nv, heads), dtype=torch.long)
    for i in range(nv):
        cams = vis[:, i].nonzero()[:, 0].tolist()
        for h in range(heads):
            if placement == "first":
                j = 0
            elif placement == "middle":
                j = len(cams) // 2
            elif placement == "last":
                j = len(cams) - 1
            elif placement == "refill":
                j = 9
            elif placement == "per_head":
                j = (3 * h + 1) % len(cams)
            elif placement.startswith("slot"):
                j = int(placement[4:])
            else:
                lg = int(placement[5:])
                later = [t for t, c in enumerate(cams) if c >= lg]
                j = later[0] if later else len(cams) - 1
            dom[i, h] = cams[min(j, len(cams) - 1)]
    return dom


def _dominant_sign(vis, dom, heads):
    """[N, n_valid, heads]: +1 on the dominant camera of (voxel, head), -1 elsewhere"""
    N = vis.shape[0]
    return torch.where(torch.arange(N)[:, None, None] == dom[None], 1.0, -1.0).double()


def _attend_magnitude(hd):
    m = 1
    while hd ** 0.5 * m * m < 89.0:
        m += 1
    return float(m)                                      # 4 at head_dim 32: q = 4, k = +-4, score = +-90.5


def dominant_attend_case(pl, C, heads, placement):
    """-> q, kv, want: ctx must be the v row of the dominant camera of every (voxel, head), exactly"""
    vis = pl["vis"]
    N, nv = vis.shape
    hd = C // heads
    m = _attend_magnitude(hd)
    dom = dominant_cameras(N, heads, placement)
    sign = _dominant_sign(vis, dom, heads)
    k = (sign[..., None] * m).expand(N, nv, heads, hd).reshape(N, nv, C)
    v = _ints((N, nv, C), -8, 8, _gen(7 * N + C + heads))
    q = torch.full((nv, C), m, dtype=torch.float64)
    kv = to_rows(torch.cat([k, v], 2), pl)
    want = torch.gather(v.reshape(N, nv, heads, hd), 0, dom[None, :, :, None].expand(1, nv, heads, hd))[0].reshape(nv, C)
    s, _ = ref_attend_scores(q, kv, pl, heads)
    assert _gap(s) >= 110.0 and float(s.max()) > 88.8, "the dominant score leads by >= 110 and is above the exp overflow"
    assert torch.equal(ref_attend(q, kv, pl, heads).float(), want.float()), "float64 reference == the dominant camera's v row"
    return q.float(), kv.float().contiguous(), want.float()


def dominant_pq_case(pl, C, placement):
    """projected-query twin: qp_h is non-zero on channel block h only, x_n is positive there when n dominates head h.  -> qp,
    x, want [n_valid, 8 * C]: head h's result is the whole x row of its dominant camera, exactly"""
    vis = pl["vis"]
    N, nv = vis.shape
    H, B = 8, C // 8
    dom = dominant_cameras(N, H, placement)
    sign = _dominant_sign(vis, dom, H)
    mag = _ints((N, nv, H, B), 3, 5, _gen(11 * N + C))
    x = (sign[..., None] * mag).reshape(N, nv, C)
    qp = torch.zeros((nv, H, H, B), dtype=torch.float64)
    for h in range(H):
        qp[:, h, h, :] = 32.0 / B                        # score = (32 / B) * sum of B values in 3 .. 5: 96 .. 160
    qp = qp.reshape(nv, H * C)
    rows = to_rows(x, pl)
    want = torch.gather(x, 0, dom.t()[:, :, None].expand(H, nv, C)).permute(1, 0, 2).reshape(nv, H * C)
    s, _ = ref_pq_scores(qp, rows, pl)
    assert _gap(s) >= 110.0 and float(s.max()) > 88.8
    assert torch.equal(ref_pq(qp, rows, pl).float(), want.float())
    return qp.float(), rows.float().contiguous(), want.float()


def equal_score_case(pl, C, seed):
    """all visible cameras of a voxel share one key row.  -> q, kv, gctx (integer-valued), want = the correctly rounded mean
    of the voxel's v rows"""
    vis = pl["vis"]
    N, nv = vis.shape
    g = _gen(seed)
    k = _ints((1, nv, C), -3, 3, g).expand(N, nv, C)
    v = _ints((N, nv, C), -8, 8, g)
    q = _ints((nv, C), -3, 3, g)
    gctx = _ints((nv, C), -4, 4, g)
    kv = to_rows(torch.cat([k, v], 2), pl)
    want = (v * vis[..., None]).sum(0) / vis.sum(0)[:, None]
    return q.float(), kv.float().contiguous(), gctx.float(), want.float(), v


def check_mean_exact(ops, device, C, N, variant):
    pl = pair_list(ops, device, N, variant)
    d = _ints((N, pl["n_valid"], C), -8, 8, _gen(5 * N + C))
    feat = to_rows(d, pl).float()
    want = ((d * pl["vis"][..., None]).sum(0) / pl["vis"].sum(0)[:, None]).float()
    got = run_mean(ops, device, pl, feat)
    assert torch.equal(got, want), f"view_mean on integers, C {C} N {N} {variant}: {int((got != want).sum())} elements differ"


def check_attend_exact(ops, device, C, heads, N, variant):
    pl = pair_list(ops, device, N, variant)
    for placement in PLACEMENTS:
        q, kv, want = dominant_attend_case(pl, C, heads, placement)
        got = run_attend(ops, device, pl, q, kv, heads)
        assert torch.equal(got, want), \
            f"view_attend, dominant camera {placement}, C {C} heads {heads} N {N} {variant}: rows {(got != want).any(1).nonzero()[:, 0].tolist()}"
    q, kv, _, want, _ = equal_score_case(pl, C, 13 * N + C + heads)
    assert (ref_attend(q.double(), kv.double(), pl, heads) - want.double()).abs().max() < 1e-6      # the fp32 rounding of the mean
    got = run_attend(ops, device, pl, q, kv, heads)
    assert torch.equal(got, want), \
        f"view_attend, equal scores, C {C} heads {heads} N {N} {variant}: rows {(got != want).any(1).nonzero()[:, 0].tolist()}"


def check_pq_exact(ops, device, C, N, variant):
    pl = pair_list(ops, device, N, variant)
    vis = pl["vis"]
    nv = pl["n_valid"]
    for placement in PLACEMENTS:
        qp, x, want = dominant_pq_case(pl, C, placement)
        got = run_pq(ops, device, pl, qp, x)
        assert torch.equal(got, want), \
            f"view_attend_pq, dominant camera {placement}, C {C} N {N} {variant}: rows {(got != want).any(1).nonzero()[:, 0].tolist()}"
    # equal scores: one x row per voxel.  The kernel multiplies by the rounded weight e / sum, so the result is not exact:
    # each weight carries <= 2^-24 relative error, each of the cnt accumulations <= 2^-24 of a partial sum <= max|x|
    g = _gen(17 * N + C)
    xd = _ints((1, nv, C), -8, 8, g).expand(N, nv, C)
    qp = (_ints((nv, 8 * C), -2, 2, g) / 8.0).float()
    x = to_rows(xd, pl).float()
    got = run_pq(ops, device, pl, qp, x)
    want = xd[0][:, None, :].expand(nv, 8, C).reshape(nv, 8 * C)
    assert (ref_pq(qp, x, pl) - want).abs().max() < 1e-12
    bound = (vis.sum(0).double() * 2.0 ** -23 * float(xd.abs().max()))[:, None]
    err = (got.double() - want).abs()
    assert bool((err <= bound).all()), f"view_attend_pq, equal scores, C {C} N {N} {variant}: worst {float((err - bound).max()):.3e} over the bound"
    single = vis.sum(0) == 1
    assert bool(single.any()) and torch.equal(got[single], want[single].float()), "one visible camera: s is its x row"


def check_backward_exact(ops, device, C, heads, N, variant):
    """one visible camera: a = 1 and S = da in the kernel's own arithmetic, so ctx = v, grad_v = grad_ctx, grad_q = grad_k = 0"""
    pl = pair_list(ops, device, N, variant)
    vis = pl["vis"]
    q, kv, gctx, _, v = equal_score_case(pl, C, 19 * N + C + heads)
    ctx, gq, gkv = run_backward(ops, device, pl, q, kv, heads, gctx)
    single = (vis.sum(0) == 1).nonzero()[:, 0]
    assert len(single) >= 2
    sl = pl["slot_c"].long()[:, pl["vi_c"].long()]
    for i in single.tolist():
        n = int(vis[:, i].nonzero()[0, 0])
        p = int(sl[n, i])
        what = f"view_attend_backward, one visible camera, C {C} heads {heads} N {N} {variant}, voxel row {i}"
        assert torch.equal(ctx[i], v[n, i].float()), what + ": ctx != v"
        assert torch.equal(gkv[p, C:], gctx[i]), what + ": grad_v != grad_ctx"
        assert not bool(gkv[p, :C].any()), what + ": grad_k != 0"
        assert not bool(gq[i].any()), what + ": grad_q != 0"
    want_q, want_kv = ref_attend_backward(q, kv, gctx, pl, heads)
    close(gq, want_q, 2e-5, "equal scores grad_q")
    close(gkv, want_kv, 2e-5, "equal scores grad_kv")


def check_unsupported_head_dim(ops, device):
    """C = 24 with 8 heads (head_dim 3): the HIP library has no lane grouping for it and must say so, in the forward and in the
    backward; the oracle has one general form and computes it"""
    N, heads, C = 3, 8, 24
    pl = pair_list(ops, device, N, "production")
    g = _gen(24)
    q, kv, gctx = torch.randn(pl["n_valid"], C, generator=g), torch.randn(pl["n_pairs"], 2 * C, generator=g), torch.randn(pl["n_valid"], C, generator=g)
    if not _cuda(ops):
        close(run_attend(ops, device, pl, q, kv, heads), ref_attend(q.double(), kv.double(), pl, heads), 1e-5, "oracle at head_dim 3")
        return
    raised = 0
    for call in (lambda: run_attend(ops, device, pl, q, kv, heads),
                 lambda: ops.view_attend_backward(q.to(device), kv.to(device), pl["slot"], pl["valid_index"], heads, q.to(device), gctx.to(device))):
        try:
            call()
        except RuntimeError:
            raised += 1
    assert raised == 2, "view_attend / view_attend_backward must raise at head_dim 3"


def check_pq_capacity(ops, device):
    """the LDS score table holds kPqMaxViews = 128 cameras: N = 128 is supported (and ``scene(128)`` has a voxel seen by all
    128), N = 129 is not"""
    mask, names = scene(128)
    assert int(mask[:, names.index("all")].sum()) == 128
    for C in PQ_C:
        assert ops.view_attend_pq_supported(128, C, 8)
        if _cuda(ops):
            assert not ops.view_attend_pq_supported(129, C, 8)
            assert not ops.view_attend_pq_supported(128, C, 4) and not ops.view_attend_pq_supported(128, 64, 8)


# --------------------------------------------------------------------------------------------------------------------
# (b) bit identity across the forms of one entry point (what view_pool.hip and tuning.hpp state)
# --------------------------------------------------------------------------------------------------------------------
def check_mean_forms(ops, device, C, N):
    pl = pair_list(ops, device, N, "production")
    feat, = _randn_case("mean", C, 0, N, pl["n_pairs"], pl["n_valid"])
    res = {kn: tuned(ops, *kn, lambda: run_mean(ops, device, pl, feat)) for kn in KNOBS}
    for kn in KNOBS[:2]:
        assert torch.equal(res[kn], res[(0, 4)]), f"view_mean C {C} N {N}: view_group/view_depth {kn} differs from the per-camera loop"


def check_attend_forms(ops, device, C, heads, N):
    pl = pair_list(ops, device, N, "production")
    q, kv, _ = _randn_case("attend", C, heads, N, pl["n_pairs"], pl["n_valid"])
    res = {kn: tuned(ops, *kn, lambda: run_attend(ops, device, pl, q, kv, heads)) for kn in KNOBS}
    for kn in KNOBS[:2]:
        assert torch.equal(res[kn], res[(0, 4)]), \
            f"view_attend C {C} heads {heads} N {N}: view_group/view_depth {kn} differs from the per-camera loop"


def check_pq_forms(ops, device, C, N):
    pl = pair_list(ops, device, N, "production")
    qp, x = _randn_case("pq", C, 8, N, pl["n_pairs"], pl["n_valid"])
    res = {d: tuned(ops, 1, d, lambda: run_pq(ops, device, pl, qp, x)) for d in PQ_DEPTHS}
    for d in PQ_DEPTHS[1:]:
        assert torch.equal(res[d], res[4]), f"view_attend_pq C {C} N {N}: view_depth {d} differs from 4"


# --------------------------------------------------------------------------------------------------------------------
# upsample2x_occ on unit axes and odd channel counts
# --------------------------------------------------------------------------------------------------------------------
def _interp(vol, grid):
    C = vol.shape[1]
    x = vol.double().view(*grid, C).permute(3, 0, 1, 2)[None]
    return F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=False)[0].permute(1, 2, 3, 0).reshape(-1, C)


def check_upsample(ops, device, C, grid):
    g = _gen(C + 100 * grid[0] + 10 * grid[1] + grid[2])
    V = grid[0] * grid[1] * grid[2]
    vol = torch.randn(V, C, generator=g)
    w, b = torch.randn(C, generator=g) * 0.1, torch.randn(1, generator=g)
    up, occ, og = ops.upsample2x_occ(vol.to(device), grid, w.to(device), b.to(device))
    assert og == tuple(2 * d for d in grid) and up.shape == (8 * V, C) and occ.shape == (8 * V,)
    want = _interp(vol, grid)
    close(up.cpu(), want, 1e-6, f"upsample2x_occ up C {C} grid {grid}")
    close(occ.cpu(), torch.sigmoid(want @ w.double() + b.double()), 2e-6, f"upsample2x_occ occ C {C} grid {grid}")
    up_only, none, _ = ops.upsample2x_occ(vol.to(device), grid)
    assert none is None and torch.equal(up_only, up)
    # integer inputs: every weight is a multiple of 1 / 4 (0 or 1 along a unit axis), every product and sum is exact
    vol_i = _ints((V, C), -8, 8, g).float()
    up_i, _, _ = ops.upsample2x_occ(vol_i.to(device), grid)
    assert torch.equal(up_i.cpu(), _interp(vol_i, grid).float()), f"upsample2x_occ on integers, C {C} grid {grid}"
