"""The buffer cases (tests/buffer_contract.py) of include/sgcdet_amd_level_train.h -- the LayerNorm backward, the sampling locations
forward / backward, the view-mean backward -- and the float64 torch formulations they and tests/test_gpu_level_train.py compare
with: autograd of what the default training path of a level computes today (``F.layer_norm``; the ``view`` / ``softmax`` / ``cat`` /
``div`` / ``add`` chain of ``_forward_pairs_train``; ``index_add`` + ``div``).  tests/test_level_train_cpu.py holds this table to the
coverage rule; tests/test_gpu_buffers_level_train.py runs it on the GPU.

The unread padding columns of ``proj`` carry NaN: the header says they are never read."""
import torch
import torch.nn.functional as F

from buffer_contract import Case

CASES = []
EPS = 1e-5


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
def ln_inputs(rows, C, seed, special=False):
    """x, dy [rows, C], gamma, beta [C].  ``special`` (rows >= 3): row 0 constant, row 1 zeros, row 2 with mean 10 and spread 3."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 1.5 + 0.3
    if special:
        x[0] = 0.75
        x[1] = 0.0
        x[2] = 10.0 + 3.0 * torch.randn(C, generator=g)
    return dict(x=x, dy=torch.randn(rows, C, generator=g), gamma=0.5 + torch.rand(C, generator=g), beta=0.3 * torch.randn(C, generator=g))


def ln_reference(i, dtype=torch.float64):
    """(y, dx, dgamma, dbeta) by autograd of F.layer_norm in ``dtype`` on the CPU."""
    x = i["x"].detach().cpu().to(dtype).requires_grad_(True)
    gamma, beta = (i[k].detach().cpu().to(dtype).requires_grad_(True) for k in ("gamma", "beta"))
    y = F.layer_norm(x, (x.shape[1],), gamma, beta, EPS)
    dx, dgamma, dbeta = torch.autograd.grad(y, (x, gamma, beta), i["dy"].detach().cpu().to(dtype))
    return dict(y=y.detach(), dx=dx, dgamma=dgamma, dbeta=dbeta)


def _ln_case(rows, C):
    def ref(i):
        r = ln_reference(i)
        r.pop("y")
        return r
    # 1e-5 of max(1, max |ref|), the bound of the suite's other fp32 row kernels: at most 77 rows, every sum a chain of at most
    # 77 / 4 + 20 fp32 adds of terms of order one (the bounds derived from torch's own fp32 error are in tests/test_gpu_level_train.py)
    return Case(f"layer_norm_rows_backward-{rows}x{C}", ("sgc_layer_norm_rows_backward",), lambda: ln_inputs(rows, C, 11),
                lambda ops, t: dict(zip(("dx", "dgamma", "dbeta"), ops.layer_norm_rows_backward(t["x"], t["gamma"], t["dy"], EPS))),
                ref=ref, tol=1e-5, only="cuda")


CASES += [_ln_case(5, 96), _ln_case(77, 128), _ln_case(9, 256)]


# ---- sampling locations -----------------------------------------------------------------------------------------------------------
def sampling_inputs(n, M, L, P, ldp, seed, pad_value=float("nan"), edge_logits=False):
    """ref [n, 3], proj [n, ldp] (NaN behind 4 M L P), normalizer [L, 3] with different (W, H, D) per level, grad_loc, grad_attn.
    ``edge_logits``: the first (pair, head) items get logits with equal values, a spread of +-80 and a -inf among finite ones."""
    g = torch.Generator().manual_seed(seed)
    LP, K = L * P, 4 * M * L * P
    proj = torch.cat([2.0 * torch.randn(n, K, generator=g), torch.full((n, ldp - K), pad_value)], 1).contiguous()
    if edge_logits:
        rows = [[80.0, 80.0, -80.0, float("-inf")], [0.25] * 4, [80.0, -80.0, 1.0, -1.0], [0.5, float("-inf"), -0.5, 2.0]]
        logits = proj[:, 3 * M * LP:K].unflatten(1, (M, LP))      # a view: [n, M, LP]
        assert LP == 4
        for k, r in enumerate(rows[:n * M]):
            logits[k // M, k % M] = torch.tensor(r)
    normalizer = torch.tensor([[40.0 - 7 * l, 30.0 - 5 * l, 12.0 + 4 * l] for l in range(L)])
    return dict(ref=torch.rand(n, 3, generator=g), proj=proj, normalizer=normalizer, grad_loc=torch.randn(n, M, L, P, 3, generator=g),
                grad_attn=torch.randn(n, M, L, P, generator=g), M=M, L=L, P=P)


def sampling_reference(i, dtype=torch.float64):
    """(loc, attn, grad_proj) by autograd of the chain of ``DeformCrossAttention_DFA3D._forward_pairs_train`` in ``dtype`` on the CPU;
    grad_proj [n, ldp] with zeros behind the 4 M L P columns the chain reads."""
    M, L, P = i["M"], i["L"], i["P"]
    K = 4 * M * L * P
    n, ldp = i["proj"].shape
    proj = i["proj"].detach().cpu()[:, :K].to(dtype).requires_grad_(True)
    ref, normalizer = i["ref"].detach().cpu().to(dtype), i["normalizer"].detach().cpu().to(dtype)
    off_uv = proj[:, :2 * M * L * P].view(n, M, L, P, 2)
    off_d = proj[:, 2 * M * L * P:3 * M * L * P].view(n, M, L, P, 1)
    attn = proj[:, 3 * M * L * P:].view(n, M, L * P).softmax(-1).view(n, M, L, P)
    loc = ref.view(n, 1, 1, 1, 3) + torch.cat([off_uv, off_d], -1) / normalizer[None, None, :, None, :]
    gp, = torch.autograd.grad((loc, attn), proj, (i["grad_loc"].detach().cpu().to(dtype), i["grad_attn"].detach().cpu().to(dtype)))
    return dict(loc=loc.detach(), attn=attn.detach(), grad_proj=F.pad(gp, (0, ldp - K)))


def sampling_run(ops, t):
    loc, attn = ops.sampling_locations_forward(t["ref"], t["proj"], t["normalizer"], t["M"], t["L"], t["P"])
    gp = ops.sampling_locations_backward(attn, t["grad_loc"], t["grad_attn"], t["normalizer"], t["proj"].shape[1])
    return dict(loc=loc, attn=attn, grad_proj=gp)


def _sampling_case(n, M, L, P, ldp):
    # 1e-5 of max(1, max |ref|): one division and one add per location, a softmax over at most 16 values of |logit| <= 10
    return Case(f"sampling_locations-{n}x{M}x{L}x{P}-ldp{ldp}", ("sgc_sampling_locations_forward", "sgc_sampling_locations_backward"),
                lambda: sampling_inputs(n, M, L, P, ldp, 13), sampling_run, ref=sampling_reference, tol=1e-5, only="cuda")


# the float4 form (rows of 128 columns, two levels, padding columns) and the scalar form (L P = 3; L P = 4 on a pitch that is no multiple of 4)
CASES += [_sampling_case(65, 8, 1, 4, 128), _sampling_case(9, 4, 2, 2, 64), _sampling_case(7, 1, 1, 4, 32), _sampling_case(9, 2, 1, 3, 24),
          _sampling_case(5, 2, 1, 4, 35)]


# ---- mean over views ---------------------------------------------------------------------------------------------------------------
def pair_list(mask):
    """mask [N, Nq] bool -> (slot [N, Nq] int32: camera-major pair index or -1, valid_index [n_valid] int32, n_pairs): what
    ``sgc_compact_pairs`` produces."""
    flat = mask.reshape(-1)
    slot = torch.full((flat.numel(),), -1, dtype=torch.int32)
    slot[flat] = torch.arange(int(flat.sum()), dtype=torch.int32)
    return slot.view(mask.shape).contiguous(), mask.any(0).nonzero()[:, 0].to(torch.int32).contiguous(), int(flat.sum())


def view_mask(N, Nq, seed):
    """Voxels seen by no camera (every fifth), by exactly one (every fifth, offset 1), by all (offset 2), the rest at random."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(N, Nq, generator=g) < 0.5
    v = torch.arange(Nq)
    mask[:, v % 5 == 0] = False
    mask[:, v % 5 == 1] = False
    mask[(v[v % 5 == 1] // 5) % N, v[v % 5 == 1]] = True
    mask[:, v % 5 == 2] = True
    return mask


def view_mean_inputs(N, Nq, C, seed):
    slot, valid_index, n_pairs = pair_list(view_mask(N, Nq, seed))
    g = torch.Generator().manual_seed(seed + 1)
    return dict(grad_mean=torch.randn(valid_index.numel(), C, generator=g), feat=torch.randn(n_pairs, C, generator=g), slot=slot,
                valid_index=valid_index, n_pairs=n_pairs)


def view_mean_reference(i, dtype=torch.float64):
    """(mean, grad_feat) by autograd of ``index_add`` + ``div``, the default training path's formulation."""
    slot, vi = i["slot"].cpu().long(), i["valid_index"].cpu().long()
    N, Nq = slot.shape
    row_of = torch.full((Nq,), -1, dtype=torch.long)
    row_of[vi] = torch.arange(vi.numel())
    cam_q = (slot >= 0).nonzero()                                  # camera-major, as the pairs are numbered
    q = torch.empty(i["n_pairs"], dtype=torch.long)
    q[slot[cam_q[:, 0], cam_q[:, 1]]] = cam_q[:, 1]
    count = (slot >= 0).sum(0).to(dtype)
    feat = i["feat"].detach().cpu().to(dtype).requires_grad_(True)
    mean = torch.zeros((vi.numel(), feat.shape[1]), dtype=dtype).index_add(0, row_of[q], feat) / count[vi][:, None]
    gf, = torch.autograd.grad(mean, feat, i["grad_mean"].detach().cpu().to(dtype))
    return dict(mean=mean.detach(), grad_feat=gf)


def _view_mean_case(N, Nq, C):
    # one division of an input element: half an ulp, 6e-8 relative
    return Case(f"view_mean_backward-{N}x{Nq}x{C}", ("sgc_view_mean_backward",), lambda: view_mean_inputs(N, Nq, C, 17),
                lambda ops, t: dict(grad_feat=ops.view_mean_backward(t["grad_mean"], t["slot"], t["valid_index"], t["n_pairs"])),
                ref=lambda i: dict(grad_feat=view_mean_reference(i)["grad_feat"]), tol=1e-7, only="cuda")


CASES += [_view_mean_case(3, 70, 32), _view_mean_case(3, 70, 6)]
