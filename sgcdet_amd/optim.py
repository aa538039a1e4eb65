"""The parameter update of a training step on the MI355X: global-norm gradient clipping + AdamW in three HIP launches.

The reference takes this step from Lightning and torch: ``gradient_clip_val=35`` (main.py:71-72), ``torch.optim.AdamW`` over two
parameter groups -- names containing ``backbone`` at 0.1 x lr, everything else at lr (LightningTools/pl_model.py:92-118) -- and
``OneCycleLR`` with one ``max_lr`` per group (pl_model.py:120-136).  ``FusedAdamW`` is that update for a model trained with this
library on its own; ``reference_param_groups`` / ``build_optimizer`` rebuild the reference's set-up from its config dicts.

    optimizer, scheduler = build_optimizer(model, cfg["optimizer"], cfg["lr_scheduler"])      # max_grad_norm = 35
    losses = model.forward_train_from_features(...)
    sum(losses.values()).backward()
    optimizer.step(); scheduler.step(); optimizer.zero_grad()

``step()`` issues at most three kernels (``sgc_grad_sqnorm_batch``: two, ``sgc_adamw_step_batch``: one) and one asynchronous copy
of the item list; it never waits for the device.  There is no CPU path.
"""
import math

import torch

from . import ext

__all__ = ["FusedAdamW", "reference_param_groups", "build_optimizer"]

_N_STAGING = 4


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (``amsgrad=False, maximize=False``, fp32) preceded by ``torch.nn.utils.clip_grad_norm_(params,
    max_grad_norm)`` over ALL parameters of the optimiser, as two multi-tensor HIP kernels (csrc/optim.hip).

    * ``param_groups``, ``add_param_group``, ``zero_grad``, lr schedulers and checkpointing are ``torch.optim.Optimizer``'s.  The
      state of a parameter lives under torch's keys (``step``: fp32 scalar on the CPU, ``exp_avg``, ``exp_avg_sq``) and the groups
      carry torch's AdamW keys, so ``state_dict()`` loads into ``torch.optim.AdamW`` and the reverse.
    * ``max_grad_norm=None``: no clipping and no norm kernel (one launch per step); otherwise ``last_grad_norm`` is the
      1-element device tensor of the norm BEFORE clipping, valid (on the step's stream) after ``step()``.
    * The gradients are read, not written: torch's clip scales ``p.grad`` in place, here the scaled value exists only in
      registers.  Code that reads ``p.grad`` after ``step()`` sees the unclipped gradient.
    * A parameter whose ``grad`` is None is skipped and its ``step`` does not advance (torch's behaviour; the reference trains
      with ``find_unused_parameters=True``).
    * ``step()`` bumps the version counter of every parameter it updates: ``TrainWeightPlanes.get`` and the scene-graph cache key
      on it (a raw-pointer kernel does not move it by itself).
    * Parameters must be dense fp32 tensors: another dtype is a ``TypeError`` naming the parameter, at construction.  The
      optimiser (and a scheduler on it) can be built while the model is still on the CPU, but ``step()`` needs every
      parameter on one CUDA device and raises ``RuntimeError`` otherwise: the product has no CPU fallback.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, block_elems=None):
        if isinstance(lr, torch.Tensor):
            raise TypeError("FusedAdamW: lr must be a Python number (hyper-parameters travel as kernel arguments)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (None switches clipping off)")
        # torch.optim.AdamW's group keys, so that a state_dict moves between the two unchanged
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.block_elems = block_elems
        self.last_grad_norm = None
        self.item_uploads = 0            # item lists copied to the device so far (tests, tools)
        self._device = None
        self._dev_items = None           # uint8 device buffer holding the current item list
        self._dev_blob = None            # the bytes it holds
        self._staging = []               # pinned host buffers, rotated: [tensor, event of the last copy out of it]
        self._turn = 0
        self._partials = None
        self._norm = None
        super().__init__(params, defaults)

    # ---- parameter checks ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _name(group, gi, i):
        names = group.get("param_names")
        return names[i] if names else f"param_groups[{gi}]['params'][{i}]"

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        gi = len(self.param_groups) - 1
        group = self.param_groups[gi]
        if len(self.param_groups) > 8:
            raise ValueError("FusedAdamW: at most 8 parameter groups (they are passed to the kernel by value)")
        for i, p in enumerate(group["params"]):
            name = self._name(group, gi, i)
            if p.dtype != torch.float32:
                raise TypeError(f"FusedAdamW: parameter {name} is {p.dtype}; only float32 parameters, gradients and state are supported")
            if p.layout != torch.strided or not p.is_contiguous():
                raise TypeError(f"FusedAdamW: parameter {name} is not a dense contiguous tensor")

    # ---- the step -------------------------------------------------------------------------------------------------------------
    def _entries(self):
        """(entries of TensorOps.optim_item_list, hyper-parameters per group, parameters) of this step; advances ``step``."""
        entries, hyper, updated = [], [], []
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("FusedAdamW: amsgrad / maximize are not implemented")
            if not group.get("decoupled_weight_decay", True):
                raise NotImplementedError("FusedAdamW: decoupled_weight_decay=False is Adam, not AdamW")
            lr, (beta1, beta2) = group["lr"], group["betas"]
            if isinstance(lr, torch.Tensor):
                raise TypeError("FusedAdamW: a tensor lr would need a host read-back every step; use a Python number")
            hyper.append((lr, group["weight_decay"], beta1, beta2, group["eps"]))
            for i, p in enumerate(group["params"]):
                if p.device != self._device:
                    if p.device.type != "cuda":
                        raise RuntimeError(f"FusedAdamW: parameter {self._name(group, gi, i)} is on {p.device}; the gfx950 library "
                                           "has no CPU fallback")
                    if self._device is not None:
                        raise RuntimeError(f"FusedAdamW: parameter {self._name(group, gi, i)} is on {p.device}, others on {self._device}")
                    self._device = p.device
                g = p.grad
                if g is None:
                    continue
                if g.dtype != torch.float32 or g.layout != torch.strided or g.device != p.device:
                    raise TypeError(f"FusedAdamW: the gradient of {self._name(group, gi, i)} is {g.dtype} / {g.layout} on {g.device}; "
                                    "only dense float32 gradients on the parameter's device are supported")
                if not g.is_contiguous():
                    raise TypeError(f"FusedAdamW: the gradient of {self._name(group, gi, i)} is not contiguous")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                if m.dtype != torch.float32 or v.dtype != torch.float32 or m.device != p.device or v.device != p.device \
                        or not m.is_contiguous() or not v.is_contiguous():
                    raise TypeError(f"FusedAdamW: the state of {self._name(group, gi, i)} must be contiguous float32 on {p.device}")
                step_t = state["step"]
                if step_t.is_cuda:
                    raise TypeError(f"FusedAdamW: state['step'] of {self._name(group, gi, i)} is on the device (a capturable / fused "
                                    "torch checkpoint loaded without moving it): reading it would synchronise every step")
                step_t += 1
                step = int(step_t)
                # as torch: Python floats (double), rounded to fp32 where they meet the tensors
                entries.append((p, g, m, v, gi, step, 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)))
                updated.append(p)
        return entries, hyper, updated

    def _upload(self, blob):
        """The item list on the device: copied only when it differs from what is there, asynchronously, out of a pinned buffer
        that is not written again before the copy has run (four buffers in rotation, each guarded by an event)."""
        if blob == self._dev_blob:
            return
        cap = 1 << max(12, (len(blob) - 1).bit_length())
        if self._dev_items is None or self._dev_items.numel() < cap:
            self._dev_items = torch.empty(cap, dtype=torch.uint8, device=self._device)
            self._staging = []
        if not self._staging:
            self._staging = [[torch.empty(cap, dtype=torch.uint8, pin_memory=True), None] for _ in range(_N_STAGING)]
        slot = self._staging[self._turn % _N_STAGING]
        self._turn += 1
        if slot[1] is not None and not slot[1].query():      # the host is four steps ahead of the device: wait for that copy
            slot[1].synchronize()
        slot[0][:len(blob)] = torch.frombuffer(blob, dtype=torch.uint8)
        self._dev_items[:len(blob)].copy_(slot[0][:len(blob)], non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()
        self._dev_blob = blob
        self.item_uploads += 1

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries, hyper, updated = self._entries()
        if not entries:
            return loss
        ops = ext.ops()
        with torch.cuda.device(self._device):
            blob, n_items, total_blocks = ops.optim_item_list(entries, self.block_elems)
            if n_items == 0:
                return loss
            self._upload(bytearray(blob))
            norm = None
            if self.max_grad_norm is not None:
                need = ops.grad_sqnorm_workspace_floats(total_blocks)
                if self._partials is None or self._partials.numel() < need:
                    self._partials = torch.empty(max(need, 4096), dtype=torch.float32, device=self._device)
                if self._norm is None:
                    self._norm = torch.empty(1, dtype=torch.float32, device=self._device)
                norm = ops.grad_sqnorm_batch(self._dev_items, n_items, total_blocks, self._partials, self._norm)
                self.last_grad_norm = norm
            ops.adamw_step_batch(self._dev_items, n_items, total_blocks, hyper, norm,
                                 self.max_grad_norm if norm is not None else 0.0)
        # the kernels wrote through raw pointers: move the version counters as an in-place torch op would have
        torch._C._increment_version(updated)
        return loss


def reference_param_groups(model, lr, weight_decay):
    """The two parameter groups of the reference (LightningTools/pl_model.py:100-109): trainable parameters whose name contains
    ``backbone`` at 0.1 x lr, all others at lr, the same weight decay for both.  An empty group is dropped (a detector built
    from precomputed feature maps has no backbone)."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [
        dict(params=[p for n, p in named if "backbone" in n], lr=lr * 0.1, weight_decay=weight_decay * 1.0, name="backbone"),
        dict(params=[p for n, p in named if "backbone" not in n], lr=lr, weight_decay=weight_decay, name="others"),
    ]
    return [g for g in groups if g["params"]]


def build_optimizer(model, optimizer_cfg, lr_scheduler_cfg, max_grad_norm=35.0):
    """``(optimizer, scheduler)`` from the ``optimizer`` / ``lr_scheduler`` dicts of the reference's configs as they stand
    (configs/SGCDet_ScanNet.py:209-225), built as LightningTools/pl_model.py:92-136 builds them: ``FusedAdamW`` over
    ``reference_param_groups`` with the global-norm clip of main.py:71-72 folded in, and torch's own ``OneCycleLR`` with
    ``max_lr = [0.1 x max_lr, max_lr]`` for the groups that exist.  ``interval`` / ``frequency`` are Lightning's (step the
    scheduler once per optimiser step) and are ignored."""
    if optimizer_cfg["type"] != "AdamW":
        raise NotImplementedError(f"optimizer type {optimizer_cfg['type']!r}")
    groups = reference_param_groups(model, optimizer_cfg["lr"], optimizer_cfg["weight_decay"])
    if not groups:
        raise ValueError("build_optimizer: the model has no trainable parameter")
    optimizer = FusedAdamW(groups, max_grad_norm=max_grad_norm)
    if lr_scheduler_cfg["type"] != "OneCycleLR":
        raise NotImplementedError(f"lr_scheduler type {lr_scheduler_cfg['type']!r}")
    max_lr = {"backbone": lr_scheduler_cfg["max_lr"] * 0.1, "others": lr_scheduler_cfg["max_lr"]}
    scheduler = torch.optim.lr_scheduler.OneCycleLR(
        optimizer,
        max_lr=[max_lr[g["name"]] for g in groups],
        total_steps=lr_scheduler_cfg["total_steps"],
        pct_start=lr_scheduler_cfg["pct_start"],
        cycle_momentum=lr_scheduler_cfg["cycle_momentum"],
        anneal_strategy=lr_scheduler_cfg["anneal_strategy"],
        final_div_factor=lr_scheduler_cfg["final_div_factor"],
    )
    return optimizer, scheduler
