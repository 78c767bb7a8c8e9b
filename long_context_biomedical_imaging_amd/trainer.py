"""Training step — the hot-path driver of /root/reference/trainer/trainer_base.py (:94-189).

One process per GPU (torchrun), torch.distributed over RCCL (backend "nccl" on ROCm). The model is wrapped
in DDP exactly as the reference does (trainer_base.py:98); its bucketed fp32 gradient all-reduce runs on
RCCL over xGMI, overlapped with backward. Per step (trainer_base.py:157-182): forward under autocast,
loss, backward, optimizer step, zero_grad, and the LR scheduler's step (OneCycleLR per update :181-182, StepLR /
ReduceLROnPlateau per epoch :211-219 -> TrainStep.end_epoch).

Documented deviations from the reference step:
  * autocast dtype is bf16 on gfx950 (the reference's utils/status.py:50-58 `support_bfloat16` checks for
    "A100"/"H100" in the device name and would pick fp16 here); with bf16 no GradScaler is needed;
  * DDP broadcast_buffers=False: the only buffers are constant index tables (relative_position_index,
    Hyena pos-emb t/deltas), so the per-forward broadcast the reference pays moves nothing that changes;
  * a batch of 1 is duplicated as the reference does (trainer_base.py:160-164) when the model holds a BatchNorm
    (the UperNet heads: a PSP bin-1 map has one value per channel and sample, which BatchNorm cannot train on).
    Without one the duplicate changes nothing — a mean loss over two identical samples has the loss and the
    gradients of one — so it is skipped there (the 3-D ViTUNETR / SwinUNETR benches at one volume per GPU
    would otherwise do twice the work for the same update).
"""
from __future__ import annotations

import argparse
import math
import os
import weakref

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F
from torch.optim.adam import _fused_adam


def init_distributed():
    """Returns (rank, local_rank, world_size); initialises the process group when launched by torchrun."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        # LCI_DIST_BACKEND=gloo: rehearse N ranks on fewer GPUs (gloo moves CUDA tensors through the host)
        backend = os.environ.get("LCI_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend)
    return rank, local, world


TUNED_GEMMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop_gfx950.csv")


def use_tuned_gemms(path: str = TUNED_GEMMS) -> bool:
    """Route torch's Linear / matmul GEMMs through PyTorch-ROCm TunableOp with the solutions recorded for this
    package's shapes on MI355X (hipBLASLt / rocBLAS solution ids, written by a tuning run of bench.py with
    PYTORCH_TUNABLEOP_ENABLED=1; e.g. the ViT-small qkv projection at L = 65536: 0.58 -> 0.15 ms). Tuning itself
    stays off (it costs ~2 min per workload on first use); shapes absent from the file keep the default
    heuristics, and a file recorded under another PyTorch / ROCm / hipBLASLt / arch is rejected by TunableOp's
    validators. LCI_TUNED_GEMMS=0 disables. Returns whether the table is active."""
    if os.environ.get("LCI_TUNED_GEMMS", "1") == "0" or not os.path.exists(path) or not torch.cuda.is_available():
        return False
    import torch.cuda.tunable as tunable
    tunable.enable(True)
    tunable.tuning_enable(False)
    # anything TunableOp writes at exit goes to the temp dir, never over the shipped table
    import tempfile
    tunable.set_filename(os.path.join(tempfile.gettempdir(), f"lci_tunableop_{os.getpid()}.csv"))
    return bool(tunable.read_file(path))


class _LciAdamStep:
    """Adam / AdamW whose update runs on csrc/optim.hip (kernels.adam_step). A subclass of torch's optimizer built
    with fused=True, so its state (per-parameter device `step`, `exp_avg`, `exp_avg_sq`), param_groups and
    state_dict are torch's own and checkpoints move between the two; only the arithmetic kernel differs (the same
    formulas: csrc/optim.hip). torch's fused kernel gave each 64-K-element chunk one workgroup (~1000 over a
    SwinUNETR step at ~1 TB/s); this one streams at the HBM rate. Groups with options the reference never sets
    (amsgrad, complex or non-f32 parameters, differentiable) take torch's fused update.

    LR schedules reach the kernel through device memory, so a captured step follows them: a tensor `group["lr"]` of
    one CUDA f32 element (torch's convention for capturable optimizers; StepLR / ReduceLROnPlateau fill_ it) is read
    by the kernel, and a registered LciOneCycleLR is evaluated there from each tensor's step count (learning rate and
    beta1; param_groups' "lr" / "betas" are then only the host mirror its step() keeps). `_lci_grad_coef`, set by
    TrainStep around a clipped update, multiplies every gradient in the kernel.

    torch's fused Adam declares `_step_supports_amp_scaling`, so a GradScaler (the reference's loop,
    trainer_base.py:116,171-182) does not unscale / inf-check for it but hands the optimizer `grad_scale` and
    `found_inf`; while either is set the step runs torch's fused kernel with them (gradients unscaled in the kernel,
    the update skipped on a device-side inf / NaN), exactly what the class it derives from does."""

    _decoupled = False
    _lci_sched = None       # weakref to the LciOneCycleLR whose schedule the kernel evaluates (set by its constructor)
    _lci_grad_coef = None   # one f32 CUDA element every gradient is multiplied by in the next step (TrainStep's clip)

    def onecycle_constants(self, group):
        """The one-cycle constants of `group` for kernels.adam_step(sched=...), read from the registered scheduler and
        the keys it keeps in the group (so a loaded state_dict of either is followed); None without a scheduler."""
        sched = self._lci_sched() if self._lci_sched is not None else None
        if sched is None:
            return None
        return (sched.total_steps, sched._schedule_phases[0]["end_step"], group["initial_lr"], group["max_lr"],
                group["min_lr"], group["base_momentum"], group["max_momentum"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        scaled = grad_scale is not None or found_inf is not None
        coef = self._lci_grad_coef
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps = [], [], [], [], [], []
            has_complex = self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps)
            if not params:
                continue
            beta1, beta2 = group["betas"]
            lr, sched = group["lr"], self.onecycle_constants(group)
            # a device learning rate (torch's convention for capturable optimizers: StepLR / ReduceLROnPlateau fill_
            # it) is read by the kernel; the one-cycle schedule, evaluated there, takes precedence over either form
            lr_tensor = lr if isinstance(lr, torch.Tensor) and sched is None else None
            bad_lr = lr_tensor is not None and not (lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1)
            if (scaled or has_complex or group["amsgrad"] or group.get("differentiable") or bad_lr
                    or any(p.dtype != torch.float32 or not p.is_cuda for p in params)
                    or any(g.is_sparse or not g.is_contiguous() for g in grads)):
                if sched is not None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                    # torch's kernel would take the host mirror's lr / betas: constants of the graph from then on
                    raise ValueError("LciAdam: a group that takes torch's fused update (amsgrad, non-f32 parameters, "
                                     "a GradScaler, ...) cannot follow OneCycleLR inside a captured step")
                if coef is not None:
                    torch._foreach_mul_(grads, coef)
                _fused_adam(params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps, grad_scale, found_inf,
                                             amsgrad=group["amsgrad"], has_complex=has_complex, beta1=beta1,
                                             beta2=beta2, lr=group["lr"], weight_decay=group["weight_decay"],
                                             eps=group["eps"], maximize=group["maximize"], capturable=True,
                                             differentiable=False, decoupled_weight_decay=self._decoupled)
                continue
            torch._foreach_add_(steps, 1)
            from . import kernels
            kernels.adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2,
                              group["weight_decay"], group["eps"], self._decoupled, group["maximize"],
                              lr_tensor=lr_tensor, sched=sched, grad_coef=coef)
        return loss


class LciAdam(_LciAdamStep, torch.optim.Adam):
    def __init__(self, params, **kw):
        torch.optim.Adam.__init__(self, params, fused=True, **kw)


class LciAdamW(_LciAdamStep, torch.optim.AdamW):
    _decoupled = True

    def __init__(self, params, **kw):
        torch.optim.AdamW.__init__(self, params, fused=True, **kw)


class LciOneCycleLR(torch.optim.lr_scheduler.OneCycleLR):
    """torch's OneCycleLR (the recipes' --scheduler_type, optim_base.py:113-115) whose schedule an LciAdam / LciAdamW
    evaluates inside its update kernel, from each tensor's device step count (csrc/optim.hip: learning rate and, as
    cycle_momentum is on by default, beta1). The optimizer's step therefore follows the schedule inside a captured
    graph too, where the host values `step()` writes would be baked in at capture.

    Everything on the host is torch's: the constructor's arguments and errors, `step()` (which keeps the host mirror:
    param_groups' "lr" and "betas" for logging, last_epoch, and the ValueError past total_steps) and the state_dict,
    which holds no extra key, so a checkpoint's sched_state loads into either class. The constructor only registers
    itself with the optimizer, which reads total_steps and the first phase's end from it and the remaining constants
    from the keys torch keeps in each param group. With any other optimizer (SGD, NAdam, torch's Adam, CPU), or with
    an option the kernel does not evaluate (three_phase, linear annealing, cycle_momentum=False), nothing is
    registered and the class is torch's."""

    def __init__(self, optimizer, *args, **kwargs):
        super().__init__(optimizer, *args, **kwargs)
        if (isinstance(optimizer, _LciAdamStep) and len(self._schedule_phases) == 2
                and self._anneal_func_type == "cos" and self.cycle_momentum):
            optimizer._lci_sched = weakref.ref(self)


def _no_scheduler(config):
    return getattr(config, "scheduler_type", None) in (None, "None", "none")


def build_optimizer(params, config):
    """The reference's optimizers (optim_base.py:87-93; same hyper-parameters). On the GPU Adam / AdamW update on
    csrc/optim.hip (LciAdam / LciAdamW, torch-compatible state); LCI_HIP_ADAM=0 uses torch's fused kernel,
    LCI_FUSED_ADAM=0 torch's multi-tensor one (~150 launches per SwinUNETR step, 6.4 ms per C3 step).

    With --scheduler_type StepLR / ReduceLROnPlateau an LciAdam / LciAdamW gets its learning rate as one f32 device
    element: torch's scheduler classes then update it in place and a captured step sees the change."""
    o = config.optim
    params = list(params)
    fused = all(p.is_cuda for p in params) and os.environ.get("LCI_FUSED_ADAM", "1") != "0"
    hip = fused and os.environ.get("LCI_HIP_ADAM", "1") != "0"
    # only LciAdam / LciAdamW: SGD / NAdam keep torch's host float, which torch's schedulers then update as ever
    if (hip and params and config.optim_type in ("adam", "adamw")
            and getattr(config, "scheduler_type", None) in ("StepLR", "ReduceLROnPlateau")):
        o = argparse.Namespace(**vars(o))
        o.lr = torch.tensor(float(o.lr), device=params[0].device, dtype=torch.float32)
    if config.optim_type == "adam":
        if hip:
            return LciAdam(params, lr=o.lr, betas=(o.beta1, o.beta2), weight_decay=o.weight_decay)
        return torch.optim.Adam(params, lr=o.lr, betas=(o.beta1, o.beta2), weight_decay=o.weight_decay,
                                fused=fused or None)
    if config.optim_type == "adamw":
        if hip:
            return LciAdamW(params, lr=o.lr, betas=(o.beta1, o.beta2), weight_decay=o.weight_decay)
        return torch.optim.AdamW(params, lr=o.lr, betas=(o.beta1, o.beta2), weight_decay=o.weight_decay,
                                 fused=fused or None)
    if config.optim_type == "nadam":
        return torch.optim.NAdam(params, lr=o.lr, betas=(o.beta1, o.beta2), weight_decay=o.weight_decay)
    if config.optim_type == "sgd":   # optim_base.py:90-91: momentum 0.9
        return torch.optim.SGD(params, lr=o.lr, momentum=0.9, weight_decay=o.weight_decay)
    raise NotImplementedError(f"Optimizer not implemented: {config.optim_type}")


def compute_total_updates(config, num_samples: int, world: int = 1) -> int:
    """optim_utils.py:10-21: the optimizer updates of a whole run, OneCycleLR's total_steps."""
    per_update = config.batch_size * max(1, int(getattr(config, "iters_to_accumulate", 1) or 1)) * world
    return int(math.ceil(num_samples / per_update) * config.num_epochs)


def build_scheduler(optim, config, total_updates=None):
    """The reference's schedulers with its constructor arguments (optim_base.py:101-120); None for
    --scheduler_type None. OneCycleLR (every recipe's choice) needs `total_updates` (compute_total_updates) and is an
    LciOneCycleLR: evaluated in the update kernel for LciAdam / LciAdamW, plain torch for any other optimizer."""
    if _no_scheduler(config):
        return None
    s, kind = config.scheduler, config.scheduler_type
    if kind == "ReduceLROnPlateau":
        return torch.optim.lr_scheduler.ReduceLROnPlateau(optim, mode="min", factor=s.factor, patience=s.patience,
                                                          cooldown=s.cooldown, min_lr=s.min_lr)
    if kind == "StepLR":
        return torch.optim.lr_scheduler.StepLR(optim, step_size=s.step_size, gamma=s.gamma, last_epoch=-1)
    if kind == "OneCycleLR":
        if total_updates is None:
            raise ValueError("OneCycleLR needs total_updates (trainer.compute_total_updates)")
        return LciOneCycleLR(optim, max_lr=config.optim.lr, total_steps=int(total_updates), pct_start=s.pct_start,
                             anneal_strategy="cos")
    raise NotImplementedError(f"Scheduler not implemented: {kind}")


def loss_fn(config):
    if config.loss_func == "CrossEntropy":
        return nn.CrossEntropyLoss()
    if config.loss_func == "CombinationEnhance":   # loss/loss_base.py:28-29, the enhancement recipes' loss
        from .losses import CombinationEnhanceLoss
        return CombinationEnhanceLoss()
    return nn.MSELoss()


class TrainStep:
    """model (already on device) -> DDP -> step(inputs, targets) returns the loss tensor (no host sync)."""

    def __init__(self, model, config, device, ddp: bool, total_updates: int | None = None):
        """total_updates: the optimizer updates of the whole run (compute_total_updates), needed by --scheduler_type
        OneCycleLR only (ValueError without it)."""
        self.device = device
        self.model = model
        if ddp:
            kw = {"device_ids": [device.index]} if device.type == "cuda" else {}
            # gradient_as_bucket_view: the parameters' .grad are views into DDP's all-reduce buckets instead of
            # separate tensors copied in and out of them (C5: 3.29 GB of f32 gradients, 805 M of them the zero
            # pos-embed, held once instead of twice)
            self.model = nn.parallel.DistributedDataParallel(model, find_unused_parameters=False,
                                                             broadcast_buffers=False, gradient_as_bucket_view=True,
                                                             **kw)
        self.optim = build_optimizer(self.model.parameters(), config)
        # optim_base.py:101-120; stepped per update (OneCycleLR, step()) or per epoch (end_epoch())
        self.sched_type = None if _no_scheduler(config) else config.scheduler_type
        self.sched = build_scheduler(self.optim, config, total_updates)
        self.hold_sched = False   # GraphedStep: the captured step must not advance the host mirror
        self.loss_func = loss_fn(config)
        self.use_amp = bool(config.use_amp)
        # --deterministic: every step runs under kernels.deterministic_mode (fixed-order gradient sums);
        # a GraphedStep of this trainer captures those launches
        self.deterministic = bool(getattr(config, "deterministic", False))
        self.clip = float(getattr(config, "clip_grad_norm", 0.0) or 0.0)
        # the clip on a CUDA LciAdam(W): norm and coefficient by kernels.grad_clip_coef, the multiply inside the
        # update kernel (p.grad itself stays unscaled; it is zeroed right after the step)
        self.fused_clip = (self.clip > 0 and isinstance(self.optim, _LciAdamStep)
                           and all(p.is_cuda and p.dtype == torch.float32 for p in self.model.parameters()))
        self.grad_norm = None     # the last clipped update's total gradient norm (device tensor)
        self.accum = max(1, int(getattr(config, "iters_to_accumulate", 1) or 1))
        self.micro = 0   # micro-batches since the last optimizer step (trainer_base.py:172 `idx`)
        self.dup_batch1 = any(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in model.modules())
        # opt-in: a metrics.TaskMetrics scored on every step (trainer_base.py:186 on_train_step_end), on the device
        self.metrics = None
        self.optim.zero_grad(set_to_none=True)

    def step(self, inputs, targets, update: bool | None = None):
        """trainer_base.py:160-182: a batch of 1 is duplicated (BatchNorm), autocast forward + loss /
        iters_to_accumulate, backward; the optional grad-norm clip, optimizer step and zero_grad run only at the end
        of an accumulation window, i.e. every `iters_to_accumulate` calls (`update=None`), as the reference's
        `(idx + 1) % iters_to_accumulate == 0`. `update=True` forces the step (the reference's last iteration of an
        epoch, `idx + 1 == total_iters`), `update=False` suppresses it."""
        if self.deterministic:
            from . import kernels
            with kernels.deterministic_mode(True):
                return self._step(inputs, targets, update)
        return self._step(inputs, targets, update)

    def _step(self, inputs, targets, update):
        if inputs.shape[0] == 1 and self.dup_batch1:
            inputs = torch.cat([inputs] * 2, dim=0)
            targets = torch.cat([targets] * 2, dim=0)
        dev = "cuda" if self.device.type == "cuda" else "cpu"
        with torch.autocast(device_type=dev, dtype=torch.bfloat16, enabled=self.use_amp):
            out = self.model(inputs)
            loss = self.loss_func(out, targets) / self.accum
        loss.backward()
        if self.metrics is not None:
            self.metrics.update(loss.detach() * self.accum, out.detach(), targets)
        self.micro += 1
        if update is None:
            update = self.micro % self.accum == 0
        if update:
            self._update()
        return loss.detach()

    def _update(self):
        """trainer_base.py:173-182: clip, optimizer step, zero_grad, and OneCycleLR's per-update step."""
        grads = None
        if self.fused_clip:
            grads = [p.grad for p in self.model.parameters() if p.grad is not None]
            if not grads or any(g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() for g in grads):
                grads = None
        if grads is not None:
            from . import kernels
            self.grad_norm, self.optim._lci_grad_coef = kernels.grad_clip_coef(grads, self.clip)
            try:
                self.optim.step()
            finally:
                self.optim._lci_grad_coef = None
        else:
            if self.clip > 0:
                self.grad_norm = nn.utils.clip_grad_norm_(self.model.parameters(), self.clip)
            self.optim.step()
        self.optim.zero_grad(set_to_none=True)
        self.micro = 0
        if self.sched_type == "OneCycleLR" and not self.hold_sched:
            self.sched.step()

    def end_epoch(self, loss=None):
        """trainer_base.py:211-219: the per-epoch schedulers. StepLR steps; ReduceLROnPlateau steps on `loss` (the
        epoch's validation loss, or the last step's as the reference falls back to). OneCycleLR and no scheduler:
        nothing to do."""
        if self.sched_type == "StepLR":
            self.sched.step()
        elif self.sched_type == "ReduceLROnPlateau":
            if loss is None:
                raise ValueError("end_epoch: ReduceLROnPlateau steps on a loss")
            self.sched.step(float(loss))


class GraphedStep:
    """A TrainStep captured once into a HIP graph and replayed (HIP graphs instead of a tracing compiler).

    The step (autocast forward, loss, backward, optimizer step, zero_grad) on static input/target buffers is warmed
    up on a side stream, then captured; `step(x, y)` copies the batch into the static buffers (skipped when they
    are the same tensors) and replays the graph. Every liblci launch goes to torch's current stream, so the
    kernels are captured as graph nodes; the per-op host work of the Python modules and autograd (~2000 launches
    per Swin-tiny step) is paid once at capture. Single process only (no DDP: its all-reduce hooks are not part
    of the capture here); the optimizer runs with capturable=True (fused Adam / AdamW keep their step on device).

    Constructing it TRAINS: the `warmup` side-stream steps are real optimizer steps on the static batch (`warmup`
    updates before the first replay; the capture itself records the step and runs nothing). If the capture fails, the optimizer's `capturable`
    flags are restored before the error propagates (the weights keep the warm-up updates). Gradient accumulation
    (iters_to_accumulate > 1) is refused: the graph replays one fixed step, always with the optimizer update.

    With an LR scheduler the optimizer must be LciAdam / LciAdamW (ValueError otherwise): its kernel evaluates
    OneCycleLR from the device step count and reads StepLR's / ReduceLROnPlateau's learning rate from a device tensor
    (step those with `trainer.end_epoch()` between replays). OneCycleLR's host mirror advances once per warm-up step
    and once per replay, not for the capture, so after any sequence of warm-up, capture and replays
    `sched.last_epoch == int(optim.state[p]["step"])`; a replay past total_steps raises torch's ValueError before
    anything is launched. Per replay the host does the mirror's float arithmetic and nothing else. A param group
    that would take torch's fused update instead of the HIP kernel (amsgrad, non-f32 parameters, a GradScaler) under
    OneCycleLR makes the capture raise ValueError: its host lr / betas would become constants of the graph.
    """

    def __init__(self, trainer: "TrainStep", inputs, targets, warmup: int = 2):
        if not isinstance(trainer.model, nn.Module) or isinstance(trainer.model, nn.parallel.DistributedDataParallel):
            raise ValueError("GraphedStep: single-process TrainStep only")
        if trainer.accum != 1:
            raise ValueError("GraphedStep: iters_to_accumulate > 1 is not supported (the graph always updates)")
        # a schedule must reach the captured update through device memory: LciAdam / LciAdamW evaluate OneCycleLR in
        # the kernel and read StepLR's / ReduceLROnPlateau's learning rate from a device tensor; a host float of any
        # other optimizer would be baked into the graph at capture
        if trainer.sched is not None and not (
                isinstance(trainer.optim, _LciAdamStep)
                and all(trainer.optim.onecycle_constants(g) is not None if trainer.sched_type == "OneCycleLR"
                        else isinstance(g["lr"], torch.Tensor) for g in trainer.optim.param_groups)):
            raise ValueError("GraphedStep: an LR scheduler needs the LciAdam / LciAdamW optimizer (the captured "
                             "update reads the schedule on the device)")
        # TrainStep.step's duplication of a batch of 1, once on the static buffers; replays duplicate exactly when
        # the capture did (a BatchNorm model captured at batch 1), never a genuine batch of 2
        self.dup = inputs.shape[0] == 1 and trainer.dup_batch1
        if self.dup:
            inputs, targets = self._dup(inputs), self._dup(targets)
        saved = [(g, g["capturable"]) for g in trainer.optim.param_groups if "capturable" in g]
        for g, _ in saved:
            g["capturable"] = True
        self.trainer = trainer
        self.inputs, self.targets = inputs, targets
        try:
            side = torch.cuda.Stream(device=inputs.device)
            side.wait_stream(torch.cuda.current_stream(inputs.device))
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    trainer.step(inputs, targets, update=True)
            torch.cuda.current_stream(inputs.device).wait_stream(side)
            torch.cuda.synchronize(inputs.device)
            self.graph = torch.cuda.CUDAGraph()
            # the capture runs nothing, so it must not advance the scheduler's host mirror either: the mirror moves
            # once per warm-up step and once per replay, and last_epoch stays equal to the device step count
            trainer.hold_sched = True
            # relaxed: the kernels' one-time launch attributes (hipFuncSetAttribute) are legal during the capture
            with torch.cuda.graph(self.graph, capture_error_mode="relaxed"):
                self.loss = trainer.step(inputs, targets, update=True)
        except Exception:
            for g, c in saved:
                g["capturable"] = c
            raise
        finally:
            trainer.hold_sched = False

    @staticmethod
    def _dup(t):
        return None if t is None else torch.cat([t] * 2, dim=0)

    def step(self, inputs=None, targets=None):
        if inputs is not None and inputs is not self.inputs:
            if self.dup and inputs.shape[0] == 1:
                inputs = self._dup(inputs)
            self.inputs.copy_(inputs)
        if targets is not None and targets is not self.targets:
            if self.dup and targets.shape[0] == 1:
                targets = self._dup(targets)
            self.targets.copy_(targets)
        sched = self.trainer.sched
        if self.trainer.sched_type == "OneCycleLR":
            # the host mirror of the update about to be replayed (float arithmetic only); past total_steps torch's
            # ValueError stops the replay before anything is launched, with the mirror left where the device is
            try:
                sched.step()
            except ValueError:
                sched.last_epoch -= 1
                sched._step_count -= 1
                raise
        self.graph.replay()
        return self.loss


class EvalStep:
    """The reference's evaluation step (trainer_base.py:292-315): step(inputs, targets) runs the model in eval()
    under torch.inference_mode() and the trainer's bf16 autocast, computes the configured loss and scores the batch
    into `self.metrics` (a metrics.TaskMetrics unless one is passed, sums kept on the device). Returns (output, loss), both device
    tensors: no host sync per step; `metrics.result()` is the one sync of an evaluation loop. Every module's training
    flag is restored afterwards, so a step can be interleaved with training.

    Deviation: a batch of 1 is not duplicated. The reference repeats it and slices the output back
    (trainer_base.py:305-311) "so batch norm doesn't throw an error", but in eval mode BatchNorm normalises with its
    running statistics, which neither fails on one sample nor depends on the batch: the duplicate only doubles the
    work."""

    def __init__(self, model, config, device, metrics=None):
        """metrics: the metric manager to score into (metrics.build_metrics(config, "eval", capacity) for the
        classification metrics); default a TaskMetrics(config)."""
        from .metrics import TaskMetrics
        self.device = device
        self.model = model
        self.loss_func = loss_fn(config)
        self.use_amp = bool(config.use_amp)
        self.metrics = TaskMetrics(config) if metrics is None else metrics

    def step(self, inputs, targets):
        flags = [(m, m.training) for m in self.model.modules()]
        self.model.eval()
        dev = "cuda" if self.device.type == "cuda" else "cpu"
        try:
            with torch.inference_mode(), torch.autocast(device_type=dev, dtype=torch.bfloat16, enabled=self.use_amp):
                out = self.model(inputs)
                loss = self.loss_func(out, targets)
                self.metrics.update(loss, out, targets)
        finally:
            for m, flag in flags:
                m.training = flag
        return out, loss


def synthetic_batch(config, batch, device, seed):
    """U[0,1) images (B, C, T, H, W) and targets of the task's shape."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(batch, config.no_in_channel, config.time, config.height, config.width, generator=g)
    if config.task_type == "seg":
        y = torch.randint(0, config.no_out_channel, (batch, config.time, config.height, config.width), generator=g)
    elif config.task_type == "class":
        y = torch.randint(0, config.no_out_channel, (batch,), generator=g)
    else:
        y = torch.randn(batch, config.no_out_channel, config.time, config.height, config.width, generator=g)
    return x.to(device), y.to(device)


__all__ = ["init_distributed", "TrainStep", "EvalStep", "synthetic_batch", "LciAdam", "LciAdamW", "LciOneCycleLR",
           "build_scheduler", "compute_total_updates", "F"]
