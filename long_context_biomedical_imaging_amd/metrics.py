"""Per-step task metrics — the reference's metrics/metrics_base.py (:50-126, :150-215) and metrics_utils.AverageMeter.

The reference scores every training and evaluation step through torchmetrics and pulls each value to the host with
`.item()`: one device sync per metric per step. TaskMetrics runs the fused ops of csrc/metrics.hip
(kernels.enhance_metrics, kernels.seg_f1) and keeps the running sums `value * n` and the counts `n` on the device;
the only sync is `result()`.

  task_type   metrics                reference
  enhance     loss, ssim, psnr       torchmetrics SSIM / PSNR, data_range=None (metrics_base.py:99-115)
  seg         loss, f1               samplewise macro F1 of argmax, averaged over the batch (metrics_base.py:80-97)
  class       loss                   TaskMetrics scores the loss only; ClassMetrics (below, opt-in through build_metrics):
              train: loss, auroc                 softmax + torchmetrics AUROC per step (metrics_base.py:59-78, 157-160)
              eval: loss, acc_1, auroc, f1       + Accuracy, F1Score; with --exact_metrics once over every sample of
                                                 the epoch and of all ranks (metrics_base.py:268-285, 304-376)

ClassMetrics runs csrc/class_metrics.hip (kernels.class_metrics per step; kernels.class_append into a device buffer and
kernels.class_score once per epoch in exact mode). AUROC there is an exact integer count of ordered positive / negative
score pairs, not an f32 ROC curve; the definitions are restated in include/lci.h and DESIGN.md.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import _lib


class AverageMeter:
    """metrics/metrics_utils.py:32-57: the current value, the running count-weighted average and the history."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0
        self.vals = []
        self.counts = []

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count
        self.vals.append(val)
        self.counts.append(n)

    def status(self):
        import numpy as np
        return np.array(self.vals), np.array(self.counts)


def metric_names(task_type: str) -> tuple:
    if task_type == "enhance":
        return ("loss", "ssim", "psnr")
    if task_type == "seg":
        return ("loss", "f1")
    return ("loss",)


class TaskMetrics:
    """The metric manager's per-step update and per-epoch average for one split.

    update(loss, output, labels): the step's metrics (n = output.shape[0], as the reference counts) are added to
    f64 device sums as value * n next to the count n, with in-place ops on buffers that are allocated once — no host
    sync, and a HIP-graph capture of the step replays the accumulation. reset() zeroes the sums in place. result()
    returns {name: sum / count} as floats after one sync; when torch.distributed is initialised the sums and counts
    are all-reduced first, the reference's count-weighted mean over ranks (metrics_base.py:191-215). Before any
    update the averages are NaN."""

    def __init__(self, config):
        self.task_type = getattr(config, "task_type", None)
        self.names = metric_names(self.task_type)
        self._acc = None   # (len(names) + 1,) f64: the sums of value * n, then the count

    def _buffer(self, device):
        if self._acc is None or self._acc.device != device:
            # a plain tensor even when first touched under inference_mode (EvalStep), so reset() works outside it
            with _lib.plain_tensors():
                self._acc = torch.zeros(len(self.names) + 1, device=device, dtype=torch.float64)
        return self._acc

    def values(self, loss, output, labels):
        """The step's metric values in `names` order as one (len(names),) f32 device tensor."""
        from . import kernels
        loss = torch.as_tensor(loss, device=output.device).detach().to(torch.float32).reshape(1)
        if self.task_type == "enhance":
            return torch.cat([loss, kernels.enhance_metrics(output, labels)])
        if self.task_type == "seg":
            f1, _ = kernels.seg_f1(output, labels)
            return torch.cat([loss, f1.reshape(1)])
        return loss

    def update(self, loss, output, labels):
        vals = self.values(loss, output, labels)
        n = output.shape[0]
        acc = self._buffer(vals.device)
        acc[:-1].add_(vals.to(torch.float64), alpha=n)
        acc[-1:].add_(n)
        return vals

    def reset(self):
        if self._acc is not None:
            self._acc.zero_()

    def result(self) -> dict:
        ranks = dist.is_available() and dist.is_initialized()
        if self._acc is None:
            if not ranks:
                return {k: float("nan") for k in self.names}
            # a rank without a step still takes part in the all-reduce
            self._buffer(torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl"
                         else torch.device("cpu"))
        acc = self._acc.clone()
        if ranks:
            dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        *sums, count = acc.tolist()
        return {k: (s / count if count else float("nan")) for k, s in zip(self.names, sums)}


CLASS_METRICS = {"train": ("loss", "auroc"), "eval": ("loss", "acc_1", "auroc", "f1")}
_CLASS_SLOT = {"acc_1": 0, "auroc": 1, "f1": 2}   # kernels.class_score's result order


def merge_rank_rows(probs, labels, counts):
    """The union of the ranks' stored rows: probs[r] (>= counts[r], K) and labels[r] (>= counts[r],) hold rank r's
    rows, padded to a common length for the all-gather; the padding is cut off and the rest concatenated in rank
    order."""
    return (torch.cat([p[:n] for p, n in zip(probs, counts)]), torch.cat([l[:n] for l, n in zip(labels, counts)]))


class ClassMetrics:
    """TaskMetrics' interface (names, values, update, reset, result) for task_type=class.

    split "train": ("loss", "auroc"); "eval": ("loss", "acc_1", "auroc", "f1"), the reference's metric sets
    (metrics_base.py:59-78). Every step is scored by kernels.class_metrics and its values are averaged with the
    weights n = B, exactly as TaskMetrics does (f64 device sums, no host sync before result()).

    Exact mode (split "eval" and config.exact_metrics): update() only appends the batch's softmax rows and labels to
    a device buffer of `capacity` rows (kernels.class_append) and adds loss * n; result() scores all rows at once
    (kernels.class_score). The buffers are plain tensors allocated at the first update, so they survive
    inference_mode and a captured update appends on every replay; reset() zeroes the row count in place. result() is
    the only sync: it raises RuntimeError when more rows were fed than `capacity`; when torch.distributed is
    initialised it all-gathers the ranks' row counts, then their rows padded to the largest count (over the host
    when the backend is gloo), scores the union on every rank and all-reduces the loss sum and count.

    Deviations from the reference: C == 1 raises ValueError (softmax over one column is constant); every rank gets
    the exact values, not only rank 0; ranks may hold different sample counts (dist.gather needs equal ones); a label
    outside [0, C) is not checked: it is never a positive and never a correct prediction."""

    def __init__(self, config, split: str, capacity: int | None = None):
        if split not in CLASS_METRICS:
            raise ValueError(f"ClassMetrics: split {split!r} (train or eval)")
        self.task_type = getattr(config, "task_type", None)
        if self.task_type != "class":
            raise ValueError(f"ClassMetrics: task_type {self.task_type!r} (class only)")
        self.split = split
        self.names = CLASS_METRICS[split]
        self.exact = split == "eval" and bool(getattr(config, "exact_metrics", False))
        if self.exact and (capacity is None or int(capacity) < 1):
            raise ValueError("ClassMetrics: exact_metrics needs capacity, the evaluation epoch's samples on this rank")
        self.capacity = int(capacity) if self.exact else None
        self.num_classes = getattr(config, "no_out_channel", None)
        self._acc = None      # non-exact: the sums of value * n, then n; exact: the sum of loss * n, then n (f64)
        self._probs = self._labels = self._count = None

    @staticmethod
    def _check(output, labels):
        if output.dim() != 2 or output.shape[1] < 2:
            raise ValueError(f"ClassMetrics: output {tuple(output.shape)} must be (B, C) with C >= 2")
        if not output.is_cuda:
            raise _lib.LciError("liblci ops run on the GPU only (tensor on %s); there is no CPU path" % output.device)

    def _buffer(self, device):
        if self._acc is None or self._acc.device != device:
            with _lib.plain_tensors():
                self._acc = torch.zeros(2 if self.exact else len(self.names) + 1, device=device, dtype=torch.float64)
        return self._acc

    def _rows(self, device, C):
        if self._probs is None or self._probs.device != device or self.num_classes != C:
            self.num_classes = C
            with _lib.plain_tensors():
                self._probs = torch.zeros(self.capacity, 1 if C == 2 else C, device=device, dtype=torch.float32)
                self._labels = torch.zeros(self.capacity, device=device, dtype=torch.int64)
                self._count = torch.zeros(1, device=device, dtype=torch.int64)
        return self._probs, self._labels, self._count

    def _values64(self, loss, output, labels):
        from . import kernels
        self._check(output, labels)
        res, _, _ = kernels.class_metrics(output, labels)
        loss = torch.as_tensor(loss, device=output.device).detach().to(torch.float64).reshape(1)
        # slices only (an index list would be a host-to-device copy): eval takes all three, train the auroc
        return torch.cat([loss, res if self.split == "eval" else res[1:2]])

    def values(self, loss, output, labels):
        """The step's metric values in `names` order as one (len(names),) f32 device tensor."""
        return self._values64(loss, output, labels).to(torch.float32)

    def update(self, loss, output, labels):
        n = output.shape[0]
        if not self.exact:
            vals = self._values64(loss, output, labels)
            acc = self._buffer(vals.device)
            acc[:-1].add_(vals, alpha=n)
            acc[-1:].add_(n)
            return vals.to(torch.float32)
        from . import kernels
        self._check(output, labels)
        probs, lab, count = self._rows(output.device, output.shape[1])
        kernels.class_append(output, labels, probs, lab, count)
        loss = torch.as_tensor(loss, device=output.device).detach().to(torch.float64).reshape(1)
        acc = self._buffer(output.device)
        acc[:1].add_(loss, alpha=n)
        acc[1:].add_(n)
        return loss.to(torch.float32)

    def reset(self):
        if self._acc is not None:
            self._acc.zero_()
        if self._count is not None:
            self._count.zero_()

    def _mean_result(self, ranks):
        if self._acc is None:
            if not ranks:
                return {k: float("nan") for k in self.names}
            self._buffer(torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl"
                         else torch.device("cpu"))
        acc = self._acc.clone()
        if ranks:
            if dist.get_backend() != "nccl":
                acc = acc.cpu()
            dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        *sums, count = acc.tolist()
        return {k: (s / count if count else float("nan")) for k, s in zip(self.names, sums)}

    def result(self) -> dict:
        ranks = dist.is_available() and dist.is_initialized()
        if not self.exact:
            return self._mean_result(ranks)
        if self._count is None and not ranks:
            return {k: float("nan") for k in self.names}
        from . import kernels
        if self._count is None:
            # a rank without a step still takes part in the gathers
            if self.num_classes is None:
                raise RuntimeError("ClassMetrics: a rank without an update needs config.no_out_channel")
            self._rows(torch.device("cuda", torch.cuda.current_device()), int(self.num_classes))
            self._buffer(self._count.device)
        n = int(self._count.item())
        if n > self.capacity:
            raise RuntimeError(f"ClassMetrics: {n} rows were fed to a buffer of capacity {self.capacity}")
        device = self._count.device
        probs, labels, acc = self._probs, self._labels, self._acc.clone()
        if ranks:
            host = dist.get_backend() != "nccl"
            via = torch.device("cpu") if host else device
            world = dist.get_world_size()
            mine = torch.tensor([n], dtype=torch.int64, device=via)
            every = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            counts = [int(c.item()) for c in every]
            pad = max(max(counts), 1)
            # a rank whose capacity is below the largest count sends zero rows past its own: they are cut off again
            p = torch.zeros(pad, probs.shape[1], dtype=torch.float32, device=via)
            l = torch.zeros(pad, dtype=torch.int64, device=via)
            p[:n].copy_(probs[:n])
            l[:n].copy_(labels[:n])
            ps, ls = [torch.empty_like(p) for _ in range(world)], [torch.empty_like(l) for _ in range(world)]
            dist.all_gather(ps, p)
            dist.all_gather(ls, l)
            probs, labels = merge_rank_rows(ps, ls, counts)
            probs, labels = probs.to(device), labels.to(device)
            n = sum(counts)
            acc = acc.to(via)
            dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        loss_sum, count = acc.tolist()
        out = {"loss": loss_sum / count if count else float("nan")}
        if n == 0:
            out.update({k: float("nan") for k in self.names[1:]})
            return out
        res, _, _ = kernels.class_score(probs, labels, n, int(self.num_classes))
        vals = res.tolist()
        out.update({k: vals[_CLASS_SLOT[k]] for k in self.names[1:]})
        return out


def build_metrics(config, split: str, capacity: int | None = None):
    """The metric manager of one split: a ClassMetrics for task_type=class (split "train" or "eval"; `capacity` rows
    for --exact_metrics), a TaskMetrics otherwise."""
    if getattr(config, "task_type", None) == "class":
        return ClassMetrics(config, split, capacity)
    return TaskMetrics(config)


__all__ = ["AverageMeter", "TaskMetrics", "ClassMetrics", "build_metrics", "merge_rank_rows", "metric_names",
           "CLASS_METRICS"]
