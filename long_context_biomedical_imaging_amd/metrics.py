"""Per-step task metrics — the reference's metrics/metrics_base.py (:50-126, :150-215) and metrics_utils.AverageMeter.

The reference scores every training and evaluation step through torchmetrics and pulls each value to the host with
`.item()`: one device sync per metric per step. TaskMetrics runs the fused ops of csrc/metrics.hip
(kernels.enhance_metrics, kernels.seg_f1) and keeps the running sums `value * n` and the counts `n` on the device;
the only sync is `result()`.

  task_type   metrics                reference
  enhance     loss, ssim, psnr       torchmetrics SSIM / PSNR, data_range=None (metrics_base.py:99-115)
  seg         loss, f1               samplewise macro F1 of argmax, averaged over the batch (metrics_base.py:80-97)
  other       loss                   classification's acc_1 / auroc / f1 on (B,) vectors are not provided
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


__all__ = ["AverageMeter", "TaskMetrics", "metric_names"]
