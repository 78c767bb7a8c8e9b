#!/usr/bin/env python
"""Times the fused task metrics (kernels.enhance_metrics, kernels.seg_f1: csrc/metrics.hip) against the torch composite
a torchmetrics-based step executes, in f32 on the same GPU, at the recipes' shapes.

    python tools/metrics_bench.py [--out profiles/metrics_bench.txt] [--rounds 5]

Composite, enhance: the restatement of tests/test_metrics_cpu.py with the dense grouped convolution (reflect-pad 5,
one 11 x 11 (x 11) 'valid' conv over the five stacked moment maps with groups = 5 C, crop 5), min / max for the data
range, and PSNR from the squared error — the torch ops torchmetrics launches. Composite, seg: torch.argmax and a
bincount over (sample, label, prediction) for the confusion counts, then the F1 arithmetic on the (B, C) counts.
Neither composite copies anything to the host, which flatters it: the reference adds one .item() per metric.

Timing: HIP events around `iters` back-to-back calls on one stream, after a warm-up of every variant; fused and
composite alternate over `rounds` rounds in one process and the best and the median round are reported. Peak memory is
torch's allocator peak over one call above what was allocated before it. The share of the HBM peak takes the bytes
the metric needs at least (every input read once) over the fused time; both metrics are bandwidth-bound by that
count. A GPU is required: there is no CPU timing path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from long_context_biomedical_imaging_amd import kernels  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X
ENHANCE_SHAPES = [("run_micro", (2, 1, 1, 1024, 1024)), ("run_cmr", (2, 1, 32, 128, 128))]
SEG_SHAPES = [("run_abct", (1, 10, 64, 256, 256)), ("run_vessel", (2, 2, 1, 1024, 1024))]


def composite_enhance(p, t):
    if p.shape[2] == 1:
        p, t = p[:, :, 0], t[:, :, 0]
    nd, C = p.dim() - 2, p.shape[1]
    j = torch.arange(11, device=p.device, dtype=p.dtype)
    g = torch.exp(-(((j - 5) / 1.5) ** 2) / 2)
    g = g / g.sum()
    k = g
    for _ in range(nd - 1):
        k = k.unsqueeze(-1) * g
    R = torch.maximum(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    pp, tp = F.pad(p, (5, 5) * nd, mode="reflect"), F.pad(t, (5, 5) * nd, mode="reflect")
    stack = torch.cat([pp, tp, pp * pp, tp * tp, pp * tp], dim=1)
    out = (F.conv2d if nd == 2 else F.conv3d)(stack, k.expand(5 * C, 1, *k.shape).contiguous(), groups=5 * C)
    mp, mt, epp, ett, ept = out.split(C, dim=1)
    vp, vt, cov = (epp - mp * mp).clamp_min(0), (ett - mt * mt).clamp_min(0), ept - mp * mt
    s = ((2 * mp * mt + c1) * (2 * cov + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
    s = s[(..., *([slice(5, -5)] * nd))]
    ssim = s.reshape(s.shape[0], -1).mean(1).mean()
    zero = torch.zeros((), device=p.device, dtype=p.dtype)
    rng = torch.maximum(t.max(), zero) - torch.minimum(t.min(), zero)
    psnr = 10 * torch.log10(rng ** 2 / ((p - t) ** 2).mean())
    return torch.stack([ssim, psnr])


def composite_seg(logits, labels):
    B, C = logits.shape[:2]
    pred = torch.argmax(logits, 1).reshape(B, -1)
    lab = labels.reshape(B, -1)
    idx = (torch.arange(B, device=pred.device).unsqueeze(1) * C + lab) * C + pred
    conf = torch.bincount(idx.reshape(-1), minlength=B * C * C).reshape(B, C, C).double()
    tp = conf.diagonal(dim1=1, dim2=2)
    fp, fn = conf.sum(1) - tp, conf.sum(2) - tp
    den = 2 * tp + fp + fn
    per = torch.where(den > 0, 2 * tp / den.clamp_min(1), torch.zeros_like(den))
    f = per[:, 1] if C == 2 else per.sum(1) / (den > 0).sum(1).clamp_min(1)
    return f.mean().float()


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    del r
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def bench(name, cfg, fused, composite, min_bytes, rounds, iters, citers, emit):
    for _ in range(3):
        a, b = fused(), composite()
    torch.cuda.synchronize()
    a, b = [float(v) for v in a.reshape(-1)], [float(v) for v in b.reshape(-1)]
    tf, tc = [], []
    for _ in range(rounds):
        tf.append(_time(fused, iters))
        tc.append(_time(composite, citers))
    best_f, best_c = min(tf), min(tc)
    emit({"op": name, "config": cfg, "fused_ms": round(best_f, 4), "fused_ms_median": round(statistics.median(tf), 4),
          "composite_ms": round(best_c, 3), "composite_ms_median": round(statistics.median(tc), 3),
          "speedup": round(best_c / best_f, 1), "speedup_median": round(statistics.median(tc) / statistics.median(tf), 1),
          "rounds": rounds, "iters": [iters, citers], "peak_mib_fused": _peak_mib(fused),
          "peak_mib_composite": _peak_mib(composite), "min_bytes": min_bytes,
          "fused_gb_s": round(min_bytes / best_f / 1e6, 1), "share_of_hbm_peak": round(min_bytes / (best_f * 1e-3) / HBM_PEAK, 4),
          "fused_value": a, "composite_value": b})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--composite-iters", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metrics_bench: needs a GPU (no CPU timing path)")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/metrics_bench.py  (one {torch.cuda.get_device_name(0)}, {arch}; HIP events; f32; fused {a.iters} and "
             f"composite {a.composite_iters} calls per round, {a.rounds} alternating rounds, best and median round; "
             f"MIOPEN_FIND_MODE={os.environ['MIOPEN_FIND_MODE']})"]

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    g = torch.Generator().manual_seed(37)
    for recipe, shape in ENHANCE_SHAPES:
        t = torch.rand(shape, generator=g).to(dev)
        p = (t + 0.1 * torch.randn(shape, generator=g).to(dev)).contiguous()
        bench("enhance_metrics (ssim, psnr)", f"{recipe} {shape} float32", lambda: kernels.enhance_metrics(p, t),
              lambda: composite_enhance(p, t), 2 * 4 * p.numel(), a.rounds, a.iters, a.composite_iters, emit)
        del p, t
    for recipe, (B, C, *sp) in SEG_SHAPES:
        lg = torch.randn(B, C, *sp, generator=g).to(dev)
        lb = torch.randint(0, C, (B, *sp), generator=g).to(dev)
        bench("seg_f1", f"{recipe} logits {(B, C, *sp)} float32", lambda: kernels.seg_f1(lg, lb)[0],
              lambda: composite_seg(lg, lb), 4 * lg.numel() + 8 * lb.numel(), a.rounds, a.iters, a.composite_iters, emit)
        del lg, lb
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
