#!/usr/bin/env python
"""Times the optimizer update with an LR schedule (csrc/optim.hip: lci_adam_step_ex, lci_grad_sumsq,
lci_grad_clip_coef) on the parameter lists of the C3 model (Swin-tiny + SwinUNETR, bench.py's swin_p2_128) and the
metric model (ViT-small + ViTUNETR, vit_p2_512).

    python tools/optim_bench.py [--out profiles/optim_sched_bench.txt] [--rounds 7] [--iters 20]
                                [--other-lib path/to/another/liblci.so]

--other-lib adds the constant-lr lci_adam_step of another build of the library (the parent commit's, built in a
checkout of it) against this tree's, for the "did the constant path regress" question. The file is rewritten by every
run; lines a person adds below the tool's say so themselves.

Variants, all updating the same f32 parameters, random gradients and optimizer state (shared buffers):
  a  constant-lr lci_adam_step (LciAdam)
  b  the one-cycle schedule evaluated in the kernel (LciAdam + LciOneCycleLR; the host mirror steps per update)
  c  the learning rate read from a device tensor (LciAdam(lr=tensor))
  d  fused clip: kernels.grad_clip_coef (norm pass) + the step multiplying by the coefficient
  e  nn.utils.clip_grad_norm_ + a
  f  torch's fused Adam (capturable) + torch's OneCycleLR.step()
Expected from the bytes moved per parameter alone: a = b = c = 28 B (read p, g, m, v; write p, m, v), d = 32 B (the
norm pass reads g once more), e = 40 B (clip_grad_norm_ reads g for the norm, then reads and writes it).

Timing: every variant's update is captured into a HIP graph once (how the Swin workloads run their step: the host work
of ~300 tensors' argument lists is paid at capture) and `iters` replays are timed between two HIP events; the variants
alternate over `rounds` rounds in one process; best and median round are reported, with a's own round-to-round range
as the yardstick for b and c. A scheduler's host-side step() runs once per replay where the trainer would run it. A
GPU is required: there is no CPU timing path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from long_context_biomedical_imaging_amd import config as lconfig  # noqa: E402
from long_context_biomedical_imaging_amd import kernels  # noqa: E402
from long_context_biomedical_imaging_amd.trainer import LciAdam, LciOneCycleLR  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X
MODELS = [("C3 swin_p2_128 (Swin-tiny + SwinUNETR)", "swin_p2_128"), ("metric vit_p2_512 (ViT-small + ViTUNETR)",
                                                                      "vit_p2_512")]
BYTES = {"a": 28, "b": 28, "c": 28, "d": 32, "e": 40, "f": 28}
KW = dict(betas=(0.9, 0.99), eps=1e-8)
MAX_NORM = 1.0


def param_shapes(workload):
    """The model's parameter shapes, from the model built on the host (no weights are kept)."""
    import bench
    from long_context_biomedical_imaging_amd.model_base import EncoderDecoderModel
    cfg = lconfig.parse_config(bench.WORKLOADS[workload] + ["--batch_size", "1"])
    model = EncoderDecoderModel(cfg, cfg.encoder_name, cfg.decoder_name, cfg.no_in_channel, cfg.no_out_channel)
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


class Variant:
    """One optimizer; `update` is captured once and replayed. Every variant updates the SAME buffers (parameters,
    gradients, exp_avg, exp_avg_sq, step counts: the first variant's state dicts are shared), so where an allocation
    happens to lie in HBM cannot favour one of them (separate copies differed by +-3 % between variants on that alone).
    The values drift as the replays go on (e rescales the shared gradients in place); the time does not depend on
    them."""

    def __init__(self, key, params, dev, state=None):
        self.key = key
        self.params = params
        self.sched = None
        if key == "f":
            self.opt = torch.optim.Adam(self.params, lr=1e-4, fused=True, capturable=True, **KW)
            self.sched = torch.optim.lr_scheduler.OneCycleLR(self.opt, max_lr=1e-4, total_steps=10 ** 7)
        elif key == "c":
            self.opt = LciAdam(self.params, lr=torch.tensor(1e-4, device=dev), **KW)
        else:
            self.opt = LciAdam(self.params, lr=1e-4, **KW)
            if key == "b":
                self.sched = LciOneCycleLR(self.opt, max_lr=1e-4, total_steps=10 ** 7)
        if state is not None:
            for p in params:
                self.opt.state[p] = state[p]
        self.update()                       # creates the optimizer state (first variant) outside the capture
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.update()

    def update(self):
        if self.key == "d":
            _, self.opt._lci_grad_coef = kernels.grad_clip_coef([p.grad for p in self.params], MAX_NORM)
            self.opt.step()
            self.opt._lci_grad_coef = None
        elif self.key == "e":
            torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
            self.opt.step()
        else:
            self.opt.step()

    def replay(self):
        self.graph.replay()
        if self.sched is not None:
            self.sched.step()


def bench_model(name, workload, rounds, iters, emit, dev):
    shapes = param_shapes(workload)
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    g = torch.Generator(device=dev).manual_seed(2)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.02) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g)
    variants = []
    for k in "abcdef":
        variants.append(Variant(k, params, dev, variants[0].opt.state if variants else None))
    for v in variants:
        for _ in range(3):
            v.replay()
    torch.cuda.synchronize()
    times = {v.key: [] for v in variants}
    for _ in range(rounds):
        for v in variants:
            times[v.key].append(_time(v.replay, iters))
    res = {}
    for k, ts in times.items():
        best, med = min(ts), statistics.median(ts)
        res[k] = {"best_ms": round(best, 4), "median_ms": round(med, 4), "worst_ms": round(max(ts), 4),
                  "bytes_per_param": BYTES[k], "gb_s_best": round(BYTES[k] * n / best / 1e6, 1),
                  "share_of_hbm_peak": round(BYTES[k] * n / (best * 1e-3) / HBM_PEAK, 3)}
    lo, hi = res["a"]["best_ms"], res["a"]["worst_ms"]
    verdict = {
        "a_round_range_ms": [lo, hi],
        "b_within_a_range": bool(res["b"]["best_ms"] <= hi and res["b"]["median_ms"] <= hi),
        "c_within_a_range": bool(res["c"]["best_ms"] <= hi and res["c"]["median_ms"] <= hi),
        "d_faster_than_e": bool(res["d"]["median_ms"] < res["e"]["median_ms"] and res["d"]["best_ms"] < res["e"]["best_ms"]),
        "d_over_e_median": round(res["d"]["median_ms"] / res["e"]["median_ms"], 3),
        "a_over_f_median": round(res["a"]["median_ms"] / res["f"]["median_ms"], 3),
    }
    emit({"model": name, "tensors": len(shapes), "parameters": n, "rounds": rounds, "iters": iters, "variants": res,
          "verdict": verdict})
    del variants, params
    torch.cuda.empty_cache()


def bench_other_lib(name, workload, other, rounds, iters, emit, dev):
    """lci_adam_step (constant lr) of another build of liblci.so, e.g. the parent commit's, against this tree's: both
    libraries loaded into this process with ctypes, the same buffers, one captured update each, replays alternating
    (the order swaps every round). The C entry point is called directly, so the binding's ABI check does not apply."""
    import ctypes
    from long_context_biomedical_imaging_amd import _lib
    P = ctypes.c_void_p
    libs = {"other": ctypes.CDLL(os.path.abspath(other)), "this": ctypes.CDLL(_lib.DEFAULT_LIB)}
    for lib in libs.values():
        _lib.bind(lib, ["lci_adam_step"])
    shapes = param_shapes(workload)
    g = torch.Generator(device=dev).manual_seed(3)
    p = [torch.randn(s, device=dev, generator=g) * 0.02 for s in shapes]
    gr = [torch.randn(s, device=dev, generator=g) for s in shapes]
    m, v = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p]
    st = [torch.ones((), device=dev) for _ in p]

    def update(lib):
        stream = torch.cuda.current_stream().cuda_stream
        for i0 in range(0, len(p), 40):
            sl = slice(i0, i0 + 40)
            n = len(p[sl])
            arr = lambda ts: (P * n)(*[t.data_ptr() for t in ts])   # noqa: E731
            sizes = (ctypes.c_longlong * n)(*[t.numel() for t in p[sl]])
            if lib.lci_adam_step(arr(p[sl]), arr(gr[sl]), arr(m[sl]), arr(v[sl]), arr(st[sl]), sizes, n, 1e-4, 0.9,
                                 0.99, 0.0, 1e-8, 0, 0, stream) != 0:
                raise RuntimeError("lci_adam_step failed")

    graphs = {}
    for k, lib in libs.items():
        update(lib)
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            update(lib)
    times = {k: [] for k in libs}
    for r in range(rounds):
        for k in (("other", "this") if r % 2 == 0 else ("this", "other")):
            times[k].append(_time(graphs[k].replay, iters))
    emit({"model": name, "lci_adam_step": "another build's library against this tree's, one process, same buffers",
          "rounds": rounds, "iters": iters,
          **{k: {"best_ms": round(min(t), 4), "median_ms": round(statistics.median(t), 4),
                 "worst_ms": round(max(t), 4)} for k, t in times.items()}})
    del graphs, p, gr, m, v, st
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_sched_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--other-lib", default=None, metavar="LIBLCI_SO",
                    help="also time lci_adam_step of this build of liblci.so (e.g. the parent commit's) against this "
                         "tree's on the same buffers")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_bench: needs a GPU (no CPU timing path)")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/optim_bench.py  (one {torch.cuda.get_device_name(0)}, {arch}; HIP events around {a.iters} graph "
             f"replays per round, {a.rounds} alternating rounds, best / median / worst round; f32; variants: a constant "
             "lr, b in-kernel one-cycle, c tensor lr, d fused clip (norm pass + step), e clip_grad_norm_ + a, f torch "
             "fused Adam + OneCycleLR.step())"]

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    for name, workload in MODELS:
        bench_model(name, workload, a.rounds, a.iters, emit, dev)
    if a.other_lib:
        for name, workload in MODELS:
            bench_other_lib(name, workload, a.other_lib, a.rounds, a.iters, emit, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
