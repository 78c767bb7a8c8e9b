#!/usr/bin/env python3
"""Headline benchmark: image-tokens/s fwd+bwd, ViT patch=2 at 512^2 (L = 65 536), 1..8 MI355X.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    torchrun --nproc-per-node N bench.py --gpus N ...               (the driver's N > 1 launch; RCCL DDP)

A plain run does only what the headline figure needs: build the model, W untimed warm-up steps, exactly K timed
steps, the optional output dump, one JSON line (`value` = tokens/s, `ms_per_step` = milliseconds per timed step).
Everything else this file measures (listed under "`--full` also reports" below) takes steps or runs of its own and
sits behind `--full`.

`--dump-outputs DIR` writes what the timed path hands its caller in the last timed step (rank 0): `DIR/loss.npy`, the
loss `TrainStep.step` / `GraphedStep.step` returns, float32, shape (1,). Model weights (torch.manual_seed(0)) and the
batch (seed 1234 + rank) are the same from run to run, so two builds can be compared on it. Two runs of one build
agree to ~3e-4 relative at the metric config, not to the bit: weight gradients summed with float atomics (the patch
embedding's, csrc/patch_embed.hip) add in a different order from run to run and the later steps' weights carry that.

`python bench.py --gpus N` with N > 1 outside torchrun starts the N ranks itself (torch.distributed.run as a child
process, 127.0.0.1 rendezvous) before this process touches the GPU, and exits with its code; every rank checks
that the process group really has N ranks and the line reports `rccl_world` (the collective's world size).

A step = one DDP training step of the reference's segmentation model (trainer_base.py:157-182):
EncoderDecoderModel(ViT-small, p2, 512x512, 2-D) + ViTUNETR decoder, bf16 autocast, CrossEntropy loss,
backward (DDP gradient all-reduce over RCCL), Adam step — on synthetic U[0,1) images already on the GPU.
Throughput = (world * B * L) tokens / step time (max over ranks).

`--full` also reports (rank 0): `roofline` of the dominant liblci kernel (HIP events on that kernel's launches in the
last timed step; an untimed probe step picks it), per-kernel breakdown (two steps after the timed region), `cpu_baseline` = the CPU oracle's forward on a bounded sample (N = 1 only), and
`secondary.swin_p2_128` = the same harness on BASELINE configs[2] (Swin-tiny + SwinUNETR, 128^3 patch 2, one
volume per GPU), which north_star also names; for the HIP-graph workloads, `config.eager_ms_per_step` (the same step
timed eager). `--workload` runs one of the other configs on its own.
With `--full`, `--no-kernel-timer` drops the per-launch HIP events (for rocprofv3 PMC passes: the profiler serialises
dispatches and the extra event packets are not needed there); the line then has no `roofline`/`kernels`.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from long_context_biomedical_imaging_amd import config as lconfig  # noqa: E402
from long_context_biomedical_imaging_amd import kernels  # noqa: E402
from long_context_biomedical_imaging_amd.model_base import EncoderDecoderModel  # noqa: E402
from long_context_biomedical_imaging_amd.trainer import (GraphedStep, TrainStep, init_distributed, synthetic_batch,  # noqa: E402
                                                         use_tuned_gemms)

MFMA_BF16_PEAK_TFLOPS = 2500.0   # dense bf16, MI355X_MICROARCH.md chip table
HBM_PEAK_GBS = 8000.0
# kernels whose roofline is HBM: algorithmic bytes per unit of KernelTimer work (the scan's work is
# its algorithmic bytes already — 1184 / 1984 B per token at Dx = 192, N = 8, bf16 I/O; FFT-conv units are
# row-elements, f32 in/out). Others: MFMA FLOPs.
ROOF = {"selective_scan_fwd": ("hbm", 1.0), "selective_scan_bwd": ("hbm", 1.0),
        "fftconv_fwd": ("hbm", 8.0), "fftconv_bwd": ("hbm", 16.0),
        # LayerNorm work is counted in bytes already (f32 x in, bf16 y out; bwd + bf16 dy in, f32 dx out)
        "ln_fwd": ("hbm", 1.0), "ln_bwd": ("hbm", 1.0), "ln_add_fwd": ("hbm", 1.0),
        # GELU work is its bytes too (bf16 x in, y out; bwd + dy in)
        "gelu_fwd": ("hbm", 1.0), "gelu_bwd": ("hbm", 1.0),
        # direct (Toeplitz) long conv of Swin-window rows: FLOPs on the f32-input MFMA (157.3 TF dense)
        "direct_conv_fwd": ("mfma_f32", 1.0), "direct_conv_bwd": ("mfma_f32", 1.0), "direct_conv_dk": ("mfma_f32", 1.0)}
MFMA_F32_PEAK_TFLOPS = 157.3     # v_mfma_f32_32x32x2_f32, MI355X_MICROARCH.md chip table

WORKLOADS = {
    # metric config (BASELINE.json `metric`, configs[1] shape at patch 2): ViT-small, patch 2, 512x512 -> L = 65536
    "vit_p2_512": ["--encoder_name", "ViT", "--decoder_name", "ViTUNETR", "--task_type", "seg",
                   "--height", "512", "--width", "512", "--time", "1", "--no_in_channel", "1",
                   "--no_out_channel", "2", "--ViT.size", "small", "--ViT.patch_size", "1", "2", "2",
                   "--use_amp"],
    # configs[2] (C3): Swin-tiny + SwinUNETR 3-D segmentation, 128^3, patch 2, window 7 -> 64^3 = 262144 tokens
    "swin_p2_128": ["--encoder_name", "Swin", "--decoder_name", "SwinUNETR", "--task_type", "seg",
                    "--height", "128", "--width", "128", "--time", "128", "--no_in_channel", "1",
                    "--no_out_channel", "2", "--Swin.size", "tiny", "--Swin.patch_size", "2", "2", "2",
                    "--Swin.window_size", "7", "7", "7", "--use_amp"],
    # configs[4] (C5): ViT-small with the Mamba mixer + ViTUNETR 3-D segmentation, 256^3, patch 2 -> 2^21 tokens
    "vit_mamba_p2_256": ["--encoder_name", "ViT", "--decoder_name", "ViTUNETR", "--task_type", "seg",
                         "--height", "256", "--width", "256", "--time", "256", "--no_in_channel", "1",
                         "--no_out_channel", "2", "--ViT.size", "small", "--ViT.patch_size", "2", "2", "2",
                         "--ViT.use_mamba", "True", "--use_amp"],
    # ViT-small with the Hyena mixer at the metric shape (512^2 p2, L = 65536 <= the reference's l_max = 66000),
    # ViTUNETR head: the same mixer at the largest L the reference itself accepts
    "vit_hyena_p2_512": ["--encoder_name", "ViT", "--decoder_name", "ViTUNETR", "--task_type", "seg",
                         "--height", "512", "--width", "512", "--time", "1", "--no_in_channel", "1",
                         "--no_out_channel", "2", "--ViT.size", "small", "--ViT.patch_size", "1", "2", "2",
                         "--ViT.use_hyena", "True", "--use_amp"],
    # configs[3] (C4): ViT-small + Hyena + UperNet2D denoising (enhance, MSE), 1024^2 patch 2 -> L = 262144. The
    # reference raises here (l_max = 66000 hard-coded, hyena.py:314); --ViT.hyena_l_max 262144 is the opt-in
    # deviation that sizes the implicit filter for it (backbone_vit.HYENA_L_MAX)
    "vit_hyena_p2_1024": ["--encoder_name", "ViT", "--decoder_name", "UperNet2D", "--task_type", "enhance",
                          "--loss_func", "MSE", "--height", "1024", "--width", "1024", "--time", "1",
                          "--no_in_channel", "1", "--no_out_channel", "1", "--ViT.size", "small",
                          "--ViT.patch_size", "1", "2", "2", "--ViT.use_hyena", "True",
                          "--ViT.hyena_l_max", "262144", "--use_amp"],
    # configs[1] (C2): ViT-small + ViTUNETR 2-D segmentation, 512x512, patch 4 -> L = 16384, full attention
    "vit_p4_512": ["--encoder_name", "ViT", "--decoder_name", "ViTUNETR", "--task_type", "seg",
                   "--height", "512", "--width", "512", "--time", "1", "--no_in_channel", "1",
                   "--no_out_channel", "2", "--ViT.size", "small", "--ViT.patch_size", "1", "4", "4",
                   "--use_amp"],
    # the reference's project recipes (projects/run_*.sh): Swin-tiny patch 2 with Mamba / Hyena inside the windows
    # (shift 0, backbone_swin.py:674) + UperNet3D segmentation, here on a 128^3 volume (64^3 = 262144 tokens);
    # window 4 as run_abct.sh (Mamba), window 8 as run_cmr.sh (Hyena)
    "swin_mamba_p2_128": ["--encoder_name", "Swin", "--decoder_name", "UperNet3D", "--task_type", "seg",
                          "--height", "128", "--width", "128", "--time", "128", "--no_in_channel", "1",
                          "--no_out_channel", "2", "--Swin.size", "tiny", "--Swin.patch_size", "2", "2", "2",
                          "--Swin.window_size", "4", "4", "4", "--Swin.use_mamba", "True", "--use_amp"],
    "swin_hyena_p2_128": ["--encoder_name", "Swin", "--decoder_name", "UperNet3D", "--task_type", "seg",
                          "--height", "128", "--width", "128", "--time", "128", "--no_in_channel", "1",
                          "--no_out_channel", "2", "--Swin.size", "tiny", "--Swin.patch_size", "2", "2", "2",
                          "--Swin.window_size", "8", "8", "8", "--Swin.use_hyena", "True", "--use_amp"],
    # not a metric: a torch-only model (no HIP kernels), so the N-rank launch path itself can be rehearsed on CPU /
    # gloo (tests/test_ddp.py::test_bench_gpus2_launch_cpu)
    "rehearsal": ["--task_type", "enhance", "--loss_func", "MSE", "--optim_type", "adam"],
}
WORKLOAD_NAMES = {
    "vit_p4_512": ("image-tokens/sec fwd+bwd, ViT patch=4 512^2 (L=16384)",
                   "ViT-small p4 512x512 2-D seg (ViTUNETR head), full attention (BASELINE configs[1])"),
    "swin_mamba_p2_128": ("image-tokens/sec fwd+bwd, Swin-Mamba patch=2 128^3 (L=262144), window 4",
                          "Swin-tiny p2 128^3 3-D seg (UperNet3D head), Mamba inside 4^3 windows (run_abct.sh recipe)"),
    "swin_hyena_p2_128": ("image-tokens/sec fwd+bwd, Swin-Hyena patch=2 128^3 (L=262144), window 8",
                          "Swin-tiny p2 128^3 3-D seg (UperNet3D head), Hyena inside 8^3 windows (run_cmr.sh recipe)"),
    "vit_p2_512": ("image-tokens/sec fwd+bwd, ViT patch=2 512^2 (L=65536), 1/2/4/8 MI355X",
                   "ViT-small p2 512x512 2-D seg (ViTUNETR head), full attention"),
    "swin_p2_128": ("image-tokens/sec fwd+bwd, Swin patch=2 128^3 (L=262144), window 7",
                    "Swin-tiny p2 128^3 3-D seg (SwinUNETR head), shifted-window attention"),
    "vit_mamba_p2_256": ("image-tokens/sec fwd+bwd, ViT-Mamba patch=2 256^3 (L=2097152)",
                         "ViT-small p2 256^3 3-D seg (ViTUNETR head), Mamba selective-scan mixer"),
    "vit_hyena_p2_512": ("image-tokens/sec fwd+bwd, ViT-Hyena patch=2 512^2 (L=65536)",
                         "ViT-small p2 512x512 2-D seg (ViTUNETR head), Hyena FFT long-conv mixer"),
    "rehearsal": ("harness rehearsal (not a metric)",
                  "torch-only 2-layer MLP: rehearses the N-rank launch, barriers and max-over-ranks timing on CPU / gloo"),
    "vit_hyena_p2_1024": ("image-tokens/sec fwd+bwd, ViT-Hyena patch=2 1024^2 (L=262144), UperNet2D denoising",
                          "ViT-small p2 1024x1024 2-D enhance (UperNet2D head, MSE), Hyena FFT long-conv mixer, "
                          "hyena_l_max 262144 (opt-in; the reference raises above 66000)"),
}


def cpu_threads():
    """Host threads for the CPU baseline: every core in this process's affinity mask, capped by OMP_NUM_THREADS
    when the launcher sets it (the GPU box exposes the whole machine's CPUs but allots 16 per GPU and sets
    OMP_NUM_THREADS accordingly)."""
    n = len(os.sched_getaffinity(0))
    omp = os.environ.get("OMP_NUM_THREADS", "")
    return min(n, int(omp)) if omp.isdigit() and int(omp) > 0 else n


def cpu_baseline(budget_s: float = 20.0):
    """Oracle (CPU restatement) forward of the same encoder, bounded sample, extrapolated per token.

    SURVEY.md §8(d): the attention of one layer at L = 65536 is computed in query-row chunks of 4096 (per-row
    softmax is exact, 6.4 GB of f32 scores per chunk for the 6 heads); chunks are timed until the budget is
    spent and the per-chunk time is scaled to the 16 chunks of a layer. LN + qkv + out_proj + MLP are timed on
    one 4096-token chunk and scaled the same way. tokens/s = L / (12 * t_layer).
    """
    from oracle import attention as oatt
    ncores = cpu_threads()
    torch.set_num_threads(ncores)
    L, D, H, dh, MLP, CH = 65536, 384, 6, 64, 1536, 4096
    g = torch.Generator().manual_seed(0)
    w = {k: torch.randn(s, generator=g) * 0.02 for k, s in
         {"qkv": (3 * D, D), "out": (D, D), "l1": (MLP, D), "l2": (D, MLP)}.items()}
    x = torch.randn(1, CH, D, generator=g)
    F = torch.nn.functional
    t0 = time.perf_counter()
    h = F.layer_norm(x, (D,))
    qkv = F.linear(h, w["qkv"])
    o = F.linear(qkv[..., :D], w["out"])
    h2 = F.layer_norm(x + o, (D,))
    _ = F.linear(F.gelu(F.linear(h2, w["l1"])), w["l2"])
    t_lin = (time.perf_counter() - t0) * (L / CH)
    k = torch.randn(1, H, L, dh, generator=g)
    v = torch.randn(1, H, L, dh, generator=g)
    t_att, done = 0.0, 0
    t_start = time.perf_counter()
    while done < L and (done == 0 or time.perf_counter() - t_start < budget_s * 0.8):
        q = torch.randn(1, H, CH, dh, generator=g)
        t1 = time.perf_counter()
        oatt.attention_core(q, k, v, dh ** -0.5)
        t_att += time.perf_counter() - t1
        done += CH
    t_layer = t_lin + t_att * (L / done)
    return {"value": round(L / (12 * t_layer), 1), "unit": "image-tokens/s (fwd only, fp32)", "cores": ncores,
            "kind": "port",
            "sample": f"oracle ViT-small encoder forward at L=65536, B=1: per layer, attention over all 65536 keys "
                      f"in query-row chunks of {CH} (all 6 heads), {done // CH} of the layer's {L // CH} chunks "
                      f"timed, plus LN/Linear/MLP on one {CH}-token chunk; both scaled linearly to the full layer, "
                      f"x12 layers; {ncores} threads (affinity mask capped by OMP_NUM_THREADS)"}


def profiled_traffic(timer: str, workload: str):
    """HBM bytes per launch of KernelTimer `timer` in `workload`, from that workload's committed PMC profile
    (profiles/traffic.json `workloads`, written by tools/summarize_prof.py from separate rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE passes of that workload, or by tools/fft_traffic.py for the FFT-conv timers, which launch several
    kernels per call), or None when the workload has no such profile. Returns (bytes, source)."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    if not os.path.exists(path):
        return None, None
    with open(path) as f:
        prof = json.load(f)
    wl = prof.get("workloads", {}).get(workload)
    if not wl or timer not in wl.get("timers", {}):
        return None, None
    return int(wl["timers"][timer]["bytes_per_call"]), f"profiles/traffic.json workloads.{workload} ({wl['source']})"


def profiled_launch_ms(timer: str, workload: str):
    """Average launch time of KernelTimer `timer` in `workload`'s committed rocprofv3 kernel trace (the same
    profiles/traffic.json entry: sum over the timer's kernels of avg_ms x launches / the timer's launches), or None.
    Reported beside the live HIP-event figure: the two come from different boxes and runs (box-to-box spread)."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        wl = json.load(f).get("workloads", {}).get(workload)
    if not wl or timer not in wl.get("timers", {}):
        return None
    t = wl["timers"][timer]
    tot = sum(wl["kernels"][k]["avg_ms"] * wl["kernels"][k]["launches"] for k in t.get("kernels", [])
              if k in wl.get("kernels", {}) and "avg_ms" in wl["kernels"][k])
    n = t.get("launches") or 0
    return tot / n if tot > 0 and n > 0 else None


def _sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def timed_steps(step, steps, warmup, world, device, rank, label="", on_start=None, on_step=None):
    """The contract's timing: `warmup` untimed steps, then exactly `steps` timed steps bracketed by a barrier and a
    device synchronize on both sides; returns (max elapsed seconds over ranks, last step's return value).
    Device-agnostic (CUDA/RCCL on the GPU box; CPU/gloo in the multi-process rehearsal test)."""
    for i in range(warmup):
        tw = time.perf_counter()
        step()
        _sync(device)
        if rank == 0 and label:
            print(f"[bench] {label} warmup step {i}: {time.perf_counter() - tw:.2f} s", file=sys.stderr, flush=True)
    _sync(device)
    if world > 1:
        dist.barrier()
    _sync(device)
    if on_start is not None:
        on_start()
    t0 = time.perf_counter()
    out = None
    for i in range(steps):
        if on_step is not None:
            on_step(i)
        out = step()
    _sync(device)
    if world > 1:
        dist.barrier()
    _sync(device)
    elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return t.item(), out


GRAPHED = ("swin_p2_128", "swin_mamba_p2_128", "swin_hyena_p2_128", "vit_p4_512")


def write_dump(dump_dir, loss):
    """--dump-outputs: what the timed step hands its caller, the loss tensor, as float32 `loss.npy` of shape (1,)."""
    import numpy as np
    os.makedirs(dump_dir, exist_ok=True)
    np.save(os.path.join(dump_dir, "loss.npy"), loss.detach().float().cpu().numpy().reshape(1))


def run_workload(workload, batch, steps, warmup, rank, world, device, kernel_timer=True, cfg_extra=(),
                 ckpt_blocks=None, use_graph=None, full=False, dump_dir=None):
    """Build the workload's model, run `warmup` untimed and `steps` timed training steps (barrier + sync on both
    sides, max over ranks). Returns the bench dict on rank 0 (None elsewhere); frees the model. `full` adds the
    per-kernel figures (probe step, events in the last timed step, two breakdown steps after the timed region, the
    graphed workloads' eager re-timing); `dump_dir` stores the last timed step's loss (rank 0)."""
    kernel_timer = kernel_timer and full
    if workload in ("swin_p2_128", "vit_mamba_p2_256", "swin_mamba_p2_128", "swin_hyena_p2_128"):
        # any 3-D conv left on MIOpen (none in these heads today): heuristic solver instead of a minutes-long find
        os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    cfg = lconfig.parse_config(WORKLOADS[workload] + ["--batch_size", str(batch)] + list(cfg_extra))
    if device.type == "cuda":
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(device)
    torch.manual_seed(0)
    if workload == "rehearsal":
        model = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.GELU(), torch.nn.Linear(256, 64)).to(device)
    else:
        model = EncoderDecoderModel(cfg, cfg.encoder_name, cfg.decoder_name, cfg.no_in_channel,
                                    cfg.no_out_channel).to(device)
    if use_graph is None:   # host-bound workloads (many small ops per step); LCI_GRAPH=0/1 overrides
        env = os.environ.get("LCI_GRAPH", "")
        use_graph = env == "1" or (env != "0" and workload in GRAPHED)
    # C5: the first 10 of 12 encoder blocks re-run their forward in the backward (~24 GB of saved activations per
    # un-checkpointed block at 2^21 tokens; 10 -> 230 GB peak of 288, 12 -> 182 GB; 1770 vs 1819 ms per step)
    ckpt = ckpt_blocks if ckpt_blocks is not None else (10 if workload == "vit_mamba_p2_256" else 0)
    if ckpt:
        model.encoder.checkpoint_blocks = ckpt   # ~35 GB of saved activations per block at 2^21 tokens
    trainer = TrainStep(model, cfg, device, ddp=world > 1)
    if workload == "rehearsal":
        g = torch.Generator().manual_seed(1234 + rank)
        L = 4096
        x, y = torch.randn(batch, L, 64, generator=g).to(device), torch.randn(batch, L, 64, generator=g).to(device)
    else:
        x, y = synthetic_batch(cfg, batch, device, seed=1234 + rank)
        L = (model.encoder.patch_embedding.n_patches if hasattr(model.encoder, "patch_embedding")
             else cfg.time * cfg.height * cfg.width // 8)

    def on_timed_start():
        kernels.KernelTimer.reset()
        kernels.KernelTimer.enabled = kernel_timer

    graphed = use_graph and world == 1 and device.type == "cuda"
    if graphed:
        # the whole step as one HIP graph replay (trainer.GraphedStep): host-side op overhead paid once; the
        # per-kernel breakdown then comes from eager steps after the timed region (same kernels)
        try:
            gstep = GraphedStep(trainer, x, y)
        except Exception as e:   # never lose the line to the capture: time the eager step instead
            print(f"[bench] {workload}: graph capture failed ({type(e).__name__}: {e}); eager steps",
                  file=sys.stderr, flush=True)
            graphed = False
    eager_ms = None
    dom_timed, ksum_timed = None, {}
    if graphed:
        elapsed, loss = timed_steps(gstep.step, steps, warmup, world, device, rank, label=workload)
        loss = loss.detach().clone()   # the replay's loss lives in the graph's memory pool, released below
        if dump_dir is not None and rank == 0:
            write_dump(dump_dir, loss)
        del gstep
        torch.cuda.synchronize(device)
        nk = steps
        if full:
            # the same step eager (N > 1 runs are eager: DDP's all-reduce hooks are not captured), so a scaling ratio
            # against this N = 1 line can compare like with like
            e_el, _ = timed_steps(lambda: trainer.step(x, y), min(steps, 5), 1, world, device, rank)
            eager_ms = round(1000.0 * e_el / min(steps, 5), 2)
            kernels.KernelTimer.reset()
            kernels.KernelTimer.enabled = kernel_timer
            for _ in range(2):
                # a ~0.1 s device-side spin first, so the host has queued the whole step before the GPU reaches it:
                # the per-launch events then bracket kernel time only, not the GPU idling while the host enqueues
                # (these steps are host-paced when eager; without it small kernels read 2-3x their rocprofv3 durations)
                torch.cuda._sleep(250_000_000)
                trainer.step(x, y)
            nk = 2
    else:
        # One untimed probe step with every liblci launch timed picks the dominant kernel; inside the timed region
        # only that kernel's launches of the last step carry events (an event pair on each of the ~400 launches of
        # every step cost up to 22 ms of host time per step where the step is host-paced: C4 292 vs 270 ms), and
        # the per-kernel breakdown comes from two eager steps after the timed region, as in the graphed path.
        if kernel_timer and device.type == "cuda":
            kernels.KernelTimer.reset()
            kernels.KernelTimer.enabled = True
            torch.cuda._sleep(250_000_000)
            trainer.step(x, y)
            kernels.KernelTimer.enabled = False
            probe = kernels.KernelTimer.summary()
            kernels.KernelTimer.reset()
            cands = [n for n in probe if probe[n]["work_per_call"]]
            if cands:
                dom_timed = max(cands, key=lambda n: probe[n]["total_ms"])
                kernels.KernelTimer.only = {dom_timed}
        on_step = None
        if kernels.KernelTimer.only is not None:
            def on_step(i):   # the dominant kernel's launches of the last timed step (every shape it runs at)
                kernels.KernelTimer.enabled = kernel_timer and i == steps - 1
        elapsed, loss = timed_steps(lambda: trainer.step(x, y), steps, warmup, world, device, rank,
                                    label=workload, on_start=on_timed_start, on_step=on_step)
        if dump_dir is not None and rank == 0:
            write_dump(dump_dir, loss)
        nk = steps
        if kernels.KernelTimer.only is not None:
            kernels.KernelTimer.enabled = False
            kernels.KernelTimer.only = None
            ksum_timed = kernels.KernelTimer.summary()
            kernels.KernelTimer.reset()
            kernels.KernelTimer.enabled = True
            for _ in range(2):
                torch.cuda._sleep(250_000_000)
                trainer.step(x, y)
            nk = 2
    kernels.KernelTimer.enabled = False
    ksum = kernels.KernelTimer.summary() if device.type == "cuda" else {}
    kernels.KernelTimer.reset()
    loss_v = float(loss.item())
    enc = getattr(model, "encoder", None)
    model_blocks = list(enc.blocks) if hasattr(enc, "blocks") else []
    peak_mem = torch.cuda.max_memory_allocated(device) if device.type == "cuda" else 0
    del trainer, model, x, y, loss
    if device.type == "cuda":
        torch.cuda.empty_cache()
    if rank != 0:
        return None

    ms = 1000.0 * elapsed / steps
    tokens = world * batch * L * steps
    kern = {}
    for name, d in ksum.items():
        kern[name] = {"calls_per_step": d["calls"] / nk, "avg_ms": round(d["avg_ms"], 3),
                      "ms_per_step": round(d["total_ms"] / nk, 2)}
        if d["work_per_call"]:
            b, pu = ROOF.get(name, ("mfma", 1.0))
            rate = d["work_per_call"] * pu / (d["avg_ms"] * 1e-3)
            kern[name]["tflops" if b.startswith("mfma") else "gbs"] = round(rate / (1e12 if b.startswith("mfma")
                                                                                   else 1e9), 1)
    roof = None
    if ksum:
        dom = max((n for n in ksum if ksum[n]["work_per_call"]), key=lambda n: ksum[n]["total_ms"])
        dd = ksum[dom]
        if dom_timed in ksum_timed:   # the dominant kernel's launches inside the timed region
            dom, dd = dom_timed, ksum_timed[dom_timed]
        bound, per_unit = ROOF.get(dom, ("mfma", 1.0))
        work = dd["work_per_call"] * per_unit
        if bound.startswith("mfma"):
            peak = MFMA_F32_PEAK_TFLOPS if bound == "mfma_f32" else MFMA_BF16_PEAK_TFLOPS
            ach, unit = work / (dd["avg_ms"] * 1e-3) / 1e12, "TFLOP/s"
            bound = "mfma"
        else:
            ach, peak, unit = work / (dd["avg_ms"] * 1e-3) / 1e9, HBM_PEAK_GBS, "GB/s"
        traffic, tsrc = profiled_traffic(dom, workload)
        roof = {"kernel": dom, "bound": bound, "achieved": round(ach, 1), "peak": peak,
                "unit": unit, "frac": round(ach / peak, 4),
                "traffic": traffic, "traffic_source": tsrc,
                "work_per_launch": work, "avg_launch_ms": round(dd["avg_ms"], 3)}
        pms = profiled_launch_ms(dom, workload)
        if pms:   # the committed rocprofv3 trace's figure for the same kernel: the frac spread across boxes / runs
            roof["profile_avg_launch_ms"] = round(pms, 3)
            roof["profile_frac"] = round(work / (pms * 1e-3) / (1e12 if unit == "TFLOP/s" else 1e9) / peak, 4)
    return {
        "metric": WORKLOAD_NAMES[workload][0],
        "value": round(tokens / elapsed, 1), "unit": "image-tokens/s", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": round(ms, 2), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic U[0,1) images, random-init weights",
        "rccl_world": world if dist.is_initialized() and dist.get_backend() == "nccl" else None,
        "dist_backend": dist.get_backend() if dist.is_initialized() else None,
        "config": {"workload": WORKLOAD_NAMES[workload][1],
                   "global_batch": world * batch, "seq_len": L, "parallelism": f"ddp{world}",
                   "per_gpu_batch": batch, "optimizer": cfg.optim_type, "loss": cfg.loss_func,
                   "activation_checkpointing": f"first {ckpt} of {len(model_blocks)} encoder blocks" if ckpt
                   else "none",
                   "hip_graph": bool(graphed), "eager_ms_per_step": eager_ms},
        "peak_memory_gb": round(peak_mem / 2 ** 30, 1),
        "roofline": roof,
        "kernels": kern,
        "loss": round(loss_v, 5),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="images per GPU (default 2; 1 for the 3-D configs)")
    ap.add_argument("--workload", default="vit_p2_512", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="also report roofline, per-kernel breakdown, eager re-timing of the graphed workloads, the "
                         "secondary Swin 128^3 line and the CPU baseline (extra steps and runs after the timed region)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's output (the loss it returns; rank 0) as float32 DIR/loss.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the Swin 128^3 line that the default (ViT 512^2) run also reports")
    ap.add_argument("--cpu-budget", type=float, default=20.0)
    ap.add_argument("--ckpt-blocks", type=int, default=None,
                    help="checkpoint the first K encoder blocks (default: 10 of 12 for vit_mamba_p2_256, else none)")
    ap.add_argument("--no-kernel-timer", action="store_true",
                    help="no per-launch HIP events (rocprofv3 PMC passes); the line then carries no roofline")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N`: start the N ranks (one process per GPU) as a child torch.distributed.run, before
        # this process makes any GPU call, and exit with its code (never exec from here)
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
        print(f"[bench] launching {args.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
        sys.exit(subprocess.call(cmd))

    if args.batch is None:
        # 2 images per GPU, except the 3-D ViTUNETR / SwinUNETR configs (1 volume); the UperNet heads' BatchNorm needs
        # 2 samples in training (the reference duplicates a batch of 1, trainer_base.py:160-164; run_abct.sh uses 2)
        args.batch = 1 if args.workload in ("swin_p2_128", "vit_mamba_p2_256") else 2
    rank, local, world = init_distributed()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the process group has {world} ranks")
    if world > 1:
        assert dist.get_world_size() == args.gpus
    if args.workload == "rehearsal" or not torch.cuda.is_available():
        device = torch.device("cpu")
        tuned = False
    else:
        device = torch.device("cuda", local % torch.cuda.device_count())   # % : gloo rehearsals on one GPU
        torch.cuda.set_device(device)
        tuned = use_tuned_gemms()
    res = run_workload(args.workload, args.batch, args.steps, args.warmup, rank, world, device,
                       kernel_timer=not args.no_kernel_timer, ckpt_blocks=args.ckpt_blocks, full=args.full,
                       dump_dir=args.dump_outputs)
    if args.full and args.workload == "vit_p2_512" and not args.no_secondary:
        # north_star also asks for tokens/s on 128^3 patch-2 volumes (BASELINE configs[2], Swin + SwinUNETR):
        # same DDP harness, 1 volume per GPU, same steps (at most 10), reported under "secondary"
        try:
            sec = run_workload("swin_p2_128", 1, min(args.steps, 10), 2, rank, world, device,
                               kernel_timer=not args.no_kernel_timer, full=True)
        except Exception as e:   # never lose the headline line to the secondary workload
            sec = {"error": f"{type(e).__name__}: {e}"}
        if rank == 0:
            keep = ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "config", "roofline", "kernels")
            res["secondary"] = {"swin_p2_128": {k: sec[k] for k in keep if k in sec} if "error" not in sec else sec}
    if rank == 0:
        res["config"]["tuned_gemms"] = tuned
        if args.full and world == 1 and not args.no_cpu_baseline and args.workload == "vit_p2_512":
            res["cpu_baseline"] = cpu_baseline(args.cpu_budget)
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
