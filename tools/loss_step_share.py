#!/usr/bin/env python3
"""What the CombinationEnhance loss costs inside a C3 training step.

    python tools/loss_step_share.py [--steps 10] [--warmup 3]

bench.py's swin_p2_128 model (Swin-tiny + SwinUNETR, 128^3, patch 2, one volume per GPU) as an enhancement model
(--task_type enhance, one output channel), stepped through TrainStep captured as a GraphedStep (the mode bench.py runs
C3 in) once with --loss_func MSE and once with --loss_func CombinationEnhance; same seed, same synthetic batch. One
JSON line per loss (step ms) and one with the difference as a share of the step. bench.py's own swin_p2_128 line (the
seg task, CrossEntropy) is the step this is to be read against.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from long_context_biomedical_imaging_amd import config as lconfig  # noqa: E402
from long_context_biomedical_imaging_amd.model_base import EncoderDecoderModel  # noqa: E402
from long_context_biomedical_imaging_amd.trainer import GraphedStep, TrainStep, synthetic_batch  # noqa: E402


def step_ms(loss_func, steps, warmup, device):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    args = list(bench.WORKLOADS["swin_p2_128"])
    args[args.index("--task_type") + 1] = "enhance"
    args[args.index("--no_out_channel") + 1] = "1"
    cfg = lconfig.parse_config(args + ["--batch_size", "1", "--loss_func", loss_func])
    torch.manual_seed(0)
    model = EncoderDecoderModel(cfg, cfg.encoder_name, cfg.decoder_name, cfg.no_in_channel, cfg.no_out_channel).to(device)
    trainer = TrainStep(model, cfg, device, ddp=False)
    x, y = synthetic_batch(cfg, 1, device, seed=1234)
    g = GraphedStep(trainer, x, y)
    for _ in range(warmup):
        g.step()
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = g.step()
    e1.record()
    torch.cuda.synchronize(device)
    ms = e0.elapsed_time(e1) / steps
    out = {"loss_func": loss_func, "step_ms": round(ms, 3), "loss": round(float(loss), 6), "steps": steps,
           "model": "swin_p2_128 as enhance, 1 output channel, graphed"}
    del g, trainer, model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    res = {}
    for lf in ("MSE", "CombinationEnhance", "MSE", "CombinationEnhance"):     # alternated: the spread shows
        r = step_ms(lf, a.steps, a.warmup, device)
        print(json.dumps(r), flush=True)
        res.setdefault(lf, []).append(r["step_ms"])
    mse, ce = min(res["MSE"]), min(res["CombinationEnhance"])
    print(json.dumps({"mse_step_ms": mse, "combination_enhance_step_ms": ce, "extra_ms": round(ce - mse, 3),
                      "extra_share_of_step": round((ce - mse) / ce, 4)}), flush=True)


if __name__ == "__main__":
    main()
