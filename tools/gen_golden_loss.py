#!/usr/bin/env python3
"""Writes tests/golden/enhance_loss.npz: the reference's CombinationEnhance loss on seeded inputs (CPU, f32).

    python tools/gen_golden_loss.py [--reference /root/reference]

The reference's loss module (loss/loss_functions/enhancement_losses.py) is imported from the reference checkout and
run as it is; only data is stored:
  window{k}                 the three conv3d weights (kT, kH, kW) as GaussianDeriv3D_Loss builds them, f32
  {case}_outputs, _targets  seeded inputs; outputs are rounded through bf16 so one fixture serves both dtypes
  {case}_components         (mse, charbonnier, gaussian3D), f32
  {case}_loss               Combined_Loss(["mse", "charbonnier", "gaussian3D"], [1, 1, 1]) of them
  {case}_grad               d loss / d outputs
for the cases a = (2, 1, 6, 19, 23) and b = (1, 1, 1, 8, 8).
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"a": (2, 1, 6, 19, 23), "b": (1, 1, 1, 8, 8)}
SEED = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "enhance_loss.npz"))
    a = ap.parse_args()
    path = os.path.join(a.reference, "loss", "loss_functions", "enhancement_losses.py")
    spec = importlib.util.spec_from_file_location("ref_enhancement_losses", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    names = ["mse", "charbonnier", "gaussian3D"]
    combined = ref.Combined_Loss(names, [1, 1, 1])
    data = {}
    gauss = [f for f, _ in combined.losses if isinstance(f, ref.GaussianDeriv3D_Loss)][0]
    for k, w in enumerate(gauss.kernels):
        data[f"window{k}"] = w[0, 0].contiguous().numpy().astype(np.float32)
    g = torch.Generator().manual_seed(SEED)
    for case, shape in CASES.items():
        outputs = torch.randn(*shape, generator=g).to(torch.bfloat16).to(torch.float32)
        targets = torch.randn(*shape, generator=g)
        o = outputs.clone().requires_grad_(True)
        loss = combined(o, targets)
        loss.backward()
        comps = [float(ref.Combined_Loss([n], [1])(outputs, targets)) for n in names]
        data[f"{case}_outputs"] = outputs.numpy()
        data[f"{case}_targets"] = targets.numpy()
        data[f"{case}_components"] = np.asarray(comps, dtype=np.float32)
        data[f"{case}_loss"] = np.float32(loss.item())
        data[f"{case}_grad"] = o.grad.numpy()
    np.savez_compressed(a.out, **data)
    print(a.out, os.path.getsize(a.out), "bytes", {k: v.shape for k, v in data.items()})


if __name__ == "__main__":
    main()
