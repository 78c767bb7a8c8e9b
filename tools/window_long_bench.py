#!/usr/bin/env python
"""Large-window attention (csrc/window_long.hip) against the torch composite, at the two shapes beyond the recipes.

    python tools/window_long_bench.py [--out profiles/window_long_bench.txt] [--rounds 3] [--replays 3] [--only NAME]

Shapes (stage 1 of Swin-tiny, patch 2: C = 96, 3 heads of 32, shifted windows, with a qkv bias):
  s1_1024sq_w32   1024^2 image, B = 4: grid 512 x 512, windows 32 x 32 (N = 1024), shift 16 -> 1024 windows
  s1_128cu_w16    128^3 volume, B = 1: grid 64^3, windows 16^3 (N = 4096), shift 8 -> 64 windows
  resident_768    128^3 volume, B = 1: grid 64^3, windows 8 x 8 x 12 (N = 768), shift 4, 4, 6: the resident kernels of
                  csrc/window.hip at their largest window, for scale (no composite)

Kernel side: kernels.window_attention_grid_long (window_attention_grid for resident_768) through autograd, forward
alone and forward + backward (gradients of qkv, the qkv bias and the table), each captured once into a HIP graph and
replayed. Comparison: the oracle's composite (oracle.window: pad, roll, partition, (q scale) k^T + table[index] + mask,
softmax, @ v, reverse, roll, crop) under bf16 autocast on the GPU with the mask built once outside the timed region,
run eagerly under HIP events (tens of milliseconds per call: launch gaps do not matter). The two sides alternate:
--rounds times (--replays graph replays, then one composite call); reported: best and median ms per call, TFLOP/s of
the kernel side from the algorithm's 4 N^2 32 FLOP per (window, head) forward and 3 x that forward + backward, and
composite / kernel. A GPU is required.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from long_context_biomedical_imaging_amd import kernels  # noqa: E402
from oracle import window as ow  # noqa: E402

BF16 = torch.bfloat16
H, C = 3, 96
SHAPES = {   # name -> (B, grid, window, shift, long path)
    "s1_1024sq_w32": (4, (512, 512), (32, 32), (16, 16), True),
    "s1_128cu_w16": (1, (64, 64, 64), (16, 16, 16), (8, 8, 8), True),
    "resident_768": (1, (64, 64, 64), (8, 8, 12), (4, 4, 6), False),
}


def gpu_mask(dims, ws, ss):
    """oracle.window.compute_mask evaluated on the GPU (the same region ids, partition and -100 fill)."""
    img = torch.from_numpy(ow.region_ids(dims, ws, ss)).float().cuda()[None, ..., None]
    mw = ow.window_partition(img, ws).squeeze(-1)
    am = mw.unsqueeze(1) - mw.unsqueeze(2)
    return torch.where(am != 0, -100.0, 0.0)


def composite(qkv, bias, table, idx, mask, ws, ss, scale):
    S = list(qkv.shape[1:-1])
    win, dims = ow.grid_to_windows(qkv, bias, ws, ss)
    bw, n, c3 = win.shape
    t = win.reshape(bw, n, 3, H, c3 // (3 * H)).permute(2, 0, 3, 1, 4)
    rpb = table[idx].reshape(n, n, H).permute(2, 0, 1)
    out = ow.window_attention_core(t[0], t[1], t[2], rpb, mask, scale)
    return ow.windows_to_grid(out.transpose(1, 2).reshape(bw, n, c3 // 3), ws, ss, dims, S)


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run_shape(name, rounds, replays):
    B, S, ws, ss, long_path = SHAPES[name]
    n = math.prod(ws)
    g = torch.Generator(device="cuda").manual_seed(n)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")   # noqa: E731
    qkv = rn(B, *S, 3 * C).to(BF16).requires_grad_(True)
    bias = (0.5 * rn(3 * C)).requires_grad_(True)
    cot = rn(B, *S, C).to(BF16)
    scale = 32 ** -0.5
    nwin = B * math.prod(-(-s // w) for s, w in zip(S, ws))
    flop = 4.0 * nwin * H * n * n * 32
    if long_path:
        table = (0.5 * rn(math.prod(2 * w - 1 for w in ws), H)).requires_grad_(True)
        op = lambda: kernels.window_attention_grid_long(qkv, bias, table, H, scale, ws, ss, ws)   # noqa: E731
        leaves = (qkv, bias, table)
    else:
        rpb = (0.5 * rn(H, n, n)).requires_grad_(True)
        op = lambda: kernels.window_attention_grid(qkv, bias, rpb, H, scale, ws, ss)   # noqa: E731
        leaves = (qkv, bias, rpb)

    def k_fwd():
        with torch.no_grad():
            return op()

    def k_fb():
        for t in leaves:
            t.grad = None
        op().backward(cot)

    sides = {"kernel_fwd": (graph_of(k_fwd).replay, replays), "kernel_fwd_bwd": (graph_of(k_fb).replay, replays)}
    if long_path:
        idx = torch.from_numpy(ow.relative_position_index(ws)[:n, :n].copy()).cuda().reshape(-1)
        mask = gpu_mask(ow.padded_dims(S, ws), ws, ss)
        q32 = qkv.detach().float().requires_grad_(True)
        b32, t32 = bias.detach().clone().requires_grad_(True), table.detach().clone().requires_grad_(True)

        def c_fwd():
            with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
                return composite(q32, b32, t32, idx, mask, ws, ss, scale)

        def c_fb():
            for t in (q32, b32, t32):
                t.grad = None
            with torch.autocast("cuda", dtype=BF16):
                out = composite(q32, b32, t32, idx, mask, ws, ss, scale)
            out.backward(cot.to(out.dtype))

        for fn in (c_fwd, c_fb):   # warm-up: code objects, algorithm picks, the allocator's blocks
            fn()
        torch.cuda.synchronize()
        sides.update(composite_fwd=(c_fwd, 1), composite_fwd_bwd=(c_fb, 1))
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, (fn, reps) in sides.items():   # alternate the sides
            ms[k].append(timed(fn, reps))
    d = dict(shape=name, B=B, grid=list(S), window=list(ws), shift=list(ss), windows=nwin, N=n, heads=H)
    for k, v in ms.items():
        d[k + "_ms"] = round(min(v), 3)
        d[k + "_ms_median"] = round(statistics.median(v), 3)
    d["kernel_fwd_tflops"] = round(flop / min(ms["kernel_fwd"]) * 1e-9, 1)
    d["kernel_fwd_bwd_tflops"] = round(3 * flop / min(ms["kernel_fwd_bwd"]) * 1e-9, 1)
    if long_path:
        d["composite_over_kernel_fwd"] = round(min(ms["composite_fwd"]) / min(ms["kernel_fwd"]), 2)
        d["composite_over_kernel_fwd_bwd"] = round(min(ms["composite_fwd_bwd"]) / min(ms["kernel_fwd_bwd"]), 2)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_long_bench.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--only", action="append", default=None, choices=list(SHAPES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_long_bench: needs a GPU (the kernels have no CPU path)")
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/window_long_bench.py  (one {torch.cuda.get_device_name(0)}, {arch}; kernel side: HIP-graph "
             f"replays, composite: eager bf16 autocast, alternated, {a.rounds} rounds x {a.replays} replays; ms per call)"]
    print(lines[0], flush=True)
    for name in a.only or list(SHAPES):
        lines.append(json.dumps(run_shape(name, a.rounds, a.replays)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
