"""Micro-benchmark of liblci flash attention fwd / bwd (HIP events, random N(0,1) bf16 data)."""
import argparse
import json
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from long_context_biomedical_imaging_amd import kernels  # noqa: E402


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[16384, 65536])
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--H", type=int, default=6)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--fwd-variant", type=int, nargs="+", choices=[0, 1], default=None,
                    help="time the forward alone with the kernel forced (0 = 64 queries per wave, 1 = 128); several "
                         "values alternate in one process, --rounds times each")
    ap.add_argument("--dq-variant", type=int, nargs="+", choices=[0, 1], default=None,
                    help="time the backward's dQ launch(es) alone with the kernel forced (0 = 64 queries per wave, "
                         "1 = 128 + its fallback launch); several values alternate in one process, --rounds times each")
    ap.add_argument("--dkdv-wide", action="store_true",
                    help="time the backward's dK/dV launch(es) alone, alternating W = 0 (64 keys per wave alone) and "
                         "W = lci_attn_bwd_dkdv_pick (96 keys per wave on keys [0, 384 W)) in one process, --rounds "
                         "times each; where the pick is 0 only W = 0 is timed")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    for L in a.L:
        qkv = torch.randn(a.B, L, 3 * a.H * 64, device="cuda").to(torch.bfloat16)
        if a.dkdv_wide:
            f = 6.0 * a.B * a.H * L * L * 64
            dout = torch.randn(a.B, L, a.H * 64, device="cuda").to(torch.bfloat16)
            out, lse = kernels.attn_fwd(qkv, a.H, 0.125)
            lib = kernels._lib.load()
            ws = torch.empty(lib.lci_attn_bwd_ws_bytes(a.B, a.H, L) // 4, device="cuda", dtype=torch.int32)
            n_cu = torch.cuda.get_device_properties(qkv.device).multi_processor_count
            pick = lib.lci_attn_bwd_dkdv_pick(a.B, L, a.H, n_cu)
            dqkv = torch.zeros_like(qkv)
            run = lambda w, stage: kernels.attn_bwd_variant2(qkv, out, dout, lse, a.H, 0.125, -1, w, stage, ws, dqkv)  # noqa: E731
            run(0, 0)                 # the row constants, once
            ws_ = [0, pick] if pick else [0]
            ref = None
            for w in ws_:             # warm both before the first timed round; the split changes no bit
                run(w, 1)
                got = dqkv.clone()
                ref = got if ref is None else ref
                assert torch.equal(got, ref), "dK / dV differ between the splits"
            for rnd in range(a.rounds):
                for w in ws_:
                    t = timeit(lambda: run(w, 1), a.iters)
                    print(json.dumps({"L": L, "B": a.B, "H": a.H, "n_cu": n_cu, "round": rnd, "dkdv_wide_wgs": w,
                                      "dkdv_ms": round(t, 3), "dkdv_tflops_alg": round(f / t / 1e9, 1)}), flush=True)
            continue
        if a.dq_variant is not None:
            f = 2.0 * a.B * a.H * L * L * 64
            dout = torch.randn(a.B, L, a.H * 64, device="cuda").to(torch.bfloat16)
            out, lse = kernels.attn_fwd(qkv, a.H, 0.125)
            ws = torch.empty(kernels._lib.load().lci_attn_bwd_ws_bytes(a.B, a.H, L) // 4, device="cuda",
                             dtype=torch.int32)
            dqkv = torch.empty_like(qkv)
            run = lambda v, stage: kernels.attn_bwd_variant(qkv, out, dout, lse, a.H, 0.125, v, stage, ws, dqkv)  # noqa: E731
            run(0, 0)                 # the row constants, once
            for v in a.dq_variant:    # warm both before the first timed round
                _, flags = run(v, 2)
            for rnd in range(a.rounds):
                for v in a.dq_variant:
                    t = timeit(lambda: run(v, 2), a.iters)
                    print(json.dumps({"L": L, "B": a.B, "H": a.H, "round": rnd, "dq_variant": v, "dq_ms": round(t, 3),
                                      "dq_tflops_alg": round(f / t / 1e9, 1),
                                      "flagged": int(flags.sum().item()) if v == 1 else 0}), flush=True)
            continue
        if a.fwd_variant is not None:
            f = 4.0 * a.B * a.H * L * L * 64
            for v in a.fwd_variant:   # warm both before the first timed round
                kernels.attn_fwd_variant(qkv, a.H, 0.125, v)
            for rnd in range(a.rounds):
                for v in a.fwd_variant:
                    tf = timeit(lambda: kernels.attn_fwd_variant(qkv, a.H, 0.125, v), a.iters)
                    print(json.dumps({"L": L, "B": a.B, "H": a.H, "round": rnd, "fwd_variant": v,
                                      "fwd_ms": round(tf, 3), "fwd_tflops": round(f / tf / 1e9, 1)}), flush=True)
            continue
        dout = torch.randn(a.B, L, a.H * 64, device="cuda").to(torch.bfloat16)
        out, lse = kernels.attn_fwd(qkv, a.H, 0.125)
        tf = timeit(lambda: kernels.attn_fwd(qkv, a.H, 0.125), a.iters)
        tb = timeit(lambda: kernels.attn_bwd(qkv, out, dout, lse, a.H, 0.125), a.iters)
        f = 4.0 * a.B * a.H * L * L * 64
        print(json.dumps({"L": L, "B": a.B, "H": a.H, "fwd_ms": round(tf, 3), "bwd_ms": round(tb, 3),
                          "fwd_tflops": round(f / tf / 1e9, 1), "bwd_tflops_alg": round(2 * f / tb / 1e9, 1)}),
              flush=True)


if __name__ == "__main__":
    main()
