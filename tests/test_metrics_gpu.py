"""Task metrics on the GPU (csrc/metrics.hip through kernels.enhance_metrics / kernels.seg_f1, metrics.TaskMetrics,
trainer.EvalStep, TrainStep.metrics) against the float64 restatements of tests/test_metrics_cpu.py.

SSIM / PSNR bound per case: 4 x e_ref, where e_ref is the error of the same formulas evaluated by torch in float32 on
the CPU on the same inputs against float64, with floors of 1e-5 (ssim, absolute) and 1e-5 dB (psnr). F1 is counted in
integers (exact) and divided in f64: 1e-6 of float64.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_metrics_cpu import enhance_metrics_ref, f1_counts, f1_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 1, 11, 11), (2, 1, 1, 19, 23), (1, 2, 1, 37, 70), (2, 1, 11, 11, 11), (1, 1, 13, 19, 23),
          (1, 1, 17, 66, 130)]
KINDS = ("unit", "offset")
CASES = [(s, k, torch.float32) for s in SHAPES for k in KINDS] + \
        [(s, k, torch.bfloat16) for s in SHAPES[-2:] for k in KINDS]
SSIM_FLOOR, PSNR_FLOOR = 1e-5, 1e-5


def _dev():
    return torch.device("cuda", 0)


def _inputs(shape, kind, dtype=torch.float32, seed=37):
    """unit: targets U[0, 1), outputs = targets + 0.1 N(0, 1). offset: targets 1000 + 200 N(0, 1), outputs = targets +
    20 N(0, 1) — a large mean against the spread, which exercises the E[x^2] - mu^2 cancellation."""
    g = torch.Generator().manual_seed(seed)
    if kind == "unit":
        t = torch.rand(shape, generator=g)
        p = t + 0.1 * torch.randn(shape, generator=g)
    else:
        t = 1000 + 200 * torch.randn(shape, generator=g)
        p = t + 20 * torch.randn(shape, generator=g)
    return p.to(dtype), t


_REF = {}


def _reference(shape, kind, dtype):
    """(ssim, psnr) in float64 and in float32 on the CPU, computed once per case."""
    key = (shape, kind, dtype)
    if key not in _REF:
        p, t = _inputs(shape, kind, dtype)
        _REF[key] = (enhance_metrics_ref(p, t), enhance_metrics_ref(p, t, torch.float32))
    return _REF[key]


def test_shapes_cover_the_tile():
    """In 2-D and in 3-D some shape's interior exceeds the tile on every windowed axis and is no multiple of it."""
    from long_context_biomedical_imaging_amd import kernels
    tile = kernels.SSIM_TILE
    assert len(tile) == 3

    def covers(shape):
        ext = shape[3:] if shape[2] == 1 else shape[2:]
        tl = tile[1:] if shape[2] == 1 else tile
        return all(n - 10 > k and (n - 10) % k for n, k in zip(ext, tl))

    assert any(covers(s) for s in SHAPES if s[2] == 1)
    assert any(covers(s) for s in SHAPES if s[2] != 1)


@pytest.mark.parametrize("shape,kind,dtype", CASES, ids=lambda v: str(v).replace(" ", "").replace("torch.", ""))
def test_enhance_metrics_against_float64(shape, kind, dtype):
    """e_ref (float32 on the CPU against float64) per case, ssim absolute | psnr dB:

      shape              unit f32            offset f32          unit bf16 outputs   offset bf16 outputs
      (2,1,1,11,11)      1.3e-07 | 8.0e-07   3.6e-07 | 8.4e-07
      (2,1,1,19,23)      3.5e-08 | 2.4e-07   2.8e-08 | 2.8e-07
      (1,2,1,37,70)      2.4e-08 | 6.6e-07   2.0e-08 | 2.2e-06
      (2,1,11,11,11)     2.5e-07 | 7.4e-07   2.8e-08 | 1.1e-06
      (1,1,13,19,23)     1.3e-07 | 6.8e-07   1.2e-07 | 1.6e-06   3.4e-08 | 1.5e-07   1.8e-07 | 7.1e-07
      (1,1,17,66,130)    3.7e-08 | 1.9e-07   3.4e-09 | 1.8e-06   9.3e-09 | 6.9e-07   3.8e-09 | 1.7e-06

    Four times these stay below the floors, so every case is held to 1e-5 (ssim) and 1e-5 dB (psnr)."""
    from long_context_biomedical_imaging_amd import kernels
    p, t = _inputs(shape, kind, dtype)
    (ssim64, psnr64), (ssim32, psnr32) = _reference(shape, kind, dtype)
    got = kernels.enhance_metrics(p.to(_dev()), t.to(_dev())).cpu()
    assert got.dtype == torch.float32 and got.shape == (2,)
    e_ssim, e_psnr = abs(got[0].item() - ssim64), abs(got[1].item() - psnr64)
    b_ssim, b_psnr = max(4 * abs(ssim32 - ssim64), SSIM_FLOOR), max(4 * abs(psnr32 - psnr64), PSNR_FLOOR)
    print(f"{shape} {kind} {dtype}: ssim {got[0].item():.8f} err {e_ssim:.2e} (e_ref {abs(ssim32 - ssim64):.2e}), "
          f"psnr {got[1].item():.6f} err {e_psnr:.2e} (e_ref {abs(psnr32 - psnr64):.2e})")
    assert e_ssim <= b_ssim, (got[0].item(), ssim64, b_ssim)
    assert e_psnr <= b_psnr, (got[1].item(), psnr64, b_psnr)


def test_enhance_metrics_mixed_dtypes():
    """bf16 targets with f32 outputs, and both bf16: the values of the same numbers held in f32."""
    from long_context_biomedical_imaging_amd import kernels
    p, t = _inputs((1, 1, 13, 19, 23), "unit")
    pb, tb = p.to(torch.bfloat16).to(_dev()), t.to(torch.bfloat16).to(_dev())
    want = kernels.enhance_metrics(pb.float(), tb.float())
    assert torch.equal(kernels.enhance_metrics(pb, tb), want)
    assert torch.equal(kernels.enhance_metrics(pb.float(), tb), want)
    assert torch.equal(kernels.enhance_metrics(pb, tb.float()), want)


def test_enhance_metrics_identity_noncontiguous_repeatable_nan():
    from long_context_biomedical_imaging_amd import kernels
    dev = _dev()
    for shape in ((2, 1, 1, 19, 23), (1, 1, 13, 19, 23)):
        p, t = _inputs(shape, "unit")
        p, t = p.to(dev), t.to(dev)
        same = kernels.enhance_metrics(t, t.clone()).cpu()
        assert abs(same[0].item() - 1) <= 1e-6 and same[1].item() == float("inf"), same
        a, b = kernels.enhance_metrics(p, t), kernels.enhance_metrics(p, t)
        assert torch.equal(a, b), "two calls agree bitwise"
        pt = p.transpose(3, 4).contiguous().transpose(3, 4)       # same values, W-major strides
        assert not pt.is_contiguous() and torch.equal(pt, p)
        assert torch.equal(kernels.enhance_metrics(pt, t), a)
        assert torch.equal(kernels.enhance_metrics(p[:, :, :, ::1, :-1], t[..., :-1]),
                           kernels.enhance_metrics(p[..., :-1].contiguous(), t[..., :-1].contiguous()))
        q = p.clone()
        q.view(-1)[0] = float("nan")                             # a corner voxel: inside one window only
        assert torch.isnan(kernels.enhance_metrics(q, t)).all()


def _seg_case(name):
    g = torch.Generator().manual_seed(37)
    if name == "binary":              # sample 1 has no class 1 in prediction or labels: its F1 is 0
        B, C, sp = 2, 2, (1, 19, 23)
        lg = torch.randn(B, C, *sp, generator=g)
        lb = torch.randint(0, C, (B, *sp), generator=g)
        lg[1, 0] += 100
        lb[1] = 0
    elif name == "absent":            # class 7 occurs nowhere
        B, C, sp = 2, 10, (3, 5, 4)
        lg = torch.randn(B, C, *sp, generator=g)
        lg[:, 7] = -100
        lb = torch.randint(0, C, (B, *sp), generator=g)
        lb[lb == 7] = 6
    elif name == "blocks":            # several workgroups per sample
        B, C, sp = 1, 10, (6, 37, 70)
        lg = torch.randn(B, C, *sp, generator=g)
        lb = torch.randint(0, C, (B, *sp), generator=g)
    elif name == "ties":              # bf16 logits on a grid of 0.5: most maxima are tied
        B, C, sp = 1, 3, (1, 64, 65)
        lg = ((torch.randn(B, C, *sp, generator=g)).round() / 2).to(torch.bfloat16)
        lb = torch.randint(0, C, (B, *sp), generator=g)
    elif name == "odd":               # several workgroups on the one-position-per-load path (S no multiple of 4)
        B, C, sp = 1, 4, (1, 67, 129)
        lg = torch.randn(B, C, *sp, generator=g)
        lb = torch.randint(0, C, (B, *sp), generator=g)
    elif name == "stride":            # more 4096-position chunks (1026) than workgroups per sample (1024): the
        B, C, sp = 1, 2, (1, 2052, 2048)   # grid-stride loop only shows at this size
        lg = torch.randn(B, C, *sp, generator=g)
        lb = torch.randint(0, C, (B, *sp), generator=g)
    elif name == "outside":           # labels outside [0, C) match no class
        B, C, sp = 2, 3, (1, 9, 11)
        lg = torch.randn(B, C, *sp, generator=g)
        lb = torch.randint(-1, C + 1, (B, *sp), generator=g)
    return lg, lb


@pytest.mark.parametrize("name", ["binary", "absent", "blocks", "ties", "odd", "stride", "outside"])
def test_seg_f1(name):
    from long_context_biomedical_imaging_amd import kernels
    lg, lb = _seg_case(name)
    B, C = lg.shape[:2]
    pred = torch.argmax(lg, 1).reshape(B, -1)
    if name == "ties":
        top = lg.float().amax(1, keepdim=True)
        assert ((lg.float() == top).sum(1) > 1).float().mean() > 0.2, "the grid forces ties"
    want, counts = f1_ref(pred, lb.reshape(B, -1), C)
    if name == "binary":
        assert counts[1, 1].sum() == 0
    if name == "absent":
        assert counts[:, 7].sum() == 0
    f1, got = kernels.seg_f1(lg.to(_dev()), lb.to(_dev()))
    f1b, gotb = kernels.seg_f1(lg.to(_dev()), lb.to(_dev()))
    assert got.dtype == torch.int64 and f1.dtype == torch.float32 and f1.dim() == 0
    assert torch.equal(got.cpu(), counts)
    assert torch.equal(f1, f1b) and torch.equal(got, gotb), "repeatable bitwise"
    print(f"{name}: f1 {f1.item():.8f} want {want:.8f}")
    assert abs(f1.item() - want) <= 1e-6
    if name == "outside":
        assert torch.equal(got.cpu(), f1_counts(pred, lb.reshape(B, -1), C))
        assert got[..., 2].sum().item() < (pred != lb.reshape(B, -1)).sum().item()   # some misses carry no fn


def test_graph_capture_matches_eager():
    """Both ops captured once in one graph on static buffers; a replay on new contents equals eager bitwise (no host
    sync, no allocation that moves, nothing read on the host)."""
    from long_context_biomedical_imaging_amd import kernels
    dev = _dev()
    p0, t0 = _inputs((1, 1, 13, 19, 23), "unit")
    lg0, lb0 = _seg_case("blocks")
    p, t, lg, lb = p0.to(dev), t0.to(dev), lg0.to(dev), lb0.to(dev)
    kernels.enhance_metrics(p, t), kernels.seg_f1(lg, lb)        # first use outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="relaxed"):
        em = kernels.enhance_metrics(p, t)
        f1, counts = kernels.seg_f1(lg, lb)
    p1, t1 = _inputs((1, 1, 13, 19, 23), "offset", seed=38)
    g = torch.Generator().manual_seed(38)
    p.copy_(p1), t.copy_(t1)
    lg.copy_(torch.randn(lg0.shape, generator=g)), lb.copy_(torch.randint(0, 10, lb0.shape, generator=g))
    graph.replay()
    torch.cuda.synchronize()
    want_f1, want_counts = kernels.seg_f1(lg, lb)
    assert torch.equal(em, kernels.enhance_metrics(p, t))
    assert torch.equal(f1, want_f1) and torch.equal(counts, want_counts)
    assert not torch.equal(counts.cpu(), f1_counts(torch.argmax(lg0, 1).reshape(1, -1), lb0.reshape(1, -1), 10))


COMMON = ["--height", "64", "--width", "64", "--time", "1", "--no_in_channel", "1", "--optim_type", "adam",
          "--optim.lr", "1e-3", "--use_amp"]
MODELS = {
    # the smallest Swin preset under the 2-D UperNet head, two classes
    "seg": ["--encoder_name", "Swin", "--Swin.size", "tiny", "--Swin.patch_size", "1", "2", "2", "--Swin.window_size",
            "1", "7", "7", "--decoder_name", "UperNet2D", "--task_type", "seg", "--no_out_channel", "2",
            "--loss_func", "CrossEntropy"],
    # the enhance model of tests/test_enhance_loss_gpu.py::test_real_model_step_under_autocast
    "enhance": ["--encoder_name", "ViT", "--ViT.size", "custom", "--ViT.hidden_size", "128", "--ViT.mlp_dim", "256",
                "--ViT.num_layers", "12", "--ViT.num_heads", "2", "--ViT.patch_size", "4", "--decoder_name",
                "UperNet2D", "--task_type", "enhance", "--no_out_channel", "1", "--loss_func", "CombinationEnhance"],
}


def _model(task, seed=3):
    from long_context_biomedical_imaging_amd import config, model_base
    cfg = config.parse_config(MODELS[task] + COMMON)
    torch.manual_seed(seed)
    m = model_base.EncoderDecoderModel(cfg, cfg.encoder_name, cfg.decoder_name, 1, cfg.no_out_channel).to(_dev())
    return cfg, m


def _batch(task, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 1, 1, 64, 64, generator=g)
    y = torch.randint(0, 2, (n, 1, 64, 64), generator=g) if task == "seg" else 0.5 * x + 0.1
    return x.to(_dev()), y.to(_dev())


def _kernel_values(task, loss, out, y):
    from long_context_biomedical_imaging_amd import kernels
    if task == "seg":
        return [loss.item(), kernels.seg_f1(out, y)[0].item()]
    return [loss.item(), *kernels.enhance_metrics(out, y).tolist()]


@pytest.mark.parametrize("task", ["seg", "enhance"])
def test_eval_step(task):
    from long_context_biomedical_imaging_amd import trainer
    cfg, m = _model(task)
    m.train()
    ev = trainer.EvalStep(m, cfg, _dev())
    assert ev.metrics.names == (("loss", "f1") if task == "seg" else ("loss", "ssim", "psnr"))
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert any("running_mean" in k for k in before), "the head has BatchNorm"
    steps = []
    for n, seed in ((2, 11), (1, 12)):                           # the batch of 1 is not duplicated
        x, y = _batch(task, n, seed)
        out, loss = ev.step(x, y)
        assert out.shape[0] == n and out.is_cuda and loss.is_cuda and loss.dim() == 0
        assert all(mod.training for mod in m.modules()), "training flags restored"
        m.eval()
        with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            want = m(x)
        m.train()
        assert torch.equal(out, want)
        steps.append((n, _kernel_values(task, loss, out, y)))
        if len(steps) == 1:
            got = ev.metrics.result()
            assert [got[k] for k in ev.metrics.names] == steps[0][1], "the metrics are the kernels on that output"
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed"
    got = ev.metrics.result()
    print(f"eval {task}: {got}")
    for i, k in enumerate(ev.metrics.names):
        want = sum(n * v[i] for n, v in steps) / sum(n for n, _ in steps)
        assert abs(got[k] - want) <= 1e-12 * max(1.0, abs(want)), (k, got[k], want)
        assert got[k] == got[k]
    ev.metrics.reset()
    m.eval()
    ev.step(*_batch(task, 2, 11))
    assert not any(mod.training for mod in m.modules()), "an eval-mode model stays in eval mode"
    again = ev.metrics.result()
    assert [again[k] for k in ev.metrics.names] == steps[0][1], "reset() cleared the sums"
    # evaluation interleaves with training: nothing the inference-mode step left behind (cached index / weight
    # tables) stops a training step on the same model
    m.train()
    loss = trainer.TrainStep(m, cfg, _dev(), ddp=False).step(*_batch(task, 2, 13))
    assert torch.isfinite(loss).item()


class _RowTokens(torch.nn.Module):
    """A (B, 1, 1, 64, 128) image as 64 row tokens of width 128 through two ViT blocks and back. Every kernel of its
    step (HIP attention, LayerNorm, the linear weight gradients, the loss, Adam) sums in a fixed order, so two seeded
    runs agree bitwise — tests/test_ddp.py compares the same blocks across ranks that way. The UperNet models above
    do not: torch's own convolution / BatchNorm gradients there change in the last bits from run to run, with or
    without a meter, so a bitwise comparison on them would test torch."""

    def __init__(self):
        super().__init__()
        from long_context_biomedical_imaging_amd import backbone_vit
        self.blocks = torch.nn.Sequential(backbone_vit.TransformerBlock(False, False, 128, 256, 2),
                                          backbone_vit.TransformerBlock(False, True, 128, 256, 2))

    def forward(self, x):
        return self.blocks(x.reshape(x.shape[0], 64, 128)).reshape(x.shape).float()


def _train(attach, steps=4):
    from long_context_biomedical_imaging_amd import config, metrics, trainer
    cfg = config.parse_config(["--task_type", "enhance", "--optim_type", "adam", "--optim.lr", "1e-3", "--loss_func",
                               "CombinationEnhance", "--use_amp"])
    torch.manual_seed(3)
    m = _RowTokens().to(_dev()).train()
    ts = trainer.TrainStep(m, cfg, _dev(), ddp=False)
    assert ts.metrics is None
    outs = []
    if attach:
        ts.metrics = metrics.TaskMetrics(cfg)
        m.register_forward_hook(lambda mod, args, out: outs.append(out.detach().clone()))
    torch.manual_seed(5)
    losses, ys = [], []
    for i in range(steps):
        g = torch.Generator().manual_seed(20 + i)
        x = torch.rand(2, 1, 1, 64, 128, generator=g).to(_dev())
        y = 0.5 * x + 0.1
        losses.append(ts.step(x, y).clone())
        ys.append(y)
    torch.cuda.synchronize()
    return ts, losses, [p.detach().clone() for p in m.parameters()], outs, ys


def test_train_step_metrics_opt_in():
    """Four seeded steps with and without a TaskMetrics attached give bitwise-equal losses and parameters, and the
    attached meter's result is the kernels applied step by step."""
    _, l0, w0, _, _ = _train(False)
    ts, l1, w1, outs, ys = _train(True)
    assert not any(torch.equal(a, b) for a, b in zip(l1[:-1], l1[1:])), "the steps train"
    for a, b in zip(l0, l1):
        assert torch.equal(a, b)
    for a, b in zip(w0, w1):
        assert torch.equal(a, b)
    assert len(outs) == 4
    vals = [_kernel_values("enhance", loss, out, y) for loss, out, y in zip(l1, outs, ys)]
    got = ts.metrics.result()
    print(f"train meter: {got}")
    for i, k in enumerate(ts.metrics.names):
        want = sum(2 * v[i] for v in vals) / 8
        assert abs(got[k] - want) <= 1e-12 * max(1.0, abs(want)), (k, got[k], want)


def _conv_train(graphed):
    """2 eager steps, then 3 more (eager) or a capture and 3 replays (graphed), with a meter attached throughout."""
    from long_context_biomedical_imaging_amd import config, metrics, trainer
    cfg = config.parse_config(["--task_type", "enhance", "--optim_type", "adam", "--optim.lr", "1e-3", "--loss_func",
                               "CombinationEnhance"])
    torch.manual_seed(0)
    model = torch.nn.Conv3d(1, 1, 3, padding=1).to(_dev())
    ts = trainer.TrainStep(model, cfg, _dev(), ddp=False)
    ts.metrics = metrics.TaskMetrics(cfg)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1, 12, 16, 16, generator=g).to(_dev())
    y = torch.randn(2, 1, 12, 16, 16, generator=g).to(_dev())
    if graphed:
        gs = trainer.GraphedStep(ts, x, y, warmup=2)
        for _ in range(3):
            gs.step()
    else:
        for _ in range(5):
            ts.step(x, y)
    torch.cuda.synchronize()
    return ts.metrics


def test_graphed_step_captures_the_meter():
    """The meter's update is part of the captured step (no host sync in it, sums updated in place): every replay adds
    its batch, and the averages are those of the same steps run eagerly (tolerance of tests/test_graph_gpu.py)."""
    eager, graphed = _conv_train(False), _conv_train(True)
    assert eager._acc[-1].item() == graphed._acc[-1].item() == 10      # 5 executed steps of 2 samples
    a, b = eager.result(), graphed.result()
    print(f"meter eager {a} graphed {b}")
    for k in a:
        assert a[k] == a[k] and abs(a[k] - b[k]) <= 1e-5 * max(1.0, abs(a[k])), (k, a[k], b[k])
