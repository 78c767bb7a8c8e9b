"""LR schedules in the optimizer update (csrc/optim.hip: lci_adam_step_ex, lci_onecycle_eval, lci_grad_sumsq,
lci_grad_clip_coef) against torch's own scheduler classes and fused Adam / AdamW: the recipes' OneCycleLR evaluated
from the device step count, a device-tensor learning rate, the fused grad-norm clip, and the whole TrainStep /
GraphedStep under --scheduler_type OneCycleLR (trainer_base.py:173-182, optim_base.py:101-115)."""
import os
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

# sizes: tiny / ragged / one chunk / several chunks / ragged tails; 45 tensors = two launches of <= 40; the last
# tensor starts 4 bytes into its allocation (not 16-byte aligned: the kernels' scalar path)
SIZES = [1, 3, 7, 384, 2047, 2048, 2049, 4096 + 5, 65536 + 3, 147456] * 4 + [1536, 96, 8, 9, 4096 + 3]
TOL = 2.0 ** -22


def _tensors(seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ts = [torch.randn(n, device="cuda", generator=g) * scale for n in SIZES[:-1]]
    ts.append((torch.randn(SIZES[-1] + 1, device="cuda", generator=g) * scale)[1:])
    assert ts[-1].data_ptr() % 16 == 4 and ts[-1].is_contiguous()
    return ts


def _rel(x, y):
    return ((x - y).abs() / (x.abs() + 1e-30)).max().item()


def _worst(ref, lci):
    worst = 0.0
    for a, b in zip(ref.param_groups[0]["params"], lci.param_groups[0]["params"]):
        sa, sb = ref.state[a], lci.state[b]
        assert float(sa["step"]) == float(sb["step"])
        for x, y in ((a, b), (sa["exp_avg"], sb["exp_avg"]), (sa["exp_avg_sq"], sb["exp_avg_sq"])):
            worst = max(worst, _rel(x, y))
    return worst


def _set_grads(ref, lci, gen, scale=1.0):
    for a, b in zip(ref.param_groups[0]["params"], lci.param_groups[0]["params"]):
        gr = torch.randn(a.shape, device="cuda", generator=gen) * scale
        a.grad = gr.clone()
        b.grad = torch.cat([gr.new_zeros(1), gr])[1:] if b.data_ptr() % 16 else gr.clone()


def _host_onecycle(total, pct, max_lr, step_nums):
    """torch's OneCycleLR on the host at the given step numbers: the constants the kernel takes and (lr, beta1)."""
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=max_lr, betas=(0.9, 0.99))
    s = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=total, pct_start=pct,
                                            anneal_strategy="cos")
    g = opt.param_groups[0]
    consts = (s.total_steps, s._schedule_phases[0]["end_step"], g["initial_lr"], g["max_lr"], g["min_lr"],
              g["base_momentum"], g["max_momentum"])
    opt.step()
    vals = []
    for k in step_nums:
        s.last_epoch = k - 1
        s.step()
        vals.append((g["lr"], g["betas"][0]))
    return consts, vals


# ------------------------------------------------------------------------------------------- 1. schedule values
@pytest.mark.parametrize("total,pct,step_nums", [
    (10, 0.3, list(range(10))),
    (7, 0.3, list(range(7))),                          # end_step1 = 1.1, not an integer
    (200000, 0.3, [0, 1, 59999, 60000, 60001, 199999]),
])
@pytest.mark.parametrize("max_lr", [1e-4, 1e-3])
def test_onecycle_eval_matches_torch_on_the_host(total, pct, step_nums, max_lr):
    from long_context_biomedical_imaging_amd import kernels
    consts, host = _host_onecycle(total, pct, max_lr, step_nums)
    steps = torch.tensor([k + 1 for k in step_nums], device="cuda", dtype=torch.float32)   # counts after increment
    dev = kernels.onecycle_eval(steps, consts).cpu()
    # a 4-ulp double cos (the OpenCL bound the device math library follows) through anneal: 2^-50 of the larger end
    lr_bound, mom_bound = 2.0 ** -50 * consts[3], 2.0 ** -50 * consts[6]
    for i, k in enumerate(step_nums):
        d_lr, d_m = abs(dev[i, 0].item() - host[i][0]), abs(dev[i, 1].item() - host[i][1])
        print(f"step {k}: lr {dev[i, 0].item():.17g} (host diff {d_lr:.3e}, bound {lr_bound:.3e}), "
              f"beta1 {dev[i, 1].item():.17g} (host diff {d_m:.3e}, bound {mom_bound:.3e})")
        assert d_lr <= lr_bound and d_m <= mom_bound, (k, d_lr, d_m)
    assert dev[0, 0].item() == pytest.approx(max_lr / 25, rel=1e-12) and dev[0, 1].item() == pytest.approx(0.95)


def test_schedule_and_device_lr_together_are_refused():
    from long_context_biomedical_imaging_amd import _lib, kernels
    t = [torch.zeros(4, device="cuda") for _ in range(4)]
    step, lr = torch.ones((), device="cuda"), torch.full((), 1e-3, device="cuda")
    consts, _ = _host_onecycle(10, 0.3, 1e-3, [])
    with pytest.raises(_lib.LciError, match="exclude"):
        kernels.adam_step([t[0]], [t[1]], [t[2]], [t[3]], [step], 1e-3, 0.9, 0.95, 0.0, 1e-8, False, False,
                          lr_tensor=lr, sched=consts)
    assert all(float(x.abs().sum()) == 0.0 for x in t)


# ------------------------------------------------------------------------------------------- 2. one-cycle update
@pytest.mark.parametrize("adamw,wd", [(False, 0.01), (True, 0.05)])
def test_onecycle_update_matches_torch_fused_with_the_same_hyperparameters(adamw, wd):
    from long_context_biomedical_imaging_amd import kernels
    from long_context_biomedical_imaging_amd.trainer import LciAdam, LciAdamW, LciOneCycleLR
    total, pct, max_lr = 20, 0.3, 3e-4                 # end_step1 = 5.0: updates at step_num 3..7 straddle it
    kw = dict(lr=max_lr, betas=(0.9, 0.95), weight_decay=wd, eps=1e-8)
    ref = (torch.optim.AdamW if adamw else torch.optim.Adam)([torch.nn.Parameter(p) for p in _tensors(1)],
                                                             fused=True, **kw)
    lci = (LciAdamW if adamw else LciAdam)([torch.nn.Parameter(p) for p in _tensors(1)], **kw)
    sched = LciOneCycleLR(lci, max_lr=max_lr, total_steps=total, pct_start=pct)
    consts = lci.onecycle_constants(lci.param_groups[0])
    assert consts is not None and consts[1] == 5.0
    gen = torch.Generator(device="cuda").manual_seed(7)
    # one update creates the state; then both optimizers restart from the same state at step count 3
    _set_grads(ref, lci, gen)
    ref.step(), lci.step()
    for a, b in zip(ref.param_groups[0]["params"], lci.param_groups[0]["params"]):
        with torch.no_grad():
            b.copy_(a)
        for key in ("exp_avg", "exp_avg_sq"):
            lci.state[b][key].copy_(ref.state[a][key])
        ref.state[a]["step"].fill_(3.0)
        lci.state[b]["step"].fill_(3.0)
    p0 = lci.param_groups[0]["params"][0]
    seen = []
    for _ in range(5):
        lr, beta1 = kernels.onecycle_eval(lci.state[p0]["step"].reshape(1) + 1, consts)[0].tolist()
        seen.append(lr)
        ref.param_groups[0]["lr"] = lr
        ref.param_groups[0]["betas"] = (beta1, 0.95)
        _set_grads(ref, lci, gen)
        ref.step(), lci.step()
    assert float(lci.state[p0]["step"]) == 8.0
    assert seen[2] == pytest.approx(max_lr, rel=1e-12) and seen[1] < seen[2] > seen[3] and len(set(seen)) == 5
    worst = _worst(ref, lci)
    print(f"one-cycle update: max relative difference {worst:.3e}")
    assert worst <= TOL, f"max relative difference {worst:.3e}"
    assert sched.last_epoch == 0                       # the kernel follows the device count, not the host mirror


# ------------------------------------------------------------------------------------------- 3. tensor lr
def test_tensor_lr_follows_step_lr_and_a_captured_step_sees_fill():
    from long_context_biomedical_imaging_amd.trainer import LciAdam
    kw = dict(betas=(0.9, 0.95), eps=1e-8)
    ref = torch.optim.Adam([torch.nn.Parameter(p) for p in _tensors(2)], lr=torch.tensor(3e-4, device="cuda"),
                           fused=True, capturable=True, **kw)
    lci = LciAdam([torch.nn.Parameter(p) for p in _tensors(2)], lr=torch.tensor(3e-4, device="cuda"), **kw)
    s_ref = torch.optim.lr_scheduler.StepLR(ref, step_size=1, gamma=0.8)
    s_lci = torch.optim.lr_scheduler.StepLR(lci, step_size=1, gamma=0.8)
    gen = torch.Generator(device="cuda").manual_seed(9)
    for _ in range(5):
        _set_grads(ref, lci, gen)
        ref.step(), lci.step()
        s_ref.step(), s_lci.step()
    assert isinstance(lci.param_groups[0]["lr"], torch.Tensor)
    assert torch.equal(lci.param_groups[0]["lr"], ref.param_groups[0]["lr"])
    assert float(lci.param_groups[0]["lr"]) == pytest.approx(3e-4 * 0.8 ** 5, rel=1e-6)
    worst = _worst(ref, lci)
    print(f"tensor lr: max relative difference {worst:.3e}")
    assert worst <= TOL, f"max relative difference {worst:.3e}"

    # one captured step, the learning rate filled between replays = the same steps run eagerly
    pe = [torch.nn.Parameter(p) for p in _tensors(3)[-14:]]
    pg = [torch.nn.Parameter(p) for p in _tensors(3)[-14:]]
    oe = LciAdam(pe, lr=torch.tensor(1e-3, device="cuda"), **kw)
    og = LciAdam(pg, lr=torch.tensor(1e-3, device="cuda"), **kw)
    grads = [torch.randn(p.shape, device="cuda", generator=gen) for p in pe]
    for p, q, gr in zip(pe, pg, grads):
        p.grad, q.grad = gr.clone(), gr.clone()
    oe.step(), og.step()                               # state initialised outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()
    for v in (5e-4, 2.5e-4, 7e-3):
        oe.param_groups[0]["lr"].fill_(v)
        og.param_groups[0]["lr"].fill_(v)
        graph.replay()
        oe.step()
    torch.cuda.synchronize()
    for a, b in zip(pe, pg):
        assert torch.equal(a, b)
    assert float(og.state[pg[0]]["step"]) == 4.0


# ------------------------------------------------------------------------------------------- 4. grad norm and clip
@pytest.mark.parametrize("case", ["above", "below", "zero"])
def test_grad_norm_and_clip_coefficient(case):
    from long_context_biomedical_imaging_amd import kernels
    grads = _tensors(4)
    if case == "zero":
        grads = [torch.zeros_like(g) for g in grads]
    max_norm = {"above": 1.0, "below": 1e6, "zero": 1.0}[case]
    norm, coef = kernels.grad_clip_coef(grads, max_norm)
    want = torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).item()
    want_coef = min(1.0, max_norm / (want + 1e-6))
    print(f"{case}: norm {norm.item():.9g} (fp64 {want:.12g}), coefficient {coef.item():.9g} (fp64 {want_coef:.12g})")
    assert norm.dtype == coef.dtype == torch.float32
    if case == "zero":
        assert norm.item() == 0.0 and coef.item() == 1.0
        return
    assert abs(norm.item() - want) <= TOL * want
    if case == "below":
        assert coef.item() == 1.0
    else:
        assert want > max_norm and abs(coef.item() - want_coef) <= TOL * want_coef


def test_fused_clipped_step_matches_torch_on_scaled_gradients():
    from long_context_biomedical_imaging_amd import kernels
    from long_context_biomedical_imaging_amd.trainer import LciAdam
    kw = dict(lr=3e-4, betas=(0.9, 0.95), weight_decay=0.01, eps=1e-8)
    ref = torch.optim.Adam([torch.nn.Parameter(p) for p in _tensors(5)], fused=True, **kw)
    lci = LciAdam([torch.nn.Parameter(p) for p in _tensors(5)], **kw)
    gen = torch.Generator(device="cuda").manual_seed(13)
    for _ in range(3):
        _set_grads(ref, lci, gen)
        lci_params = lci.param_groups[0]["params"]
        kept = [p.grad.clone() for p in lci_params]
        norm, coef = kernels.grad_clip_coef([p.grad for p in lci_params], 10.0)
        assert 0.0 < coef.item() < 1.0
        for a in ref.param_groups[0]["params"]:
            a.grad.mul_(coef)                          # f32, clip_grad_norm_'s in-place multiply
        lci._lci_grad_coef = coef
        ref.step(), lci.step()
        lci._lci_grad_coef = None
        assert all(torch.equal(p.grad, k) for p, k in zip(lci_params, kept)), "the fused clip rewrote p.grad"
    worst = _worst(ref, lci)
    print(f"fused clipped step: max relative difference {worst:.3e}")
    assert worst <= TOL, f"max relative difference {worst:.3e}"


# ------------------------------------------------------------------------------------------- 5. whole step
TOTAL = 8


def _trainer(flags, total_updates=None):
    from long_context_biomedical_imaging_amd import backbone_swin, config
    from long_context_biomedical_imaging_amd.trainer import TrainStep
    torch.manual_seed(0)
    model = torch.nn.Sequential(
        backbone_swin.BasicLayer(False, False, dim=64, depth=2, num_heads=2, window_size=(4, 4, 4),
                                 drop_path=[0.0, 0.0], downsample=None)).cuda()
    cfg = config.parse_config(["--optim_type", "adam", "--optim.lr", "1e-3", "--loss_func", "MSE", "--use_amp", *flags])
    ts = TrainStep(model, cfg, torch.device("cuda"), ddp=False, total_updates=total_updates)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 6, 8, 8, generator=g).cuda()
    y = torch.randn(2, 64, 6, 8, 8, generator=g).cuda()
    return ts, x, y


def _weights(ts):
    torch.cuda.synchronize()
    return [p.detach().float().cpu() for p in ts.model.parameters()]


def _check_invariant(ts, want):
    steps = {int(ts.optim.state[p]["step"]) for p in ts.model.parameters()}
    assert steps == {want} and ts.sched.last_epoch == want, (steps, ts.sched.last_epoch, want)


@pytest.fixture(scope="module")
def runs():
    from long_context_biomedical_imaging_amd.trainer import GraphedStep, LciAdam
    onecycle = ["--scheduler_type", "OneCycleLR"]
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ts, x, y = _trainer(onecycle, TOTAL)
        assert isinstance(ts.optim, LciAdam)
        for _ in range(6):
            loss = ts.step(x, y)
        _check_invariant(ts, 6)
        out["eager"] = (float(loss), _weights(ts), ts, x, y)

        ts, x, y = _trainer(onecycle, TOTAL)
        gs = GraphedStep(ts, x, y, warmup=2)
        _check_invariant(ts, 2)                        # two warm-up updates; the capture applied none
        for _ in range(4):
            loss = gs.step()
        torch.cuda.synchronize()
        _check_invariant(ts, 6)
        out["graphed"] = (float(loss), _weights(ts), ts, gs)

        old = os.environ.get("LCI_HIP_ADAM")
        os.environ["LCI_HIP_ADAM"] = "0"
        try:
            ts, x, y = _trainer(onecycle, TOTAL)
        finally:
            if old is None:
                del os.environ["LCI_HIP_ADAM"]
            else:
                os.environ["LCI_HIP_ADAM"] = old
        assert type(ts.optim) is torch.optim.Adam and getattr(ts.optim, "_lci_sched", None) is None
        for _ in range(6):
            loss = ts.step(x, y)
        _check_invariant(ts, 6)
        out["torch"] = (float(loss), _weights(ts))

        ts, x, y = _trainer([])
        for _ in range(6):
            loss = ts.step(x, y)
        out["constant"] = (float(loss), _weights(ts))
    return out


def _close(a, b):
    worst = max(((x - y).abs() - 1e-5 * y.abs()).max().item() for x, y in zip(a[1], b[1]))
    print(f"loss {a[0]:.8g} vs {b[0]:.8g}; max (|a - b| - 1e-5 |b|) over the weights {worst:.3e} (atol 1e-6)")
    assert abs(a[0] - b[0]) <= 1e-5 * max(1.0, abs(b[0]))
    for x, y in zip(a[1], b[1]):
        assert torch.allclose(x, y, rtol=1e-5, atol=1e-6), (x - y).abs().max()


def test_graphed_onecycle_step_matches_eager(runs):
    _close(runs["graphed"], runs["eager"])


def test_hip_onecycle_step_matches_torch_fused_adam_with_torch_onecycle(runs):
    _close(runs["eager"], runs["torch"])


def test_onecycle_run_differs_from_a_constant_lr_run(runs):
    assert any(not torch.allclose(a, b, rtol=1e-5, atol=1e-6) for a, b in zip(runs["eager"][1], runs["constant"][1]))


def test_update_past_total_steps_raises(runs):
    """Runs last: it finishes the two cycles (updates 7 and 8) and asks for a 9th."""
    _, _, ts, x, y = runs["eager"]
    _, _, tg, gs = runs["graphed"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(2):
            ts.step(x, y)
            gs.step()
        torch.cuda.synchronize()
        _check_invariant(ts, TOTAL)
        _check_invariant(tg, TOTAL)
        with pytest.raises(ValueError, match="Tried to step"):
            gs.step()                                  # refused before the replay is launched
        torch.cuda.synchronize()
        _check_invariant(tg, TOTAL)
        with pytest.raises(ValueError, match="Tried to step"):
            ts.step(x, y)


def test_train_step_fused_clip_matches_clip_grad_norm(monkeypatch):
    """--clip_grad_norm on a CUDA LciAdam: TrainStep routes the clip through kernels.grad_clip_coef and the update
    kernel, eager and captured, and trains like clip_grad_norm_ + torch's fused Adam (LCI_HIP_ADAM=0)."""
    from long_context_biomedical_imaging_amd.trainer import GraphedStep
    clip = ["--clip_grad_norm", "0.01"]

    def run(graphed):
        ts, x, y = _trainer(clip)
        if graphed:
            gs = GraphedStep(ts, x, y, warmup=2)
            for _ in range(2):
                loss = gs.step()
        else:
            for _ in range(4):
                loss = ts.step(x, y)
        return (float(loss), _weights(ts)), ts

    eager, ts = run(False)
    assert ts.fused_clip and 0.01 < float(ts.grad_norm)          # the clip was active, by the fused route
    graphed, _ = run(True)
    monkeypatch.setenv("LCI_HIP_ADAM", "0")
    ref, tr = run(False)
    assert not tr.fused_clip
    print(f"last grad norm: fused {float(ts.grad_norm):.8g}, clip_grad_norm_ {float(tr.grad_norm):.8g}")
    assert float(ts.grad_norm) == pytest.approx(float(tr.grad_norm), rel=1e-5)
    _close(graphed, eager)
    _close(eager, ref)


EPOCH_SCHED = {
    "StepLR": (["--scheduler_type", "StepLR", "--scheduler.step_size", "1", "--scheduler.gamma", "0.5"], None),
    # patience 0: the second and third epochs' loss is no better than the first's, so each halves the lr
    "ReduceLROnPlateau": (["--scheduler_type", "ReduceLROnPlateau", "--scheduler.patience", "0",
                           "--scheduler.factor", "0.5"], 1.0),
}


def _host_epoch_lrs(kind, lr0, epochs):
    """torch's scheduler on a host-float Adam: the lr after each epoch."""
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr0)
    s = (torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5) if kind == "StepLR" else
         torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=0, cooldown=0, min_lr=1e-8))
    out = []
    for _ in range(epochs):
        opt.step()
        s.step() if kind == "StepLR" else s.step(1.0)
        out.append(opt.param_groups[0]["lr"])
    return out


@pytest.mark.parametrize("kind", sorted(EPOCH_SCHED))
def test_epoch_scheduler_on_adam_writes_a_device_lr_that_a_captured_step_follows(kind, monkeypatch):
    """build_optimizer + TrainStep.end_epoch + GraphedStep as a user reaches them: three epochs of two updates."""
    from long_context_biomedical_imaging_amd.trainer import GraphedStep, LciAdam
    flags, loss_arg = EPOCH_SCHED[kind]
    want = _host_epoch_lrs(kind, 1e-3, 3)
    assert want[-1] < 1e-3 / 3                         # the schedule really moved the lr

    def run(graphed, flags=flags, epochs=True, prepare=None):
        ts, x, y = _trainer(flags)
        if prepare is not None:
            prepare(ts)
        gs = GraphedStep(ts, x, y, warmup=2) if graphed else None     # the warm-up is the first epoch's two updates
        seen = []
        for e in range(3):
            for _ in range(0 if graphed and e == 0 else 2):
                loss = gs.step() if graphed else ts.step(x, y)
            if epochs:
                ts.end_epoch(loss_arg)
                seen.append(float(ts.optim.param_groups[0]["lr"]))
        return (float(loss), _weights(ts)), ts, seen

    eager, ts, seen = run(False)
    lr = ts.optim.param_groups[0]["lr"]
    assert isinstance(ts.optim, LciAdam) and isinstance(lr, torch.Tensor)
    assert lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1
    assert seen == pytest.approx(want, rel=2.0 ** -22)   # 1e-3 and at most three products, each rounded to f32
    graphed, tg, seen_g = run(True)
    assert seen_g == seen and int(tg.optim.state[next(tg.model.parameters())]["step"]) == 6
    print(f"{kind}: lr per epoch {seen} (host double {want})")
    _close(graphed, eager)
    constant, _, _ = run(True, flags=[], epochs=False)
    assert any(not torch.allclose(a, b, rtol=1e-5, atol=1e-6) for a, b in zip(graphed[1], constant[1]))
    # Reference for the weights: torch's fused Adam with the same hyper-parameters, i.e. the same one-element f32 lr
    # (capturable, as in the tensor-lr test above) under torch's scheduler. Not the LCI_HIP_ADAM=0 trainer as built:
    # its lr is the host double, 2.5e-9 .. 3e-8 relative away from the f32 value (the deviation DESIGN §7 records),
    # and Adam divides by sqrt(v), so on elements whose gradient is near zero a last-bit difference in the weights
    # becomes a whole +-lr step within a few updates under bf16 autocast: measured against that trainer, the losses
    # agree to every printed digit for three updates and single elements differ by 2.4e-4 (one lr) after six.
    from long_context_biomedical_imaging_amd import config
    from long_context_biomedical_imaging_amd.trainer import build_scheduler

    def same_lr_torch(tr):
        assert type(tr.optim) is torch.optim.Adam and isinstance(tr.optim.param_groups[0]["lr"], float)
        g = tr.optim.param_groups[0]
        tr.optim = torch.optim.Adam(tr.model.parameters(), lr=torch.tensor(1e-3, device="cuda"), betas=g["betas"],
                                    weight_decay=g["weight_decay"], fused=True, capturable=True)
        tr.sched = build_scheduler(tr.optim, config.parse_config(flags), None)

    monkeypatch.setenv("LCI_HIP_ADAM", "0")
    ref, tr, seen_r = run(False, prepare=same_lr_torch)
    assert seen_r == seen
    _close(eager, ref)


def test_epoch_scheduler_on_sgd_keeps_torchs_host_lr():
    """SGD / NAdam take the schedulers through torch on the host: a float lr with torch's values, eager only."""
    from long_context_biomedical_imaging_amd.trainer import GraphedStep
    for optim_type in ("sgd", "nadam"):
        ts, x, y = _trainer(["--optim_type", optim_type, *EPOCH_SCHED["StepLR"][0]])
        assert isinstance(ts.optim.param_groups[0]["lr"], float)
        seen = []
        for _ in range(3):
            ts.step(x, y)
            ts.end_epoch()
            seen.append(ts.optim.param_groups[0]["lr"])
        assert seen == _host_epoch_lrs("StepLR", 1e-3, 3) and all(isinstance(v, float) for v in seen)
        with pytest.raises(ValueError, match="LciAdam"):
            GraphedStep(ts, x, y)


def test_captured_onecycle_refuses_a_group_on_torchs_fused_update():
    """An amsgrad group takes torch's fused kernel, whose lr / betas would be the capture's host values for good."""
    from long_context_biomedical_imaging_amd.trainer import LciAdam, LciOneCycleLR
    ps = [torch.nn.Parameter(torch.randn(64, device="cuda"))]
    opt = LciAdam(ps, lr=1e-3, amsgrad=True)
    sched = LciOneCycleLR(opt, max_lr=1e-3, total_steps=10)   # kept alive: the optimizer holds a weak reference
    assert opt.onecycle_constants(opt.param_groups[0]) is not None and sched.last_epoch == 0
    ps[0].grad = torch.randn(64, device="cuda")
    opt.step()                                         # eager: torch's update with the host mirror, as documented
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="captured step"):
        with torch.cuda.graph(graph):
            opt.step()
    torch.cuda.synchronize()
    ps[0].grad = torch.randn(64, device="cuda")        # the device is usable after the abandoned capture
    opt.step()
    assert float(opt.state[ps[0]]["step"]) == 2.0


def test_graphed_step_refuses_a_scheduler_on_torchs_optimizer(monkeypatch):
    from long_context_biomedical_imaging_amd.trainer import GraphedStep
    monkeypatch.setenv("LCI_HIP_ADAM", "0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ts, x, y = _trainer(["--scheduler_type", "OneCycleLR"], TOTAL)
        with pytest.raises(ValueError, match="LciAdam"):
            GraphedStep(ts, x, y)
