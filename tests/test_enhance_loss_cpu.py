"""CombinationEnhance loss, the parts that need no GPU: the flag parses and reaches the trainer, the stencil factors
reproduce the reference's conv3d weights (tests/golden/enhance_loss.npz, written by tools/gen_golden_loss.py from the
reference's own loss module), the argument checks, and a plain-torch restatement of the formula that the GPU tests
use as their float64 reference."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enhance_loss.npz")
CASES = {"a": (2, 1, 6, 19, 23), "b": (1, 1, 1, 8, 8)}
EPS2 = 1e-6     # Charbonnier eps^2, eps = 1e-3


def golden():
    return np.load(GOLDEN)


def golden_windows(dtype=torch.float64):
    """The reference's three conv3d weights (kT, kH, kW) from the fixture."""
    g = golden()
    return [torch.from_numpy(g[f"window{k}"]).to(dtype) for k in range(3)]


def conv_same(x, w):
    """The zero-padded 'same' correlation of x (B, 1, T, H, W) with w (kT, kH, kW), in x's dtype."""
    return F.conv3d(x, w.to(x.dtype)[None, None], padding=[(s - 1) // 2 for s in w.shape])


def formula(o, t, windows):
    """loss = mean(d^2) + mean(sqrt(d^2 + 1e-6)) + (1/3) sum_k mean|conv_k(d)| with d = o - t, in plain torch on whatever
    device and dtype the operands have. Returns (loss, (mse, charbonnier, gaussian3D), [g_k]). The stencil term runs
    for every shape (it is 0 when T, H or W is 1)."""
    d = o - t
    mse = (d * d).mean()
    ch = torch.sqrt(d * d + EPS2).mean()
    gs = [conv_same(d, w) for w in windows]
    ga = sum(g.abs().mean() for g in gs) / 3
    return mse + ch + ga, (mse, ch, ga), gs


def reference_loss(outputs, targets, dtype=torch.float64, windows=None):
    """formula() evaluated in `dtype` with the fixture's windows. Returns (loss, components (3), d loss / d outputs,
    [g_k]) as detached `dtype` tensors on the inputs' device."""
    windows = golden_windows() if windows is None else windows
    o = outputs.detach().to(dtype).clone().requires_grad_(True)
    loss, comps, gs = formula(o, targets.detach().to(dtype), [w.to(o.device) for w in windows])
    (grad,) = torch.autograd.grad(loss, o)
    return loss.detach(), torch.stack(comps).detach(), grad, [g.detach() for g in gs]


def test_flag_parses_and_reaches_the_trainer():
    from long_context_biomedical_imaging_amd import config, losses, trainer
    cfg = config.parse_config(["--loss_func", "CombinationEnhance"])
    assert cfg.loss_func == "CombinationEnhance"
    assert isinstance(trainer.loss_fn(cfg), losses.CombinationEnhanceLoss)
    # the other two are what they were
    assert isinstance(trainer.loss_fn(config.parse_config(["--loss_func", "MSE"])), torch.nn.MSELoss)
    assert isinstance(trainer.loss_fn(config.parse_config(["--loss_func", "CrossEntropy"])), torch.nn.CrossEntropyLoss)


def test_factors_reproduce_the_reference_windows():
    """Outer products of the f32 factors the kernel gets against the reference's windows: half-widths 1 / 2 / 3 along
    H and W and 1 / 2 / 2 along T (round(1.5) == 2), the (T, H, W) axis order after the reference's permute, and the
    normalisations. Budget: the three factors' and the window's f32 roundings, 2^-21 |w| + 2^-30."""
    from long_context_biomedical_imaging_amd import losses
    tab = losses.CombinationEnhanceLoss().taps_host
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (3, 3, 7)
    tab = tab.double().numpy()
    shapes = [(3, 3, 3), (5, 5, 5), (5, 7, 7)]
    for k, w in enumerate(golden_windows()):
        w = w.numpy()
        assert w.shape == shapes[k]
        full = np.einsum("t,h,w->thw", tab[k, 0], tab[k, 1], tab[k, 2])      # (7, 7, 7), centred
        lo = [3 - (s - 1) // 2 for s in w.shape]
        inner = full[lo[0]:lo[0] + w.shape[0], lo[1]:lo[1] + w.shape[1], lo[2]:lo[2] + w.shape[2]]
        assert np.all(np.abs(inner - w) <= 2.0 ** -21 * np.abs(w) + 2.0 ** -30), np.abs(inner - w).max()
        outside = full.copy()
        outside[lo[0]:lo[0] + w.shape[0], lo[1]:lo[1] + w.shape[1], lo[2]:lo[2] + w.shape[2]] = 0
        assert not outside.any(), "taps past the half-width must be zero"
        assert abs(np.abs(inner).sum() - 1.0) < 1e-6


def test_two_channels_raise_value_error():
    from long_context_biomedical_imaging_amd import losses
    x = torch.zeros(2, 2, 3, 8, 8)
    with pytest.raises(ValueError, match="groups=C"):
        losses.CombinationEnhanceLoss()(x, x)


def test_weights_raise_not_implemented():
    from long_context_biomedical_imaging_amd import losses
    x = torch.zeros(2, 1, 3, 8, 8)
    with pytest.raises(NotImplementedError):
        losses.CombinationEnhanceLoss()(x, x, weights=torch.ones(2))


def test_cpu_tensors_raise():
    from long_context_biomedical_imaging_amd import _lib, losses
    x = torch.zeros(2, 1, 3, 8, 8)
    with pytest.raises(_lib.LciError):
        losses.CombinationEnhanceLoss()(x, x)


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_reproduces_the_fixture(case):
    """The float64 restatement against the reference's own f32 numbers: components, loss and gradient to 1e-6
    relative (of the largest gradient element for the gradient)."""
    g = golden()
    o, t = torch.from_numpy(g[f"{case}_outputs"]), torch.from_numpy(g[f"{case}_targets"])
    assert tuple(o.shape) == CASES[case]
    assert torch.equal(o, o.to(torch.bfloat16).float()), "fixture outputs are bf16-representable"
    loss, comps, grad, _ = reference_loss(o, t)
    want = g[f"{case}_components"].astype(np.float64)
    for i in range(3):
        assert abs(comps[i].item() - want[i]) <= 1e-6 * abs(want[i]), (i, comps[i].item(), want[i])
    assert abs(loss.item() - float(g[f"{case}_loss"])) <= 1e-6 * abs(loss.item())
    gw = torch.from_numpy(g[f"{case}_grad"]).double()
    assert (grad - gw).abs().max().item() <= 1e-6 * grad.abs().max().item()
    if case == "b":
        assert want[2] == 0.0 and comps[2].item() == 0.0
