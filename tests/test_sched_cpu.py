"""The recipes' LR-scheduler surface on the host: the flag lists parse, trainer.LciOneCycleLR is torch's OneCycleLR
wherever the update kernel is not involved, and TrainStep steps the schedulers where the reference's trainer does
(trainer_base.py:181-182 per update for OneCycleLR, :211-219 per epoch for StepLR / ReduceLROnPlateau)."""
import math
import warnings

import pytest
import torch

# the optimizer / scheduler lines of projects/run_<name>.sh (lines 25-26 and 36-40 of each), as written there
RECIPES = {
    "abct": ["--batch_size", "2", "--num_epochs=250", "--optim_type=adam", "--optim.lr=1e-4", "--optim.beta1=0.9",
             "--optim.beta2=0.99", "--scheduler_type=OneCycleLR"],
    "cmr": ["--batch_size", "16", "--num_epochs=250", "--optim_type=adam", "--optim.lr=1e-5", "--optim.beta1=0.9",
            "--optim.beta2=0.99", "--scheduler_type=OneCycleLR"],
    "emb": ["--batch_size", "4", "--num_epochs=250", "--optim_type=adam", "--optim.lr=1e-5", "--optim.beta1=0.9",
            "--optim.beta2=0.99", "--scheduler_type=OneCycleLR"],
    "micro": ["--batch_size", "4", "--num_epochs=250", "--optim_type=adam", "--optim.lr=1e-5", "--optim.beta1=0.9",
              "--optim.beta2=0.99", "--scheduler_type=OneCycleLR"],
    "ptx": ["--batch_size", "4", "--num_epochs=250", "--optim_type=adam", "--optim.lr=1e-5", "--optim.beta1=0.9",
            "--optim.beta2=0.99", "--scheduler_type", "OneCycleLR"],
    "vessel": ["--batch_size", "4", "--num_epochs=250", "--optim_type=adam", "--optim.lr=1e-3", "--optim.beta1=0.9",
               "--optim.beta2=0.99", "--scheduler_type=OneCycleLR"],
}


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipe_optimizer_and_scheduler_flags_parse(name):
    from long_context_biomedical_imaging_amd import config
    cfg = config.parse_config(RECIPES[name])
    assert cfg.scheduler_type == "OneCycleLR" and cfg.num_epochs == 250
    assert cfg.scheduler.pct_start == 0.3 and cfg.optim.beta2 == 0.99


def test_scheduler_flag_defaults():
    """sched_parser.py's defaults; no scheduler unless one is named (the documented deviation)."""
    from long_context_biomedical_imaging_amd import config
    cfg = config.parse_config([])
    assert cfg.scheduler_type is None and cfg.num_epochs == 50
    s = cfg.scheduler
    assert (s.patience, s.cooldown, s.min_lr, s.factor, s.step_size, s.gamma, s.pct_start) == \
        (0, 0, 1e-8, 0.9, 5, 0.8, 0.3)
    assert config.parse_config(["--scheduler_type", "None"]).scheduler_type is None
    with pytest.raises(SystemExit):
        config.parse_config(["--scheduler_type", "Cosine"])


@pytest.mark.parametrize("n,batch,accum,world,epochs", [(1000, 4, 1, 1, 250), (1001, 4, 1, 8, 250), (7, 2, 3, 1, 5),
                                                        (1, 16, 2, 8, 3), (513, 16, 2, 4, 50)])
def test_compute_total_updates(n, batch, accum, world, epochs):
    from long_context_biomedical_imaging_amd import config
    from long_context_biomedical_imaging_amd.trainer import compute_total_updates
    cfg = config.parse_config(["--batch_size", str(batch), "--iters_to_accumulate", str(accum), "--num_epochs",
                               str(epochs)])
    want = -(-n // (batch * accum * world)) * epochs      # ceil in integers
    assert compute_total_updates(cfg, n, world) == want == int(math.ceil(n / (batch * accum * world)) * epochs)


def _adam():
    p = torch.nn.Parameter(torch.zeros(3))
    return torch.optim.Adam([p], lr=1e-4, betas=(0.9, 0.99))


def _pair(total, pct):
    from long_context_biomedical_imaging_amd.trainer import LciOneCycleLR
    oa, ob = _adam(), _adam()
    a = LciOneCycleLR(oa, max_lr=1e-4, total_steps=total, pct_start=pct, anneal_strategy="cos")
    b = torch.optim.lr_scheduler.OneCycleLR(ob, max_lr=1e-4, total_steps=total, pct_start=pct, anneal_strategy="cos")
    return oa, a, ob, b


def _same(oa, ob):
    ga, gb = oa.param_groups[0], ob.param_groups[0]
    assert ga["lr"] == gb["lr"] and ga["betas"] == gb["betas"], (ga["lr"], gb["lr"], ga["betas"], gb["betas"])


@pytest.mark.parametrize("total,pct", [(10, 0.3), (7, 0.3)])   # (7, 0.3): end_step1 = 1.1, not an integer
def test_lci_onecycle_is_torch_on_cpu_adam_whole_cycle(total, pct):
    oa, a, ob, b = _pair(total, pct)
    assert type(a).__mro__[1] is torch.optim.lr_scheduler.OneCycleLR and oa.__dict__.get("_lci_sched") is None
    _same(oa, ob)
    for _ in range(total):
        oa.step(), ob.step()
        a.step(), b.step()
        _same(oa, ob)
    assert a.last_epoch == b.last_epoch == total
    for s in (a, b):
        with pytest.raises(ValueError, match="Tried to step"):
            s.step()


def test_lci_onecycle_is_torch_at_a_long_schedule():
    oa, a, ob, b = _pair(200000, 0.3)
    oa.step(), ob.step()
    for k in (1, 59999, 60000, 60001, 199999):
        a.last_epoch = b.last_epoch = k - 1
        a.step(), b.step()
        assert a.last_epoch == k
        _same(oa, ob)
    lr, b1 = oa.param_groups[0]["lr"], oa.param_groups[0]["betas"][0]
    assert lr < 1e-4 / 25 and 0.94 < b1 <= 0.95      # the end of the cycle: near min_lr, max_momentum


def test_lci_onecycle_state_dict_moves_between_the_classes():
    oa, a, ob, b = _pair(10, 0.3)
    for _ in range(4):
        oa.step(), ob.step()
        a.step()
    sd = a.state_dict()
    assert set(sd) == set(b.state_dict())
    b.load_state_dict(sd)
    ob.load_state_dict(oa.state_dict())
    assert b.last_epoch == 4
    for _ in range(3):
        oa.step(), ob.step()
        a.step(), b.step()
        _same(oa, ob)
    a.load_state_dict(b.state_dict())
    assert a.last_epoch == 7 and a.get_last_lr() == b.get_last_lr()


def _train_step(flags, total_updates=None, lr="1e-2"):
    from long_context_biomedical_imaging_amd import config
    from long_context_biomedical_imaging_amd.trainer import TrainStep
    torch.manual_seed(0)
    model = torch.nn.Linear(4, 4)
    cfg = config.parse_config(["--optim_type", "adam", "--optim.lr", lr, "--loss_func", "MSE", *flags])
    ts = TrainStep(model, cfg, torch.device("cpu"), ddp=False, total_updates=total_updates)
    x, y = torch.randn(2, 4), torch.randn(2, 4)
    return ts, x, y


def test_train_step_onecycle_steps_once_per_accumulation_window():
    ts, x, y = _train_step(["--scheduler_type", "OneCycleLR", "--iters_to_accumulate", "2"], total_updates=4)
    ref_opt = _adam()
    ref = torch.optim.lr_scheduler.OneCycleLR(ref_opt, max_lr=1e-2, total_steps=4, pct_start=0.3)
    assert ts.sched.last_epoch == 0
    for call in range(1, 7):
        ts.step(x, y)
        assert ts.sched.last_epoch == call // 2
        if call % 2 == 0:
            ref_opt.step(), ref.step()
        assert ts.optim.param_groups[0]["lr"] == ref_opt.param_groups[0]["lr"]
        assert ts.optim.param_groups[0]["betas"][0] == ref_opt.param_groups[0]["betas"][0]
    ts.step(x, y, update=True)                           # the 4th update: the last of the cycle
    with pytest.raises(ValueError, match="Tried to step"):
        ts.step(x, y, update=True)


def test_train_step_onecycle_needs_total_updates():
    with pytest.raises(ValueError, match="total_updates"):
        _train_step(["--scheduler_type", "OneCycleLR"])


def test_train_step_without_scheduler_is_unchanged():
    ts, x, y = _train_step([])
    assert ts.sched is None
    ts.step(x, y)
    ts.end_epoch()
    assert ts.optim.param_groups[0]["lr"] == 1e-2


def test_end_epoch_drives_step_lr():
    ts, x, y = _train_step(["--scheduler_type", "StepLR", "--scheduler.step_size", "2", "--scheduler.gamma", "0.5"])
    ref_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    ref = torch.optim.lr_scheduler.StepLR(ref_opt, step_size=2, gamma=0.5)
    for _ in range(5):
        ts.step(x, y)
        assert ts.optim.param_groups[0]["lr"] == ref_opt.param_groups[0]["lr"]   # a step does not move it
        ts.end_epoch()
        ref_opt.step(), ref.step()
        assert ts.optim.param_groups[0]["lr"] == ref_opt.param_groups[0]["lr"]
    assert ts.optim.param_groups[0]["lr"] == 1e-2 * 0.25


def test_end_epoch_drives_reduce_on_plateau():
    ts, x, y = _train_step(["--scheduler_type", "ReduceLROnPlateau", "--scheduler.patience", "1",
                            "--scheduler.factor", "0.5", "--scheduler.min_lr", "2e-3"])
    ref_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(ref_opt, mode="min", factor=0.5, patience=1, cooldown=0,
                                                     min_lr=2e-3)
    seen = []
    for loss in (1.0, 0.9, 0.95, 0.97, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0):
        ts.step(x, y)
        ts.end_epoch(torch.tensor(loss))
        ref.step(loss)
        seen.append(ts.optim.param_groups[0]["lr"])
        assert seen[-1] == ref_opt.param_groups[0]["lr"]
    assert seen[0] == 1e-2 and seen[-1] == 2e-3          # reduced, then held at min_lr
    with pytest.raises(ValueError):
        ts.end_epoch()


def test_graphed_step_refuses_a_scheduler_without_the_hip_optimizer():
    """A host-float schedule cannot reach a captured update: refused before anything touches a GPU."""
    from long_context_biomedical_imaging_amd.trainer import GraphedStep
    ts, x, y = _train_step(["--scheduler_type", "OneCycleLR"], total_updates=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="LciAdam"):
            GraphedStep(ts, x, y)
