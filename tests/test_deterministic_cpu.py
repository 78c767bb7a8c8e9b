"""CPU: the deterministic-mode switch (kernels.deterministic / kernels.deterministic_mode), the --deterministic flag
and the declarations of the *_det entry points in include/lci.h. No GPU and no built library needed."""
import os

import pytest
import torch

from long_context_biomedical_imaging_amd import _lib, config, kernels

DET_SYMBOLS = {
    "lci_ordered_sum": 7,
    "lci_selective_scan_bwd_det": 28, "lci_selective_scan_bwd_det_ws_bytes": 4,
    "lci_hyena_pre_bwd_det": 16, "lci_hyena_pre_bwd_det_ws_bytes": 5,
    "lci_fftconv_bwd_det": 17, "lci_fftconv_bwd_det_ws_bytes": 3,
    "lci_patch_embed_bwd_det": 16, "lci_patch_embed_bwd_det_ws_bytes": 6,
}


@pytest.fixture
def clean(monkeypatch):
    """No source of the mode is on: the environment variable, torch's switch, the override."""
    monkeypatch.delenv("LCI_DETERMINISTIC", raising=False)
    prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(False)
    monkeypatch.setattr(kernels, "_DET_OVERRIDE", False)
    yield monkeypatch
    torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def test_switch_follows_override_environment_and_torch(clean):
    assert kernels.deterministic() is False
    with kernels.deterministic_mode():
        assert kernels.deterministic() is True
    assert kernels.deterministic() is False
    clean.setenv("LCI_DETERMINISTIC", "1")          # read at call time, not at import
    assert kernels.deterministic() is True
    clean.setenv("LCI_DETERMINISTIC", "0")
    assert kernels.deterministic() is False
    torch.use_deterministic_algorithms(True, warn_only=True)
    assert kernels.deterministic() is True
    torch.use_deterministic_algorithms(False)
    assert kernels.deterministic() is False


def test_context_manager_restores_the_previous_state(clean):
    with kernels.deterministic_mode(True):
        with kernels.deterministic_mode(False):
            assert kernels.deterministic() is False
        assert kernels.deterministic() is True       # the inner block restored the outer override
        with kernels.deterministic_mode():
            assert kernels.deterministic() is True
        assert kernels.deterministic() is True
    assert kernels.deterministic() is False
    with pytest.raises(ZeroDivisionError):
        with kernels.deterministic_mode(True):
            assert kernels.deterministic() is True
            1 / 0
    assert kernels.deterministic() is False
    clean.setenv("LCI_DETERMINISTIC", "1")          # flag=False sets no override: the other sources still count
    with kernels.deterministic_mode(False):
        assert kernels.deterministic() is True


def test_deterministic_flag_parses():
    base = ["--optim_type", "sgd", "--loss_func", "MSE"]
    assert config.parse_config(base).deterministic is False
    assert config.parse_config([*base, "--deterministic"]).deterministic is True


def test_train_step_runs_under_the_mode_only_with_the_flag(clean):
    from long_context_biomedical_imaging_amd import trainer
    seen = []

    class Probe(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(3))

        def forward(self, x):
            seen.append(kernels.deterministic())
            return x * self.w

    for flag, want in (([], False), (["--deterministic"], True)):
        cfg = config.parse_config(["--optim_type", "sgd", "--optim.lr", "0.1", "--loss_func", "MSE", *flag])
        step = trainer.TrainStep(Probe(), cfg, torch.device("cpu"), ddp=False)
        step.step(torch.ones(2, 3), torch.zeros(2, 3))
        assert seen.pop() is want
        assert kernels.deterministic() is False      # restored after the step


def test_det_entry_points_are_declared_in_the_header():
    version, sigs = _lib.header()
    assert version >= 42
    for name, nargs in DET_SYMBOLS.items():
        assert name in sigs, f"include/lci.h does not declare {name}"
        assert len(sigs[name][1]) == nargs, (name, len(sigs[name][1]))
    assert os.path.exists(os.path.join(os.path.dirname(kernels.__file__), "csrc", "ordered_sum.hip"))
