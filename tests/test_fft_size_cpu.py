"""lci_fft_size on a CPU-only host (no compute call: the plan is host arithmetic): n = 2^ceil(log2(2L)) for every
supported row length, -1 outside 1..262144."""
import os

import pytest


def _lib():
    from long_context_biomedical_imaging_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liblci.so not built (python -m long_context_biomedical_imaging_amd.build_lib)")
    return _lib.load()


def test_fft_size_is_the_power_of_two_at_or_above_2L():
    lib = _lib()
    Ls = set(range(1, 70001, 997))
    for i in range(19):
        Ls.update(L for L in (1 << i, (1 << i) + 1) if L <= 262144)
    assert {1, 2, 3, 131072, 131073, 262144} <= Ls
    for L in sorted(Ls):
        n = 1
        while n < 2 * L:
            n *= 2
        assert lib.lci_fft_size(L) == n, L


@pytest.mark.parametrize("L", [0, -1, -262144, 262145, 1 << 19, 2 ** 31 - 1])
def test_fft_size_refuses_unsupported_lengths(L):
    assert _lib().lci_fft_size(L) == -1
