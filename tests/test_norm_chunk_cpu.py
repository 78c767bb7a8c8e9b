"""CPU: the two host rules that decide how the normalisation kernels split their work, against restatements.
lci_inorm_chunks(V, B) chooses the voxel chunks of the instance-norm / BatchNorm reductions (about 2048 workgroups in
total, at least 256 voxels per chunk); the callers then use chunk = ceil(V / nchunk), which leaves trailing chunks
without a voxel once nchunk is capped. lci_layernorm_bwd_blocks(rows) chooses the workgroups of the LayerNorm backward
(16 rows per wave, 4 waves per workgroup, at most 2048). tests/test_norm_kernel_gpu.py reaches its regimes through
these rules; the shapes it names for the empty-chunk regime are checked here to really have empty chunks."""
import pytest

from long_context_biomedical_imaging_amd import _lib

from test_norm_kernel_gpu import INORM, REGIME, _chunks, _regime


def _ln_blocks(rows):
    waves = -(-rows // 16)
    return max(1, min(2048, -(-waves // 4)))


VS = [1, 2, 27, 255, 256, 257, 511, 512, 513, 990, 16384, 16385, 75008, 75009, 524287, 524288, 524289, 1 << 24,
      (1 << 31) + 5]
BS = [1, 2, 3, 4, 7, 8, 683, 1024, 2047, 2048, 2049, 5000]


@pytest.mark.parametrize("B", BS)
def test_inorm_chunks_rule(B):
    lib = _lib.load()
    for V in VS:
        n = lib.lci_inorm_chunks(V, B)
        assert n == _chunks(V, B), (V, B)
        chunk = -(-V // n)
        assert 1 <= n <= 2048 and n * chunk >= V
        assert chunk <= 256 or n == -(-2048 // B), "only a capped split has chunks above 256 voxels"


def test_inorm_chunks_landmarks():
    lib = _lib.load()
    assert lib.lci_inorm_chunks(1, 1) == 1 and lib.lci_inorm_chunks(256, 1) == 1 and lib.lci_inorm_chunks(257, 1) == 2
    assert lib.lci_inorm_chunks(1 << 30, 1) == 2048 and lib.lci_inorm_chunks(1 << 30, 3) == 683
    assert lib.lci_inorm_chunks(1 << 30, 4096) == 1


@pytest.mark.parametrize("name", list(INORM))
def test_inorm_kernel_test_cases_reach_their_regimes(name):
    """Every case of test_norm_kernel_gpu.py is in the regime its table names; empty1 and empty7 have empty chunks."""
    B, V, C = INORM[name]
    got = _regime(B, V, C, _lib.load().lci_inorm_chunks(V, B))
    assert {k: got[k] for k in REGIME[name]} == REGIME[name], got
    if name in ("empty1", "empty7"):
        assert got["empty"] > 0 and (got["nchunk"] - got["empty"]) * got["chunk"] >= V
        assert (got["nchunk"] - got["empty"] - 1) * got["chunk"] < V
    else:
        assert got["empty"] == 0


def test_layernorm_bwd_blocks_rule():
    lib = _lib.load()
    for rows in list(range(0, 200)) + [1023, 1024, 1025, 4099, 131071, 131072, 131073, 1 << 20, (1 << 31) + 7]:
        assert lib.lci_layernorm_bwd_blocks(rows) == _ln_blocks(rows), rows
    assert _ln_blocks(3) == 1 and _ln_blocks(64) == 1 and _ln_blocks(65) == 2 and _ln_blocks(131073) == 2048
