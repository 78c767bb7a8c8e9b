"""GPU: the wide attention-backward dK/dV kernel (attn_bwd_dkdv_hs3_kernel, 96 keys per wave on keys [0, 384 W)) beside
attn_bwd_dkdv_hs_kernel on the remaining keys, the split W forced through kernels.attn_bwd_variant2 (include/lci.h
lci_attn_bwd_variant2), against the narrow kernel alone (W = 0) and the float64 oracle.

Per key both kernels do the same operations in the same order over the queries, so dK and dV must be bitwise those of
W = 0; dQ does not depend on W. Bound against the oracle: the narrow kernel's own measured relative L2 error on the same
inputs, times 1.05 (measured, MI355X; dK | dV, the same for both kernels since they agree bitwise):

    B1 L77  W1: 3.047e-3 | 3.267e-3      B2 L384 W1: 3.025e-3 | 3.079e-3      B1 L449 W1: 2.980e-3 | 2.859e-3
    B2 L833 W2: 3.033e-3 | 3.022e-3      B1 L1000 W1 and W2: 3.083e-3 | 2.979e-3

The entry points take the packed (B, L, 3 H 64) qkv only, whose row, head and batch strides follow from H: q, k and v are
strided views of it in every case (rows 3 H 64 apart, heads 64 apart), B = 2 adds the batch stride. Every call writes
into a buffer with guard rows behind it: a key block at or past L must store nothing."""
import functools

import pytest
import torch

from golden_util import rel_err
from oracle import attention as oatt

pytestmark = pytest.mark.gpu

SCALE = 0.125
H = 2
GUARD = 4096   # bf16 elements behind dqkv
CASES = [(1, 77, 1),      # one ragged wide workgroup: wave 0's third key block ragged, waves 1-3 past L
         (2, 384, 1),     # exactly one full wide workgroup, no narrow launch
         (1, 449, 1),     # wide plus a ragged narrow remainder
         (2, 833, 2),     # two wide workgroups plus remainder; 14 query tiles: the run-time ring-slot remainder path
         (1, 1000, 1),    # both splits of one input
         (1, 1000, 2)]


@functools.lru_cache(maxsize=None)
def _case(B, L):
    """Seeded inputs, the forward on the GPU (its out / lse2 feed the backward, as in training), the float64 oracle's
    gradients and the backward with the narrow dK/dV kernel alone: computed once per (B, L), shared, never modified."""
    from long_context_biomedical_imaging_amd import kernels
    g = torch.Generator().manual_seed(4100 + 3 * L + B)
    qkv = torch.randn(B, L, 3 * H * 64, generator=g).to(torch.bfloat16)
    dout = torch.randn(B, L, H * 64, generator=g).to(torch.bfloat16)
    x, dy = qkv.cuda(), dout.cuda()
    out, lse2 = kernels.attn_fwd(x, H, SCALE)
    xd = qkv.double().requires_grad_(True)
    q, k, v = oatt.split_qkv(xd, H)
    o, _ = oatt.attention_core(q, k, v, SCALE)
    (o.permute(0, 2, 1, 3).reshape(B, L, -1) * dout.double()).sum().backward()
    c = dict(x=x, dy=dy, out=out, lse2=lse2, ref=xd.grad)
    c["g0"] = _run(c, B, L, 0)
    return c


def _run(c, B, L, W):
    """One backward with the split forced, into a buffer with a guard behind it; returns dqkv on the host."""
    from long_context_biomedical_imaging_amd import kernels
    n = B * L * 3 * H * 64
    buf = torch.full((n + GUARD,), 7.0, dtype=torch.bfloat16, device="cuda")
    dqkv = buf[:n].view(B, L, 3 * H * 64)
    kernels.attn_bwd_variant2(c["x"], c["out"], c["dy"], c["lse2"], H, SCALE, -1, W, dqkv=dqkv)
    torch.cuda.synchronize()
    assert (buf[n:] == 7.0).all(), f"W={W}: stores behind dqkv"
    return dqkv.cpu()


@pytest.mark.parametrize("B,L,W", CASES)
def test_split_is_bitwise_the_narrow_kernel_and_keeps_its_oracle_error(B, L, W):
    c = _case(B, L)
    C = H * 64
    g0, gw = c["g0"], _run(c, B, L, W)
    assert torch.isfinite(gw.float()).all()
    assert torch.equal(gw[..., C:2 * C], g0[..., C:2 * C]), "dK differs from the narrow kernel's"
    assert torch.equal(gw[..., 2 * C:], g0[..., 2 * C:]), "dV differs from the narrow kernel's"
    assert torch.equal(gw[..., :C], g0[..., :C]), "dQ depends on the dK/dV split"
    for i, nm in ((1, "dK"), (2, "dV")):
        r = c["ref"][..., i * C:(i + 1) * C]
        e0, ew = rel_err(g0[..., i * C:(i + 1) * C].double(), r), rel_err(gw[..., i * C:(i + 1) * C].double(), r)
        print(f"{nm} B{B} L{L} W{W}: rel L2 against the oracle: narrow {e0:.3e} split {ew:.3e}")
        assert 0.0 < e0 < 1e-2, f"{nm}: the narrow kernel itself is off ({e0:.3e})"
        assert ew <= 1.05 * e0, f"{nm}: split {ew:.3e} against the narrow kernel's {e0:.3e}"


def test_split_deterministic():
    c = _case(2, 833)
    assert torch.equal(_run(c, 2, 833, 2), _run(c, 2, 833, 2))


def test_forced_split_must_start_inside_the_keys():
    from long_context_biomedical_imaging_amd import _lib, kernels
    c = _case(1, 77)
    with pytest.raises(_lib.LciError):
        kernels.attn_bwd_variant2(c["x"], c["out"], c["dy"], c["lse2"], H, SCALE, -1, 2)


def test_default_entry_follows_the_pick_rule():
    """lci_attn_bwd splits as lci_attn_bwd_dkdv_pick says for the device: 0 at these small shapes, so the narrow
    kernel's launch alone; at B H = 256 and L = 384 on a device of up to 256 compute units the wide kernel alone. Either
    way the result is W = 0's bitwise."""
    from long_context_biomedical_imaging_amd import _lib, kernels
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    pick = _lib.load().lci_attn_bwd_dkdv_pick
    c = _case(1, 449)
    assert pick(1, 449, H, n_cu) == 0
    assert torch.equal(kernels.attn_bwd(c["x"], c["out"], c["dy"], c["lse2"], H, SCALE).cpu(), c["g0"])
    B, Hh, L = 4, 64, 384
    if pick(B, L, Hh, n_cu) != 1:
        return   # (a device of more than 256 compute units: nothing more to compare)
    g = torch.Generator().manual_seed(65)
    x = torch.randn(B, L, 3 * Hh * 64, generator=g).to(torch.bfloat16).cuda()
    dy = torch.randn(B, L, Hh * 64, generator=g).to(torch.bfloat16).cuda()
    out, lse2 = kernels.attn_fwd(x, Hh, SCALE)
    gd = kernels.attn_bwd(x, out, dy, lse2, Hh, SCALE)
    g0 = kernels.attn_bwd_variant2(x, out, dy, lse2, Hh, SCALE, -1, 0)
    g1 = kernels.attn_bwd_variant2(x, out, dy, lse2, Hh, SCALE, -1, 1)
    assert torch.equal(gd, g1) and torch.equal(gd, g0)
