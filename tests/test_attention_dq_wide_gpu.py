"""GPU: the wide attention-backward dQ kernel (attn_bwd_dq_hs4_kernel, 128 queries per wave, one shared softmax
reference per lane) against the float64 oracle and the narrow kernel (attn_bwd_dq_hs_kernel), the dQ kernel forced
through kernels.attn_bwd_variant (include/lci.h lci_attn_bwd_variant).

Bound against the oracle: the project's own for the attention kernels (tests/test_attention_gpu.py::_check), relative
L2 <= 1e-2 and max |err| <= 2e-2 max|ref| + 2e-3. The wide kernel rounds the same quantities as the narrow one (q~ and
dS^T to bf16, the latter scaled by the per-query power-of-two-ish factor 2^(lse2_q - u) that the epilogue takes out
again), so both sit at a relative L2 of about 2.5e-3; each test prints the narrow kernel's error beside the wide one's.
dK and dV (one kernel under either dQ variant) are compared with the oracle at the bounds of
tests/test_attention_gpu.py::test_attention_backward: relative L2 <= 2e-2 and max |err| <= 3e-2 max|ref| + 2e-3.
"""
import functools

import pytest
import torch

from golden_util import rel_err
from oracle import attention as oatt

pytestmark = pytest.mark.gpu

SCALE = 0.125
NARROW, WIDE = 0, 1
SHAPES = [(1, 1, 512),     # one workgroup, eight key tiles
          (1, 1, 77),      # one ragged workgroup, ragged keys
          (1, 2, 300),     # 5 key tiles: nkt % 4 == 1, three padded tiles
          (2, 3, 1100)]    # several workgroups, a ragged last one, batch and head strides


def _inputs(B, H, L, hot):
    """Seeded randn qkv / dout; hot != 0 replaces the queries with index % 128 in [32, 64) (query block 1 of every
    wave of the wide kernel) by hot * k_0, the first key of their head: their lse2 stands far above their lane's other
    three queries'."""
    g = torch.Generator().manual_seed(9000 + 7 * L + H)
    qkv = torch.randn(B, L, 3 * H * 64, generator=g)
    dout = torch.randn(B, L, H * 64, generator=g).to(torch.bfloat16)
    if hot:
        C = H * 64
        idx = torch.arange(L)
        sel = (idx % 128 >= 32) & (idx % 128 < 64)
        k0 = qkv[:, 0, C:2 * C].to(torch.bfloat16).float()
        qkv[:, sel, 0:C] = hot * k0[:, None, :]
    return qkv.to(torch.bfloat16), dout


@functools.lru_cache(maxsize=None)
def _case(B, H, L, hot=0.0):
    """The forward on the GPU (its out / lse2 feed the backward, as in training), the float64 oracle's dQ, and the
    backward with either dQ kernel: computed once per case, shared by the tests, never modified."""
    from long_context_biomedical_imaging_amd import kernels
    qkv, dout = _inputs(B, H, L, hot)
    x, dy = qkv.cuda(), dout.cuda()
    out, lse2 = kernels.attn_fwd(x, H, SCALE)
    xd = qkv.double().requires_grad_(True)
    q, k, v = oatt.split_qkv(xd, H)
    o, _ = oatt.attention_core(q, k, v, SCALE)
    (o.permute(0, 2, 1, 3).reshape(B, L, -1) * dout.double()).sum().backward()
    gn, _ = kernels.attn_bwd_variant(x, out, dy, lse2, H, SCALE, NARROW)
    gw, flags = kernels.attn_bwd_variant(x, out, dy, lse2, H, SCALE, WIDE)
    torch.cuda.synchronize()
    return dict(x=x, out=out, lse2=lse2, dy=dy, ref=xd.grad[..., :H * 64].clone(), ref_all=xd.grad, gn=gn.cpu(),
                gw=gw.cpu(), flags=flags.cpu().clone(), C=H * 64)


def _check(a, b, what, rel=1e-2, absf=2e-2):
    """tests/test_attention_gpu.py::_check, at its default bounds unless given."""
    a, b = a.float().cpu(), b.float().cpu()
    re = rel_err(a, b)
    mx = (a - b).abs().max().item()
    assert re <= rel, f"{what}: rel L2 err {re:.3e}"
    assert mx <= absf * b.abs().max().item() + 2e-3, f"{what}: max err {mx:.3e} (max|ref| {b.abs().max():.3e})"


def _report(c, what):
    C, ref = c["C"], c["ref"]
    for nm, g in (("wide", c["gw"]), ("narrow", c["gn"])):
        d = g[..., :C].double()
        print(f"{what} {nm}: rel L2 {rel_err(d, ref):.3e} max err {(d - ref).abs().max().item():.3e} "
              f"(max|ref| {ref.abs().max().item():.3e})")


@pytest.mark.parametrize("B,H,L", SHAPES)
def test_wide_dq_against_the_oracle(B, H, L):
    c = _case(B, H, L)
    C = c["C"]
    _report(c, f"dQ B{B} H{H} L{L}")
    assert torch.isfinite(c["gw"].float()).all()
    assert (c["flags"] == 0).all(), "random data: no workgroup may leave the wide stream"
    _check(c["gw"][..., :C], c["ref"], f"wide dQ B{B} H{H} L{L}")
    # dK and dV do not depend on the dQ kernel
    assert torch.equal(c["gw"][..., C:], c["gn"][..., C:]), "dK / dV differ between the dQ variants"
    # ... and keep the oracle bound of tests/test_attention_gpu.py::test_attention_backward (2e-2, 3e-2 max|ref| + 2e-3)
    for i, nm in ((1, "dK"), (2, "dV")):
        g, r = c["gw"][..., i * C:(i + 1) * C].double(), c["ref_all"][..., i * C:(i + 1) * C]
        print(f"{nm} B{B} H{H} L{L}: rel L2 {rel_err(g, r):.3e} max err {(g - r).abs().max().item():.3e} "
              f"(max|ref| {r.abs().max().item():.3e})")
        _check(g, r, f"{nm} B{B} H{H} L{L}", rel=2e-2, absf=3e-2)


def test_narrow_dq_padded_tiles_against_the_oracle():
    """nkt % 4 == 1 for the 64-queries-per-wave kernel: three key tiles past L read as zero rows."""
    c = _case(1, 2, 300)
    _check(c["gn"][..., :c["C"]], c["ref"], "narrow dQ B1 H2 L300")


def _lane_spread(lse2):
    """Largest lse2 spread within a lane of the wide kernel: queries q, q + 32, q + 64, q + 96 of each 128."""
    B, H, L = lse2.shape
    assert L % 128 == 0
    v = lse2.cpu().view(B, H, L // 128, 4, 32)
    return (v.amax(3) - v.amin(3)).max().item()


def test_shared_reference_under_stress():
    """Every lane holds one query whose lse2 lies about 29 above its other three: still below the guard's 64, so the
    shared reference carries factors down to 2^-29 through the bf16 dS^T packs. No workgroup is flagged and the oracle
    bound holds."""
    c = _case(1, 2, 512, 3.0)
    spread = _lane_spread(c["lse2"])
    print(f"lane spread {spread:.1f}")
    assert 16.0 < spread < 64.0, f"input does not stress the shared reference below the guard: spread {spread:.1f}"
    _report(c, "dQ stress")
    assert (c["flags"] == 0).all()
    _check(c["gw"][..., :c["C"]], c["ref"], "wide dQ, lane spread ~ 29")


def test_guard_hands_flagged_workgroups_to_the_narrow_stream():
    """The same input with 9 k_0: a spread of about 94 in every lane. Every workgroup (all hold such queries) is
    flagged, and its dQ is the narrow kernel's bitwise."""
    c = _case(1, 2, 512, 9.0)
    spread = _lane_spread(c["lse2"])
    print(f"lane spread {spread:.1f}")
    assert spread > 64.0
    assert (c["flags"] == 1).all(), f"flags {c['flags'].flatten().tolist()}"
    assert torch.isfinite(c["gw"].float()).all()
    assert torch.equal(c["gw"], c["gn"])


def test_guard_is_per_workgroup():
    """L = 1100 with hot queries only below 512: workgroup 0 of every (b, h) is flagged, the others stay wide; the
    flagged queries get the narrow kernel's dQ bitwise, all of dQ keeps the oracle bound."""
    from long_context_biomedical_imaging_amd import kernels
    B, H, L = 1, 2, 1100
    qkv, dout = _inputs(B, H, L, 0.0)
    C = H * 64
    k0 = qkv[:, 0, C:2 * C].float()
    qkv[:, 32:64, 0:C] = (9.0 * k0[:, None, :]).to(torch.bfloat16)
    x, dy = qkv.cuda(), dout.cuda()
    out, lse2 = kernels.attn_fwd(x, H, SCALE)
    gn, _ = kernels.attn_bwd_variant(x, out, dy, lse2, H, SCALE, NARROW)
    gw, flags = kernels.attn_bwd_variant(x, out, dy, lse2, H, SCALE, WIDE)
    assert flags.cpu().tolist() == [[[1, 0, 0]] * H] * B
    assert torch.equal(gw[:, :512], gn[:, :512])
    assert torch.equal(gw[..., C:], gn[..., C:])
    assert rel_err(gw[:, 512:, :C], gn[:, 512:, :C]) <= 1e-2


def test_wide_deterministic():
    from long_context_biomedical_imaging_amd import kernels
    c = _case(2, 3, 1100)
    g2, _ = kernels.attn_bwd_variant(c["x"], c["out"], c["dy"], c["lse2"], 3, SCALE, WIDE)
    assert torch.equal(g2.cpu(), c["gw"])


def test_default_entry_follows_the_pick_rule():
    """lci_attn_bwd runs the dQ kernel of lci_attn_bwd_dq_pick for the device's compute-unit count: bitwise variant 1
    where the 512-query grid fills the chip (B 4, H 64, L 512: 256 workgroups), bitwise variant 0 at a small shape."""
    from long_context_biomedical_imaging_amd import _lib, kernels
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    pick = _lib.load().lci_attn_bwd_dq_pick
    B, H, L = 4, 64, 512
    assert pick(B, L, H, n_cu) == 1, f"B{B} H{H} L{L} does not fill a device of {n_cu} compute units"
    g = torch.Generator().manual_seed(64)
    x = torch.randn(B, L, 3 * H * 64, generator=g).to(torch.bfloat16).cuda()
    dy = torch.randn(B, L, H * 64, generator=g).to(torch.bfloat16).cuda()
    out, lse2 = kernels.attn_fwd(x, H, SCALE)
    gd = kernels.attn_bwd(x, out, dy, lse2, H, SCALE)
    gw, flags = kernels.attn_bwd_variant(x, out, dy, lse2, H, SCALE, WIDE)
    assert (flags == 0).all()
    assert torch.equal(gd, gw)
    c = _case(1, 2, 300)
    assert pick(1, 300, 2, n_cu) == 0
    gd = kernels.attn_bwd(c["x"], c["out"], c["dy"], c["lse2"], 2, SCALE)
    assert torch.equal(gd.cpu(), c["gn"])
