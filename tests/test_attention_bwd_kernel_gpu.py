"""GPU: the global-attention backward kernels (csrc/attention.hip: attn_bwd_delta_kernel, attn_bwd_dkdv_hs_kernel,
attn_bwd_dq_hs_kernel, attn_bwd_dq_hs4_kernel + attn_bwd_dq_hsfb_kernel) called one stage at a time through
kernels.attn_bwd_variant, against the fp64 oracle (oracle.attention.split_qkv / attention_core with autograd).

Inputs: bf16 qkv ~ N(0,1), bf16 cotangent ~ N(0,1), scale 0.125, head_dim 64, one seeded generator per case; the fp64
reference sees the bf16-rounded values. Every case runs in two feeding modes:
  isolated    out = bf16(O_fp64), lse2 = f32(lse_fp64 * log2 e), built on the CPU from the oracle: only the backward's
              own arithmetic is compared with the exact gradient (a forward change cannot move these figures, and a
              backward error cannot hide behind a forward one);
  as-trained  out, lse2 from kernels.attn_fwd, as in training (lse2 carries the forward's bf16-P denominator).

Shapes (CASES): L chosen by the kernels' structure. nqt = ceil(L / 64) query tiles feed the dK/dV kernel's 4-slot
Q / dO ring: a 4-tile unrolled loop, then a run-time-slot tail (nqt 1, 2, 3: tail only; 4: one group, no tail; 5, 6, 7:
group + tail 1, 2, 3; 9, 10: two groups + tail). A dK/dV workgroup is 256 keys (4 waves x two 32-key blocks), a narrow
dQ workgroup 256 queries, a wide one 512, and dQ pads its key loop to a multiple of 4 tiles. The dominant-key cases
replace the queries with index % 64 in [0, 32) by 3 k_j (j in the first key tile / j = L - 1): the test asserts from
the reference alone that those rows put >= 1 - 1e-4 of their softmax mass on key j.

Numeric bounds, every one from the reference side:
  whole tensor   each of dQ, dK, dV: rel-L2 <= 2e-2 and max|err| <= 3e-2 max|ref| + 2e-3, the project's attention
                 backward bounds (test_attention_gpu.py::test_attention_backward). Where the reference is identically
                 zero (L = 1: one key, so dS = 0 and dQ = dK = 0 exactly) a relative error has no meaning and the
                 absolute bound alone applies.
  per row        for each (b, h, token) row of dQ, dK, dV: ||err|| <= bound * max(||ref row||, 0.1 mean ||ref row||)
                 + allowance (the form of test_window_kernel_gpu.py), bound = max(5e-2, 2 x the worst row of torch's
                 own bf16-autocast evaluation of the same op on the same inputs, measured the same way against the same
                 fp64 reference; 5e-2 is the window test's floor).
  allowance      derived, not measured: out is stored in bf16 (unit roundoff u = 2^-8), so delta_i = sum_d dO_id O_id
                 can be off by e_i = u sum_d |dO_id O_id| in ANY evaluation that reads a bf16 out. That moves dQ row i
                 by at most scale e_i ||sum_j P_ij k_j|| and dK row j by at most scale sum_i P_ij e_i ||q_i||; dV does
                 not depend on delta. Both are computed in fp64 from the reference's P, O, q, k. On ordinary rows the
                 term is small beside the row norm; on the planted rows the true gradient is of the order of the
                 softmax's remaining mass (1e-4 and less) and the term is all there is to compare against
                 (test_window_kernel_gpu.py, PLANT comment).
  delta stage    ws[b][h][0][:] == -lse2 bitwise; |ws[b][h][1][q] - (-sum_d dO O)| <= 64 * 2^-24 * sum_d |dO O| with
                 the sum in fp64 over the bf16 out actually passed (products of two bf16 are exact in f32; only the
                 64-term f32 sum rounds, at most 63 additions of relative error 2^-24 each).
The two modes are not compared with each other: each satisfies the bounds on its own.

Exact checks: dqkv and ws are views into larger buffers with 64-element guard bands; dqkv is pre-filled with NaN.
After stage 1 alone the K and V thirds are finite and the Q third is still all NaN; after stage 2 (either variant) into
a fresh buffer the Q third is finite and the K / V thirds are all NaN; the guard bands stay intact; stage 1 and the
narrow dQ kernel leave ws bitwise unchanged and the wide one changes only its flag words; a (b, h) slice repacked as
a B1 H1 problem gives the batched run's slice bit for bit (both dQ variants), with flags == 0 on random data; stages
0, 1, 2 one after another equal one stage = -1 call bitwise; two runs (over differently pre-filled buffers) agree bit
for bit.

Measured on an MI355X, both against fp64 (worst row: the largest of dQ narrow, dQ wide, dK, dV, allowance taken off;
max err / allowed: the largest max|err| / (3e-2 max|ref| + 2e-3) of the four; the row bound was 5e-2 everywhere, 2 x the
autocast worst row never exceeding it; the delta stage used at most 1.6 % of its bound; every exact check held bit for
bit). "(0)": the reference is identically zero (L = 1). Ordinary cases: the kernels sit at 3e-3, autocast at 4.5e-3,
and the two modes do not differ. Dominant key: dQ and dK keep 3e-3; dV rises to 5e-3 .. 1.1e-2 (autocast 1.6e-3), all
of it in the planted key's own dV row (max|ref| 27 .. 49, max err 0.24 .. 0.64). In isolated mode that is the dK/dV
kernel's bf16 rounding of k~ = scale log2(e) k: at a logit of ~35 (log2 units) it moves the planted P by up to 0.9 %,
the same way for every planted query, and with lse2 given the backward cannot renormalise (an fp64 evaluation with this
one rounding gives 5.7e-3 / 6.1e-3 at L257_plant_first / L577_plant_last, the kernel 5.9e-3 / 6.8e-3). As trained, the
forward's lse2 (bf16 q~ logits, sum of bf16-rounded P) adds to it only where the planted key is the last one
(L577_plant_last: 6.8e-3 -> 1.1e-2, max err 0.39 -> 0.64 of 48.5); elsewhere the two modes agree to 2e-4.
                              kernel rel-L2                      autocast rel-L2           worst row           max err
case              mode        dQ nar. dQ wide dK      dV         dQ      dK      dV        kernel  | autocast  / allowed
L1                isolated      (0)     (0)     (0)   0.0e+00      (0)     (0)   0.0e+00   0.0e+00 | 0.0e+00   0.00
L1                as_trained    (0)     (0)     (0)   0.0e+00      (0)     (0)   0.0e+00   0.0e+00 | 0.0e+00   0.00
L33               isolated    3.1e-03 3.1e-03 3.0e-03 3.0e-03    4.0e-03 4.1e-03 3.8e-03   5.1e-03 | 6.5e-03   0.14
L33               as_trained  2.9e-03 2.9e-03 3.1e-03 2.9e-03    4.0e-03 4.1e-03 3.8e-03   5.1e-03 | 6.5e-03   0.14
L64               isolated    2.9e-03 2.9e-03 3.2e-03 2.9e-03    4.0e-03 4.0e-03 3.5e-03   4.0e-03 | 6.4e-03   0.15
L64               as_trained  2.8e-03 2.9e-03 3.3e-03 2.9e-03    4.0e-03 4.0e-03 3.5e-03   3.9e-03 | 6.4e-03   0.15
L65               isolated    2.9e-03 2.8e-03 3.2e-03 3.1e-03    3.8e-03 3.9e-03 4.7e-03   4.7e-03 | 9.0e-03   0.15
L65               as_trained  2.8e-03 2.7e-03 3.2e-03 3.1e-03    3.8e-03 3.9e-03 4.7e-03   5.5e-03 | 9.0e-03   0.15
L130              isolated    2.8e-03 2.8e-03 3.0e-03 2.9e-03    4.3e-03 4.3e-03 4.0e-03   5.3e-03 | 6.5e-03   0.14
L130              as_trained  2.8e-03 2.7e-03 3.1e-03 2.9e-03    4.3e-03 4.3e-03 4.0e-03   5.2e-03 | 6.5e-03   0.14
L256              isolated    3.0e-03 2.9e-03 3.0e-03 2.9e-03    4.5e-03 4.6e-03 4.0e-03   5.3e-03 | 9.5e-03   0.11
L256              as_trained  2.9e-03 2.9e-03 3.0e-03 2.9e-03    4.5e-03 4.6e-03 4.0e-03   5.4e-03 | 9.5e-03   0.11
L257              isolated    3.2e-03 3.2e-03 2.9e-03 2.9e-03    4.4e-03 4.4e-03 4.0e-03   4.7e-03 | 6.7e-03   0.20
L257              as_trained  2.9e-03 2.9e-03 3.0e-03 2.9e-03    4.4e-03 4.4e-03 4.0e-03   4.6e-03 | 6.7e-03   0.17
L383              isolated    3.1e-03 3.1e-03 3.0e-03 3.0e-03    4.5e-03 4.7e-03 4.6e-03   5.6e-03 | 1.2e-02   0.16
L383              as_trained  3.0e-03 3.0e-03 3.0e-03 3.0e-03    4.5e-03 4.7e-03 4.6e-03   5.3e-03 | 1.2e-02   0.16
L448              isolated    3.0e-03 3.0e-03 3.0e-03 3.1e-03    4.4e-03 4.5e-03 4.5e-03   6.3e-03 | 9.7e-03   0.12
L448              as_trained  2.9e-03 2.9e-03 3.0e-03 3.1e-03    4.4e-03 4.5e-03 4.5e-03   6.1e-03 | 9.7e-03   0.11
L513              isolated    3.0e-03 3.0e-03 3.0e-03 3.0e-03    4.4e-03 4.5e-03 4.3e-03   5.0e-03 | 1.0e-02   0.16
L513              as_trained  2.9e-03 2.9e-03 3.0e-03 3.0e-03    4.4e-03 4.5e-03 4.3e-03   4.7e-03 | 1.0e-02   0.12
L577_b2h3         isolated    3.1e-03 3.1e-03 3.0e-03 3.0e-03    4.6e-03 4.6e-03 4.4e-03   7.0e-03 | 1.3e-02   0.21
L577_b2h3         as_trained  2.9e-03 2.9e-03 3.0e-03 3.0e-03    4.6e-03 4.6e-03 4.4e-03   7.2e-03 | 1.3e-02   0.22
L257_plant_first  isolated    3.3e-03 3.4e-03 3.4e-03 5.9e-03    4.7e-03 4.7e-03 1.6e-03   8.0e-03 | 1.0e-02   0.27
L257_plant_first  as_trained  3.1e-03 3.1e-03 3.4e-03 5.9e-03    4.7e-03 4.7e-03 1.6e-03   8.0e-03 | 1.0e-02   0.27
L257_plant_last   isolated    2.9e-03 3.1e-03 2.9e-03 6.6e-03    4.4e-03 4.6e-03 1.6e-03   8.6e-03 | 9.3e-03   0.29
L257_plant_last   as_trained  2.8e-03 2.8e-03 3.0e-03 6.7e-03    4.4e-03 4.6e-03 1.6e-03   8.0e-03 | 9.3e-03   0.33
L577_plant_first  isolated    3.0e-03 3.0e-03 3.0e-03 4.9e-03    4.5e-03 4.5e-03 1.6e-03   7.4e-03 | 1.1e-02   0.20
L577_plant_first  as_trained  2.9e-03 2.9e-03 3.0e-03 5.0e-03    4.5e-03 4.5e-03 1.6e-03   7.5e-03 | 1.1e-02   0.31
L577_plant_last   isolated    3.0e-03 3.1e-03 3.0e-03 6.8e-03    4.6e-03 4.5e-03 1.7e-03   8.6e-03 | 1.2e-02   0.27
L577_plant_last   as_trained  3.0e-03 2.9e-03 3.0e-03 1.1e-02    4.6e-03 4.5e-03 1.7e-03   1.6e-02 | 1.2e-02   0.44
"""
import functools

import pytest
import torch

from golden_util import rel_err
from oracle import attention as oatt

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LOG2E = 1.4426950408889634
SCALE = 0.125
DH = 64
U_BF16 = 2.0 ** -8
GUARD = 64            # guard-band elements on either side (128 B of bf16, 256 B of int32: keeps the alignment)
SENTINEL = -7         # exact in bf16 and int32
WS_NAN = 0x7FC00000   # int32 pre-fill of the workspace: a NaN when read as f32
WS_THREE = 0x40400000  # ... and 3.0f for the second run of the determinism check
NARROW, WIDE = 0, 1
MODES = ("isolated", "as_trained")

# name -> (B, H, L, planted key or None)
CASES = {
    "L1": (1, 1, 1, None),               # one key, one query
    "L33": (1, 1, 33, None),             # key block 1 holds a single key; ragged half-tile
    "L64": (1, 1, 64, None),             # exact tile; waves 1-3 hold no key
    "L65": (1, 1, 65, None),             # nqt 2; wave 1 holds one key
    "L130": (1, 1, 130, None),           # nqt 3: tail only, tail of 3
    "L256": (1, 1, 256, None),           # nqt 4: one unrolled group, no tail, one full workgroup
    "L257": (1, 1, 257, None),           # nqt 5: group + tail 1; second workgroup with one key; dQ pads 3 tiles
    "L383": (1, 1, 383, None),           # nqt 6: tail 2, ragged
    "L448": (1, 1, 448, None),           # nqt 7: tail 3, exact tiles
    "L513": (1, 1, 513, None),           # nqt 9: two groups + tail 1; third workgroup; 2nd wide-dQ workgroup, 1 query
    "L577_b2h3": (2, 3, 577, None),      # nqt 10: two groups + tail 2; batch and head strides
    "L257_plant_first": (1, 2, 257, 5),  # dominant key in the first key tile
    "L257_plant_last": (1, 2, 257, 256),  # ... and the last key (alone in its tile and workgroup)
    "L577_plant_first": (1, 2, 577, 5),
    "L577_plant_last": (1, 2, 577, 576),
}
PLANT_MASS = 1.0 - 1e-4


# ------------------------------------------------------------------------------------------------ oracle side (CPU)
def _planted_rows(L):
    return torch.arange(L) % 64 < 32


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """CPU f32 tensors holding bf16-representable qkv (B, L, 3C) and cotangent (B, L, C)."""
    B, H, L, plant = CASES[name]
    C = H * DH
    g = torch.Generator().manual_seed(4000 + list(CASES).index(name))
    qkv = torch.randn(B, L, 3 * C, generator=g).to(BF16).float()
    cot = torch.randn(B, L, C, generator=g).to(BF16).float()
    if plant is not None:   # as test_attention_dq_wide_gpu.py::_inputs plants them: 3 x one key of the head
        kj = qkv[:, plant, C:2 * C]
        qkv[:, _planted_rows(L), 0:C] = (3.0 * kj[:, None, :]).to(BF16).float()
    return dict(qkv=qkv, cot=cot, B=B, H=H, L=L, C=C, plant=plant)


def _rows_bhl(t):
    """(B, H, L) -> (B, L, H) flattened: the order of the (b, token, h) rows of a (B, L, H * 64) tensor."""
    return t.permute(0, 2, 1).reshape(-1)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """fp64 on the CPU: out (B, L, C), lse (B, H, L), d(qkv), the planted rows' softmax mass on the planted key and
    the delta allowances of the dQ / dK rows. Computed once per case, never modified."""
    inp = _inputs(name)
    B, H, L, C = inp["B"], inp["H"], inp["L"], inp["C"]
    x = inp["qkv"].double().requires_grad_(True)
    q, k, v = oatt.split_qkv(x, H)
    o, lse = oatt.attention_core(q, k, v, SCALE)
    out = o.permute(0, 2, 1, 3).reshape(B, L, C)
    out.backward(inp["cot"].double())
    with torch.no_grad():
        p = (torch.einsum("bhxd,bhyd->bhxy", q, k) * SCALE).softmax(-1)          # (B, H, L, L)
        do = inp["cot"].double().view(B, L, H, DH).permute(0, 2, 1, 3)           # (B, H, L, DH)
        e = U_BF16 * (do * o).abs().sum(-1)                                      # (B, H, L): delta's doubt from bf16 O
        allow_dq = SCALE * e * torch.einsum("bhxy,bhyd->bhxd", p, k).norm(dim=-1)
        allow_dk = SCALE * torch.einsum("bhxy,bhx->bhy", p, e * q.norm(dim=-1))
        mass = None
        if inp["plant"] is not None:
            rest = p[:, :, _planted_rows(L), :].clone()
            rest[..., inp["plant"]] = 0.0
            mass = 1.0 - rest.sum(-1).max().item()                               # the least mass on the planted key
    return dict(out=out.detach(), lse=lse.detach(), dqkv=x.grad, mass=mass,
                allow=(_rows_bhl(allow_dq), _rows_bhl(allow_dk), None))


def _isolated_feed_cpu(name):
    """out = bf16(O_fp64), lse2 = f32(lse_fp64 * log2 e)."""
    ref = _reference(name)
    return ref["out"].to(BF16), (ref["lse"] * LOG2E).float()


# ------------------------------------------------------------------------------------------------ metrics
def _worst_row(x, ref, allow):
    """Largest (||err|| - allowance)+ / max(||ref row||, 0.1 mean ||ref row||) over the (b, token, h) rows."""
    x, ref = x.detach().double().cpu().reshape(-1, DH), ref.double().reshape(-1, DH)
    err, rn = (x - ref).norm(dim=1), ref.norm(dim=1)
    if allow is not None:
        err = (err - allow).clamp_min(0.0)
    den = rn.clamp_min(0.1 * rn.mean().item())
    return torch.where(err > 0, err / den, torch.zeros_like(err)).max().item()   # 0 / 0 (L = 1) counts as 0


def _figures(name, dqkv):
    """{dq|dk|dv: (rel-L2 or None where the reference is identically 0, max abs err, max|ref|, worst row)}."""
    ref, C = _reference(name), _inputs(name)["C"]
    got, fig = dqkv.detach().double().cpu(), {}
    for i, nm in enumerate(("dq", "dk", "dv")):
        a, b = got[..., i * C:(i + 1) * C], ref["dqkv"][..., i * C:(i + 1) * C]
        l2 = rel_err(a, b) if b.norm().item() > 0 else None
        fig[nm] = (l2, (a - b).abs().max().item(), b.abs().max().item(), _worst_row(a, b, ref["allow"][i]))
    return fig


def _fmt(l2):
    return "   (ref 0)" if l2 is None else f"{l2:10.3e}"


# ------------------------------------------------------------------------------------------------ GPU side
@functools.lru_cache(maxsize=None)
def _autocast(name):
    """Figures of torch's own bf16-autocast evaluation on the GPU: einsum -> * scale -> f32 softmax -> einsum, as
    test_attention_gpu.py::_reference_autocast_attention states the reference's AMP path, with autograd."""
    inp = _inputs(name)
    B, H, L, C = inp["B"], inp["H"], inp["L"], inp["C"]
    x = inp["qkv"].cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16):
        q, k, v = oatt.split_qkv(x, H)
        p = (torch.einsum("bhxd,bhyd->bhxy", q, k) * SCALE).softmax(-1)
        o = torch.einsum("bhxy,bhyd->bhxd", p, v)
    o.permute(0, 2, 1, 3).reshape(B, L, C).float().backward(inp["cot"].cuda())
    return _figures(name, x.grad)


@functools.lru_cache(maxsize=None)
def _feed(name, mode):
    """x, dy and the out / lse2 the backward is fed, on the GPU. Shared, never modified."""
    from long_context_biomedical_imaging_amd import kernels
    inp = _inputs(name)
    x, dy = inp["qkv"].cuda().to(BF16), inp["cot"].cuda().to(BF16)
    if mode == "isolated":
        out, lse2 = (t.cuda() for t in _isolated_feed_cpu(name))
    else:
        out, lse2 = kernels.attn_fwd(x, inp["H"], SCALE)
    torch.cuda.synchronize()
    return dict(x=x, dy=dy, out=out.contiguous(), lse2=lse2.contiguous(), H=inp["H"])


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda", dtype=dtype)
    buf[GUARD:GUARD + n] = fill
    return buf


def _inner(buf):
    return buf[GUARD:buf.numel() - GUARD]


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[buf.numel() - GUARD:] == SENTINEL).all())


def _new_dqkv(f, fill=float("nan")):
    return _guarded(f["x"].numel(), BF16, fill)


def _new_ws(f, fill=WS_NAN):
    from long_context_biomedical_imaging_amd import _lib
    B, L, _ = f["x"].shape
    return _guarded(int(_lib.load().lci_attn_bwd_ws_bytes(B, f["H"], L)) // 4, torch.int32, fill)


def _copy(buf):
    return buf.clone()


def _stage(f, variant, stage, dq_buf, ws_buf):
    """One lci_attn_bwd_variant call into the guarded buffers; returns (dqkv view, flags view)."""
    from long_context_biomedical_imaging_amd import kernels
    g, flags = kernels.attn_bwd_variant(f["x"], f["out"], f["dy"], f["lse2"], f["H"], SCALE, variant, stage,
                                        ws=_inner(ws_buf), dqkv=_inner(dq_buf).view(f["x"].shape))
    torch.cuda.synchronize()
    return g, flags


def _flag_span(f):
    B, L, _ = f["x"].shape
    n0 = B * f["H"] * 2 * L
    return n0, n0 + B * f["H"] * ((L + 511) // 512)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][3] is not None])
def test_planted_rows_are_dominated(name):
    """From the reference alone: every planted query puts >= 1 - 1e-4 of its softmax mass on the planted key."""
    mass = _reference(name)["mass"]
    print(f"{name}: least softmax mass on the planted key 1 - {1.0 - mass:.3e}")
    assert mass >= PLANT_MASS, f"{name}: the input does not stress the path: mass 1 - {1.0 - mass:.3e}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_stages_vs_fp64(name, mode):
    """Delta, dK/dV and both dQ kernels, one stage at a time into NaN-filled guarded buffers: write coverage, guard
    bands, the workspace contract, and every numeric bound of the module docstring."""
    inp, f = _inputs(name), _feed(name, mode)
    B, H, L, C = inp["B"], inp["H"], inp["L"], inp["C"]
    bad = []
    if inp["plant"] is not None:
        assert _reference(name)["mass"] >= PLANT_MASS

    # ---- stage 0: the row constants
    ws0, dq0 = _new_ws(f), _new_dqkv(f)
    _stage(f, NARROW, 0, dq0, ws0)
    f0, f1 = _flag_span(f)
    rows = _inner(ws0)[:f0].view(B, H, 2, L)
    if not torch.equal(rows[:, :, 0], (-f["lse2"]).view(torch.int32)):
        bad.append("ws row 0 is not -lse2 bitwise")
    prod = (f["dy"].double() * f["out"].double()).view(B, L, H, DH).permute(0, 2, 1, 3).cpu()
    d_err = (rows[:, :, 1].view(torch.float32).double().cpu() + prod.sum(-1)).abs()
    d_bound = 64 * 2.0 ** -24 * prod.abs().sum(-1)
    print(f"{name:18s} {mode:10s} delta: worst err / bound {(d_err / d_bound.clamp_min(1e-300)).max().item():.3f}")
    if not bool((d_err <= d_bound).all()):
        bad.append(f"-delta: worst excess over 64 * 2^-24 * sum|dO O| {(d_err - d_bound).max().item():.3e}")
    if not bool((_inner(ws0)[f0:] == WS_NAN).all()):
        bad.append("stage 0 wrote behind the row constants")
    if not bool(torch.isnan(_inner(dq0)).all()):
        bad.append("stage 0 wrote dqkv")
    if not (_guards_intact(ws0) and _guards_intact(dq0)):
        bad.append("stage 0: guard band overwritten")

    # ---- stage 1: dK, dV
    ws1, dq1 = _copy(ws0), _new_dqkv(f)
    g1, _ = _stage(f, NARROW, 1, dq1, ws1)
    if not bool(torch.isfinite(g1[..., C:]).all()):
        bad.append(f"stage 1: {int((~torch.isfinite(g1[..., C:])).sum())} dK / dV elements not written")
    if not bool(torch.isnan(g1[..., :C]).all()):
        bad.append("stage 1 wrote the Q third")
    if not torch.equal(ws1, ws0):
        bad.append("stage 1 wrote the workspace")
    if not _guards_intact(dq1):
        bad.append("stage 1: dqkv guard band overwritten")

    # ---- stage 2: dQ, either kernel
    ac = _autocast(name)
    for variant, vn in ((NARROW, "narrow"), (WIDE, "wide")):
        ws2, dq2 = _copy(ws0), _new_dqkv(f)
        g2, flags = _stage(f, variant, 2, dq2, ws2)
        if not bool(torch.isfinite(g2[..., :C]).all()):
            bad.append(f"{vn} stage 2: {int((~torch.isfinite(g2[..., :C])).sum())} dQ elements not written")
        if not bool(torch.isnan(g2[..., C:]).all()):
            bad.append(f"{vn} stage 2 wrote the K / V thirds")
        if not _guards_intact(dq2):
            bad.append(f"{vn} stage 2: dqkv guard band overwritten")
        if variant == WIDE:
            fl = flags.clone()
            if not bool(((fl == 0) | (fl == 1)).all()):
                bad.append(f"wide stage 2: flags {fl.flatten().tolist()}")
            if inp["plant"] is None and not bool((fl == 0).all()):
                bad.append("random data: a wide workgroup was flagged")
            _inner(ws2)[f0:f1] = WS_NAN
        if not torch.equal(ws2, ws0):
            bad.append(f"{vn} stage 2 wrote the workspace" + (" outside its flag words" if variant == WIDE else ""))

        # ---- the numbers: K / V thirds of stage 1 with this kernel's Q third
        fig = _figures(name, torch.cat([g2[..., :C], g1[..., C:]], dim=-1))
        for nm, (l2, mx, mref, row) in fig.items():
            if nm != "dq" and variant == WIDE:
                continue   # dK / dV: one kernel, reported and checked once
            a_l2, a_mx, _, a_row = ac[nm]
            row_max = max(5e-2, 2.0 * a_row)
            print(f"{name:18s} {mode:10s} {nm}{'' if nm != 'dq' else '/' + vn:7s} kernel rel-L2 {_fmt(l2)} max abs "
                  f"{mx:.3e} worst row {row:.3e} | autocast rel-L2 {_fmt(a_l2)} max abs {a_mx:.3e} worst row "
                  f"{a_row:.3e} | max|ref| {mref:.3e} row bound {row_max:.3e}")
            what = nm + (f" ({vn})" if nm == "dq" else "")
            if l2 is not None and not l2 <= 2e-2:
                bad.append(f"{what}: rel-L2 {l2:.3e} > 2e-2")
            if not mx <= 3e-2 * mref + 2e-3:
                bad.append(f"{what}: max err {mx:.3e} > 3e-2 * {mref:.3e} + 2e-3")
            if not row <= row_max:
                bad.append(f"{what}: worst row {row:.3e} > {row_max:.3e}")
    assert not bad, f"{name} [{mode}]: " + "; ".join(bad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_composition_and_determinism(name, mode):
    """Stages 0, 1, 2 one after another into one dqkv equal a single stage = -1 call bitwise, and a second
    stage = -1 call over buffers pre-filled with other values gives the same bits (both dQ variants)."""
    inp, f = _inputs(name), _feed(name, mode)
    f0, f1 = _flag_span(f)
    for variant in (NARROW, WIDE):
        end = f1 if variant == WIDE else f0
        wa, da = _new_ws(f), _new_dqkv(f)
        _stage(f, variant, -1, da, wa)
        assert bool(torch.isfinite(_inner(da)).all()), "stage -1 left dqkv elements unwritten"
        wb, db = _new_ws(f, WS_THREE), _new_dqkv(f, 3.0)
        _stage(f, variant, -1, db, wb)
        assert torch.equal(da, db), f"variant {variant}: two runs differ in dqkv"
        assert torch.equal(_inner(wa)[:end], _inner(wb)[:end]), f"variant {variant}: two runs differ in ws"
        assert bool((_inner(wb)[end:] == WS_THREE).all()), f"variant {variant}: ws written past its defined part"
        wc, dc = _new_ws(f), _new_dqkv(f)
        for stage in (0, 1, 2):
            _stage(f, variant, stage, dc, wc)
        assert torch.equal(dc, da), f"variant {variant}: stages 0, 1, 2 differ from stage -1 in dqkv"
        assert torch.equal(wc, wa), f"variant {variant}: stages 0, 1, 2 differ from stage -1 in ws"
        assert _guards_intact(da) and _guards_intact(wa) and _guards_intact(dc) and _guards_intact(wc)


@pytest.mark.parametrize("mode", MODES)
def test_slice_independence(mode):
    """Each (b, h) of the B2 H3 L577 case repacked as a B1 H1 problem (its own q, k, v, out, dO, lse2) gives the
    batched run's slice of dQ, dK and dV bit for bit, for both dQ variants; no wide workgroup is flagged."""
    name = "L577_b2h3"
    inp, f = _inputs(name), _feed(name, mode)
    B, H, L, C = inp["B"], inp["H"], inp["L"], inp["C"]
    for variant in (NARROW, WIDE):
        wf, df = _new_ws(f), _new_dqkv(f)
        full, flags = _stage(f, variant, -1, df, wf)
        if variant == WIDE:
            assert bool((flags == 0).all()), f"random data: flags {flags.flatten().tolist()}"
        for b in range(B):
            for h in range(H):
                cols = [t * C + h * DH + d for t in range(3) for d in range(DH)]
                one = dict(x=f["x"][b:b + 1, :, cols].contiguous(), H=1,
                           out=f["out"][b:b + 1, :, h * DH:(h + 1) * DH].contiguous(),
                           dy=f["dy"][b:b + 1, :, h * DH:(h + 1) * DH].contiguous(),
                           lse2=f["lse2"][b:b + 1, h:h + 1].contiguous())
                w1, d1 = _new_ws(one), _new_dqkv(one)
                g, fl = _stage(one, variant, -1, d1, w1)
                if variant == WIDE:
                    assert bool((fl == 0).all())
                assert torch.equal(g[0], full[b][:, cols]), f"variant {variant}: slice b{b} h{h} differs"
                assert _guards_intact(d1) and _guards_intact(w1)
