"""The wide attention-backward dK/dV kernel (csrc/attention.hip, attn_bwd_dkdv_hs3_kernel: 96 keys per wave, 384 per
workgroup) without a GPU: the host-side split of the key range between it and attn_bwd_dkdv_hs_kernel
(lci_attn_bwd_dkdv_pick) and the ISA guards tests/test_attention_isa_cpu.py applies to the narrow kernels (through
that module's helpers): no scratch, no allocator copies in the tile loop, no MFMA hazard the compiler could not see,
the register budget, and the shape of the placed stream."""
import os
import re

import pytest

import test_attention_isa_cpu as isa_cpu
from test_attention_dq_wide_cpu import _meta

WIDE = "attn_bwd_dkdv_hs3_kernel"
WIDE_K, NARROW_K = 384, 256   # keys per workgroup: 4 waves x 96, 4 waves x 64

isa = isa_cpu.isa   # the module-scoped fixture: one gfx950 compile of attention.hip


def _lib():
    from long_context_biomedical_imaging_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liblci.so not built (python -m long_context_biomedical_imaging_amd.build_lib)")
    return _lib.load()


def test_pick_pinned_points():
    pick = _lib().lci_attn_bwd_dkdv_pick
    assert pick(2, 65536, 6, 256) == 128    # the metric: 1536 wide workgroups (6 rounds) + 768 narrow (3 rounds)
    assert pick(2, 32768, 6, 256) == 0      # the only splits that fill both grids (W = 59) cost 13 against 12
    assert pick(2, 16384, 6, 256) == 0      # no W fills both grids
    assert pick(1, 65536, 12, 256) == 128   # B H is what counts
    assert pick(1, 384, 256, 256) == 1      # all keys wide, no narrow launch: 3 against 4
    assert pick(1, 383, 256, 256) == 0      # 384 W <= L
    assert pick(1, 77, 2, 256) == 0
    assert pick(2, 65536, 6, 0) == 0        # unknown device: narrow alone
    assert pick(0, 65536, 6, 256) == 0


def _fills(wgs, n_cu):
    return wgs >= n_cu and 10 * wgs >= 9 * -(-wgs // n_cu) * n_cu


def _want(B, L, H, n_cu):
    """The rule as include/lci.h states it."""
    bh = B * H
    best, cost_best = 0, 2 * -(-(bh * -(-L // NARROW_K)) // n_cu)
    for W in range(1, L // WIDE_K + 1):
        wide, rest = bh * W, bh * -(-(L - WIDE_K * W) // NARROW_K)
        if not _fills(wide, n_cu) or (rest and not _fills(rest, n_cu)):
            continue
        cost = 3 * -(-wide // n_cu) + 2 * -(-rest // n_cu)
        if cost <= cost_best:
            best, cost_best = W, cost
    return best


def test_pick_is_the_stated_rule():
    lib = _lib()
    some = 0
    for n_cu in (64, 240, 256, 304):
        for B in (1, 2, 3, 8):
            for H in (1, 6, 12):
                for L in (1, 383, 384, 500, 4096, 10000, 16384, 20000, 32768, 65536, 100000):
                    got = lib.lci_attn_bwd_dkdv_pick(B, L, H, n_cu)
                    assert got == _want(B, L, H, n_cu), (B, L, H, n_cu)
                    assert 0 <= WIDE_K * got <= L
                    some += got > 0
    assert some > 10, "the sweep never reaches a split"


def test_no_allocator_copies_in_placed_loops(isa):
    isa_cpu.test_no_allocator_copies_in_placed_loops(isa, WIDE)


def test_no_mfma_hazards(isa):
    isa_cpu.test_no_mfma_hazards(isa, WIDE)


def test_wide_registers_and_scratch(isa):
    """No scratch; arch + acc registers within 504 of the 512 of one wave per SIMD; the AGPR half exactly full (192
    accumulators + the K / V fragments of two key blocks)."""
    assert _meta(isa, WIDE, "amdhsa_private_segment_fixed_size") == 0
    assert _meta(isa, WIDE, "amdhsa_next_free_vgpr") <= 504
    assert _meta(isa, WIDE, "amdhsa_accum_offset") <= 248
    assert _meta(isa, WIDE, "amdhsa_next_free_vgpr") - _meta(isa, WIDE, "amdhsa_accum_offset") == 256
    assert "scratch_" not in isa_cpu._kernel_body(isa, WIDE)


def test_wide_stream_shape(isa):
    """The 4-tile unrolled loop: per 64-query tile 96 MFMAs (48 per half) against the narrow kernel's 64 fragment
    reads (8 row + 8 row-constant + 16 transposed per half), five LDS-DMA pieces, one barrier, and one exp2, one
    multiply and one pack per MFMA; no LDS store and no VALU the stream did not place."""
    main = max(isa_cpu._loops(isa_cpu._kernel_body(isa, WIDE)), key=len)
    code = "\n".join(l for l in main.splitlines() if not l.strip().startswith(";"))
    n = lambda pat: len(re.findall(pat, code, re.M))   # noqa: E731
    assert n(r"v_mfma_f32_32x32x16_bf16") == 4 * 96
    assert n(r"\bds_read_b128\b") == 4 * 32 and n(r"\bds_read_b64_tr_b16\b") == 4 * 32
    assert n(r"\bbuffer_load_dwordx4\b.*\blds\b") == 4 * 4 and n(r"\bbuffer_load_dword\b.*\blds\b") == 4
    assert n(r"\bbuffer_load_dword") == 4 * 5 and n(r"\bds_write") == 0
    assert n(r"\bs_barrier\b") == 4
    assert n(r"\bv_exp_f32\b") == 4 * 96 and n(r"\bv_mul_f32\b") == 4 * 96 and n(r"\bv_cvt_pk_bf16_f32\b") == 4 * 96
    assert n(r"^\s*v_(?!mfma_f32_32x32x16_bf16|exp_f32|mul_f32|cvt_pk_bf16_f32)") == 0
