"""The conditions that keep tests/test_gpu_attention_parity.py honest, checked from the references alone (no GPU, no library):
leg A's data is exact where the GPU test says a disagreement is a wrong element, leg A2's selected key leads by the stated gap, the
planted keys of leg B reach the score range they claim, and the rounding model meets every elementwise bound on every listed input
(a bound the model cannot meet is a wrong derivation, not a wrong input)."""
import math

import pytest
import torch

from tests import helpers_attention as ha

CASES = ha.ALL_CASES
IDS = [ha.case_id(c) for c in CASES]


def test_the_case_lists_reach_the_kernels_they_name():
    assert all(ha.forward_kernel(*c) == ha.X32 for c in ha.X32_CASES)
    assert all(ha.forward_kernel(*c) == ha.K16 for c in ha.K16_CASES + ha.BWD_CASES)
    assert len(set(CASES)) == len(CASES)
    for side in (0, 1):            # every tile-edge value on each side of the backward
        assert {p[side] for p in ha.BWD_PAIRS} == {63, 64, 65, 127, 128, 129}
    for d, nk in ha.CONSISTENCY_CASES:
        assert ha.forward_kernel(d, 256, nk) == ha.X32 and ha.forward_kernel(d, 200, nk) == ha.K16


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_uniform_rows_are_exact_and_sensitive(case):
    """Leg A1.  Every sum of integers from {+-1, +-2, +-3} is exact in fp32 in any order; a missing or an extra key (query) moves a
    channel's sum by at least 1 and the LSE by log2((Nk +- 1) / Nk); both exceed what the GPU test allows: one bf16 ulp of the mean is
    less than one unit of the sum while |sum| < 128, and the LSE allowance is 4 * 2^-23 * max(1, log2 Nk)."""
    d, nq, nk = case
    q, k, v, do = ha.uniform_input(case)
    assert 3 * max(nq, nk) < 2 ** 24
    assert not q.any()
    for t in (v, do):
        assert bool(((t.double().abs() >= 1) & (t.double().abs() <= 3) & (t.double() == t.double().round())).all())
        assert float(t.double().sum(dim=1).abs().max()) * 2.0 ** -7 < 1.0
    allowance = 4 * 2.0 ** -23 * max(1.0, math.log2(nk))
    assert math.log2((nk + 1) / nk) > 100 * allowance
    r = ha.ref64(q, k, v, do, d)
    assert float((r["lse"] - math.log2(nk)).abs().max()) < 1e-12
    assert float((r["o"] - v.double().mean(dim=1, keepdim=True)).abs().max()) < 1e-12
    assert float(r["dk"].abs().max()) == 0.0
    assert float((r["dv"] - do.double().sum(dim=1, keepdim=True) / nk).abs().max()) < 1e-12


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_hot_rows_lead_by_the_gap(case):
    """Leg A2: distinct K rows per head, g a power of two in 4 .. 32, the selected score at least 40 log2 units above every other of its
    row in fp64; then O[q] = V[j(q)], dQ and dK vanish and dV[j] is the integer sum of the dO rows that select j, all to 2^-30."""
    d, nq, nk = case
    q, k, v, do, g = ha.one_hot_input(case)
    assert 4 <= g <= 32 and math.log2(g) == int(math.log2(g)), g
    kh = ha.heads_view(k, d)
    gram = kh @ kh.transpose(-1, -2)
    off = ~torch.eye(nk, dtype=torch.bool)
    assert float(gram[..., off].max()) < d, "two K rows of one head coincide"
    j = ha.selected_key(nq, nk)
    s = ha.scores64(q, k, d)
    sel = s.gather(-1, j.view(1, 1, nq, 1).expand(ha.B, ha.HEADS, nq, 1))
    rest = s.masked_fill(torch.nn.functional.one_hot(j, nk).bool(), -math.inf).amax(dim=-1, keepdim=True)
    assert float((sel - rest).min()) >= ha.GAP
    assert float((sel.squeeze(-1) - g * ha.c_of(d) * d).abs().max()) < 1e-4 * g * d
    r = ha.ref64(q, k, v, do, d)
    assert float((r["o"] - v.double()[:, j]).abs().max()) < 2.0 ** -30
    assert float(r["dq"].abs().max()) < 2.0 ** -20 and float(r["dk"].abs().max()) < 2.0 ** -20
    want, allow = ha.one_hot_dv(do, nq, nk)
    assert float((r["dv"] - want).abs().max()) < 2.0 ** -20
    # where the exact integer sum is 0 fp64 itself leaves the other queries' P dO, not 0: inside the stated allowance, which stays below
    # 2^-10 of the unit a wrong row would move the sum by
    assert bool(((r["dv"] - want).abs() <= allow).all()) and float(allow[want == 0].max() if bool((want == 0).any()) else 0.0) < 2.0 ** -10
    assert bool((want[:, torch.bincount(j, minlength=nk) == 0] == 0).all())
    assert 3 * 9 * d * max(nq, nk) < 2 ** 24           # delta = dO . V[j] and the dV sums are exact fp32 integers


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_meets_the_elementwise_bounds_on_hard_inputs(case):
    """Leg B: the planted keys are their rows' maxima at 3 |q|^2 c (gain^2 more at gain 2 / 4), and the model's LSE stays inside the
    elementwise bound on every input the GPU test bounds; its outputs are finite everywhere."""
    d, nq, nk = case
    assert ha.planted(case) and all(ki >= (nk - 1) // 64 * 64 for _, ki in ha.planted(case))
    for kind in ha.DATA_KINDS:
        q, k, v, do = ha.hard_input(case, kind)
        ref, mdl, bound = ha.hard_reference(case, kind)
        if kind != "randn":
            gain = {"aligned": 1.0, "gain2": 2.0, "gain4": 4.0}[kind]
            s = ha.scores64(q, k, d)
            for qi, ki in ha.planted(case):
                claim = 3.0 * ha.heads_view(q, d)[:, :, qi].pow(2).sum(dim=-1) * ha.c_of(d)            # [B][H]
                assert float((s[:, :, qi, ki] - claim).abs().max()) <= 2.0 ** -7 * float(claim.max())  # k = bf16(3 q)
                assert bool((s[:, :, qi, ki] == s[:, :, qi].amax(dim=-1)).all())
                lo, hi = 3.0 * d * ha.c_of(d) * gain * gain * 0.3, 3.0 * d * ha.c_of(d) * gain * gain * 2.2
                assert lo <= float(claim.min()) and float(claim.max()) <= hi, (kind, float(claim.min()), float(claim.max()), lo, hi)
        assert all(bool(torch.isfinite(mdl[x]).all()) for x in ("lse", "o", "dq", "dk", "dv"))
        if kind != "gain4":
            worst = float(((mdl["lse"] - ref["lse"]).abs() / bound).max())
            assert worst <= 1.0, (kind, worst)
