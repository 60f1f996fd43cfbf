"""CPU (-m "not gpu"): the conditions that keep tests/test_gpu_gemm_exact.py honest.

1. The data is exact: every accumulator and every epilogue sum of every case is an integer (or a multiple of 2^-4) below 2^24, every
   Winograd intermediate equals its own bf16 rounding, and enough outputs are exact bf16 ties that the store's rounding mode is exercised.
2. Every case runs where it says: dfh_gemm_plan (host code) returns the kernel, tile, bm x bn, stages, lean, wide, split and n_major the
   case names, dfh_gemm_wgrad_plan the decomposition a weight-gradient case names.  A pin that falls back fails here.
3. The tables are complete: every instantiation among the [default] lines of tests/golden/gemm_plan_table.txt is covered by a forward case and
   by one with a ragged M, bar the ones helpers_gemm.UNREACHABLE names."""
import ctypes as C
import os
import re

import pytest
import torch

from difashion_amd import _lib
from tests import helpers_gemm as hg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_table.txt")
PTR = 4096                      # a made-up address: the plan tests pointers for presence only

FORWARD = hg.forward_cases()
ACT = [hg.act_case(*a) for a in hg.ACT_CASES]
ACT_GEGLU = [hg.lin(i, M, N, K, act=4) for i, M, N, K in hg.ACT_GEGLU]
PLANNED = FORWARD + hg.FALLBACK_CASES + hg.GEGLU_CASES + ACT + ACT_GEGLU
WGRAD = hg.wgrad_cases()


def plan(c, **extra):
    d = hg.fill_desc(_lib.GemmDesc(), c, lambda name: PTR)
    info = _lib.GemmPlanInfo()
    rc = _lib.raw().dfh_gemm_plan(C.byref(d), C.byref(_lib.GemmPlanExtra(**extra)), C.byref(info))
    return rc, info


def got_plan(info):
    return (info.kernel, info.tile, info.bm, info.bn, info.stages, info.lean, info.wide, info.split, info.n_major)


# ----------------------------------------------------------------------------- 1. the data is exact
@pytest.mark.parametrize("c", FORWARD, ids=hg.case_id)
def test_forward_sums_are_exact_and_ties_occur(c):
    inp = hg.forward_inputs(c)
    ref = hg.forward_ref64(c, inp)
    worst = float(inp["acc"].abs().max()) + 400 + 64 + 512
    assert worst < 2 ** 24 and bool((ref == ref.round()).all()), "fp32 holds every partial sum and the epilogue's sums exactly"
    if c.get("out_mode", 0) in (0, 1):
        share = hg.tie_share(ref)
        print(f"gemm exact inputs {hg.case_id(c)}: |acc| <= {float(inp['acc'].abs().max()):.0f} ties {share:.3f}")
        assert share >= 0.02, share


def test_reference_alone_exercises_the_rounding_mode():
    """integers of [-3, 3] at K = 2048 without bias or residual: |acc| stays far below 2^24 and some 8 % of the outputs are exact ties"""
    a, w = hg.int_operand((256, 2048), -3, 3, 1).double(), hg.int_operand((160, 2048), -3, 3, 2).double()
    acc = a @ w.T
    print(f"gemm exact inputs reference: |acc| <= {float(acc.abs().max()):.0f} ties {hg.tie_share(acc):.3f}")
    assert float(acc.abs().max()) < 2 ** 24 and hg.tie_share(acc) >= 0.02


def test_the_defects_the_tolerance_tests_cannot_see_change_the_exact_result():
    """What bit equality buys, shown on the references alone: each of the small defects a 6e-3 tolerance passes -- a second rounding in the
    epilogue (the residual added after the store's rounding), one k element counted twice, one tap reading the neighbouring pixel at
    the image border -- changes rounded_once(ref64) somewhere, so the GPU legs fail on it."""
    c = hg.lin("e8_s4_lean", 300, 320, 256, K1=64, fsplit=1)
    inp = hg.forward_inputs(c)
    ref = hg.forward_ref64(c, inp)
    want = hg.rounded_once(ref)
    twice = (hg.rounded_once(hg.pre64(inp["acc"], inp["bias"], inp["rowvec"], c["N"], c["M"])).double() + inp["resid"].double()).to(hg.BF16)
    assert int((twice != want).sum()) > 0.01 * want.numel(), "rounding before the residual moves the ties"
    a = torch.cat([inp["a0"], inp["a1"]], 1).double()
    again = ref + a[:, 64:65] * inp["w"].double()[:, 64:65].T                      # element 64 of K counted twice
    assert int((hg.rounded_once(again) != want).sum()) > 0.2 * want.numel()
    cc = hg.conv("e8_s4", 2, 5, 3, 72, 168, fsplit=1, nm=1)
    ci = hg.forward_inputs(cc)
    x = ci["x"].double()
    shifted = x.clone()
    shifted[:, :, 0] = x[:, :, 1]                                                   # the taps of column 0 read column 1
    w = ci["w"].double()
    w_tap = torch.zeros_like(w)
    w_tap[:, 4 * 72:5 * 72] = w[:, 4 * 72:5 * 72]                                   # ... for the centre tap only
    wrong_tap = hg.conv64(ci["x"], w - w_tap) + hg.conv64(shifted.to(hg.BF16), w_tap)
    good = hg.rounded_once(hg.forward_ref64(cc, ci))
    bad = hg.rounded_once(hg.ref64(wrong_tap, ci["bias"], ci["rowvec"], cc["N"], cc["rows_per_b"], 0, ci["resid"]))
    assert int((bad != good).sum()) > 0 and int((bad != good).any(1).sum()) <= 2 * 5, "only the border pixels of each image move"


@pytest.mark.parametrize("case", hg.WINO_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_winograd_intermediates_are_exact_in_bf16(case):
    inp = hg.wino_inputs(case)
    U, V, M = hg.wino_intermediates(inp)
    for name, t, bound in (("U", U, 18), ("V", V, 4), ("M", M, 144)):
        assert float(t.abs().max()) <= bound, (name, float(t.abs().max()))
        assert torch.equal(t.to(hg.BF16).double(), t), name
    # the planes, transformed back, are the conv: A^T m A
    AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1.]], dtype=torch.float64)
    B, cin, cout, H, W = case[:5]
    y = torch.einsum("ij,jkbyxc,lk->byixlc", AT, M.view(4, 4, B, H // 2, W // 2, cout), AT).reshape(B * H * W, cout)
    assert torch.equal(y, hg.conv64(inp["x"], hg.pack_conv64(inp["w"])))
    ref = hg.wino_ref64(case, inp)
    assert float(ref.abs().max()) > 256 and hg.tie_share(ref) >= 0.02, "some outputs pass 256 and round"


@pytest.mark.parametrize("c", ACT + ACT_GEGLU, ids=hg.case_id)
def test_activation_inputs_are_exact_and_span_the_range(c):
    inp = hg.act_inputs(c)
    _, rpb = hg.n_batches(c)
    pre = hg.pre64(inp["acc"], inp["bias"], inp["rowvec"], c["N"], rpb)
    assert torch.equal(pre * 16, (pre * 16).round()) and float(pre.abs().max()) * 16 < 2 ** 24, "multiples of 2^-4, exact in fp32"
    x = hg.geglu_split(pre)[1] if c["act"] == 4 else pre
    lo, hi = float(x.min()), float(x.max())
    assert bool((x == 0).any()) and bool((x == -1.25).any()) and bool((x == -1.3125).any()), "exact 0 and both sides of SiLU's minimum"
    assert (lo <= -11 and hi >= 11) if c["act"] != 4 else (lo <= -4 and hi >= 4), (lo, hi)


@pytest.mark.parametrize("c", WGRAD, ids=hg.wgrad_id)
def test_weight_gradient_sums_are_exact(c):
    inp = hg.wgrad_inputs(c)
    assert float(inp["ref"].abs().max()) < 2 ** 24 and float((inp["ref"] - inp["dw0"].double()).abs().max()) > 0


# ----------------------------------------------------------------------------- 2. every case runs where it says
@pytest.mark.parametrize("c", PLANNED, ids=hg.case_id)
def test_case_plans_the_instantiation_it_names(c):
    rc, info = plan(c)
    assert rc == 0, info.line.decode()
    assert got_plan(info) == hg.want_plan(c), info.line.decode()


def wgrad_plan(c):
    d = hg.fill_desc(_lib.GemmDesc(), dict(c, inst="e8_s4"), lambda name: PTR)
    t, w, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = _lib.raw().dfh_gemm_wgrad_plan(C.byref(d), c["msplit"], C.byref(t), C.byref(w), C.byref(s))
    return rc, (t.value, w.value, s.value)


@pytest.mark.parametrize("c", WGRAD, ids=hg.wgrad_id)
def test_weight_gradient_case_plans_the_decomposition_it_names(c):
    rc, got = wgrad_plan(c)
    assert rc == 0 and got == hg.WGRAD_PLANS[hg.wgrad_id(c)], got


def test_weight_gradient_cases_slice_ragged_and_whole():
    plans = [hg.WGRAD_PLANS[hg.wgrad_id(c)] for c in WGRAD]
    assert any(s > 1 and c["M"] % s for c, (_, _, s) in zip(WGRAD, plans)), "pixel slices that do not divide M"
    assert any(s == 1 for _, _, s in plans) and any(s >= 7 for _, _, s in plans)


# ----------------------------------------------------------------------------- 3. completeness against the golden plan table
def golden_instantiations():
    keys, sec = set(), None
    for ln in open(GOLDEN).read().splitlines():
        if ln.startswith("["):
            sec = ln
        elif sec == "[default]" and " refused: " not in ln:
            m = re.search(r"\| kernel=(\S+) tile=(\d+) (\d+x\d+) stages=(\d+) lean=(\d+) wide=(\d+) ", ln)
            keys.add((m.group(1), int(m.group(2)), m.group(3), int(m.group(4)), int(m.group(5)), int(m.group(6))))
    return keys


def test_every_instantiation_of_the_golden_table_is_covered():
    assert len(hg.UNREACHABLE) <= 2
    gold = golden_instantiations()
    assert len(gold) >= 16
    left_out = {k for k in gold if any(f(k) for f in hg.UNREACHABLE.values())}
    for name, f in hg.UNREACHABLE.items():
        assert any(f(k) for k in gold), f"{name}: names nothing of the golden table"
    fwd = FORWARD + hg.GEGLU_CASES
    covered = {hg.inst_key(c["inst"]) for c in fwd}
    ragged = {hg.inst_key(c["inst"]) for c in fwd if c["M"] % hg.INST[c["inst"]][3]}
    assert gold - left_out <= covered, sorted(gold - left_out - covered)
    assert gold - left_out <= ragged, sorted(gold - left_out - ragged)
    assert covered <= gold, "an instantiation the walks never launch: " + str(sorted(covered - gold))
    for what, pick in (("split > 1", lambda c: hg.want_plan(c)[7] > 1), ("n_major = 1", lambda c: hg.want_plan(c)[8] == 1)):
        kernels = {hg.INST[c["inst"]][1:3] + hg.INST[c["inst"]][7:] for c in fwd if pick(c)}
        assert len(kernels) >= 2, (what, kernels)


# ----------------------------------------------------------------------------- what the older tolerance tests pin
def test_report_pinned_ids_of_the_older_tests_that_plan_another_kernel():
    """test_gemm_plain and test_conv3x3 (tests/test_gpu_ops.py) parametrise over tile ids; a pin the launch cannot take falls back to the
    heuristic tile.  Counted here with dfh_gemm_plan and printed, not asserted: those tests stay as they are."""
    named = {1: (0, 0), 2: (0, 1), 3: (0, 2), 4: (0, 3), 5: (0, 4), 6: (3, 1), 9: (3, 4), 10: (0, 5), 21: (1, None)}

    def other(d, tile):
        info = _lib.GemmPlanInfo()
        assert _lib.raw().dfh_gemm_plan(C.byref(d), None, C.byref(info)) == 0
        k, sub = named[tile]
        return info.kernel != k or (sub is not None and (info.wide if k == 3 else info.tile) != sub)

    def desc(M, N, ldw, tile, order=-1, **kw):
        d = _lib.GemmDesc()
        d.W, d.out, d.zero_page, d.bias, d.M, d.N, d.ldw, d.ld_out, d.force_tile, d.force_order = PTR, PTR, PTR, PTR, M, N, ldw, N, tile, order
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    plain = [(t, o, s) for t in (1, 2, 3, 4, 5, 6, 9, 10, 21) for o in (-1, 2, 3)
             for s in ((300, 320, 320), (128, 160, 64), (77 * 3, 64, 768), (16, 1280, 200), (4, 256, 2048))]
    n_plain = sum(other(desc(M, N, K, t, o, a0=PTR, a0_c=K, resid=PTR, ld_res=N), t) for t, o, (M, N, K) in plain)
    convs = [(g, s) for g in (1, 4, 6, 9, 10, 21) for s in ((64, 160, 16, 1, 0), (32, 64, 8, 1, 0), (320, 320, 16, 1, 0), (64, 64, 16, 2, 0),
                                                             (64, 128, 8, 1, 1), (8, 64, 16, 1, 0), (64, 4, 16, 1, 0), (128, 128, 2, 1, 0))]
    n_conv = 0
    for g, (cin, cout, H, stride, ups) in convs:
        Ho = H * 2 if ups else H // stride
        n_conv += other(desc(2 * Ho * Ho, cout, 9 * cin, g, conv=1, conv_src=PTR, conv_c=cin, batch=2, Hin=H, Win=H, stride=stride, upsample=ups), g)
    print(f"gemm exact pins: test_gemm_plain {n_plain} of {len(plain)} combinations plan another kernel than the id names, "
          f"test_conv3x3 {n_conv} of {len(convs)}")
