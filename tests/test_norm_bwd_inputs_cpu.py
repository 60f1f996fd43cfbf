"""The conditions that keep tests/test_gpu_norm_bwd.py and tests/test_gpu_pointwise.py honest, checked from the reference alone (no GPU,
no library): the exact inputs are exact, the launch geometry behind the depth functions is the cases', and plain fp32 arithmetic -- torch's
own where torch has the operation -- meets every bound the HIP kernels are held to.  If the reference cannot meet a bound, the bound's
derivation is wrong, not the inputs."""
import pytest
import torch

from tests import helpers_norm as hn
from tests import helpers_norm_bwd as hb

EPS = 1e-5
G = hn.G
LN_IDS = [f"{m}x{c}" for m, c in hb.LN_CASES]


def _is_bf16(t):
    return t.dtype == torch.bfloat16 or torch.equal(t.to(torch.bfloat16).float(), t.float())


# ----------------------------------------------------------------------------- the exact inputs are what they claim
@pytest.mark.parametrize("case", hb.GN_CASES, ids=hn.case_id)
def test_groupnorm_exact_operands_are_exact_in_fp32(case):
    B, C0, C1, HW = case
    C = C0 + C1
    cpg = C // G
    o = hb.gn_exact_operands(B, C, HW)
    assert all(_is_bf16(o[k]) for k in ("x", "dy", "gamma", "pre")) and _is_bf16(o["stats"])
    mean = o["stats"][..., 0].repeat_interleave(cpg, dim=1)[:, None, :]
    rstd = o["stats"][..., 1].repeat_interleave(cpg, dim=1)[:, None, :]
    xh = (o["x"].float() - mean) * rstd
    assert torch.equal(xh * 2, (xh * 2).round()) and float(xh.abs().max()) <= 4 and float((o["x"].float() - mean).abs().max()) == 2
    assert set(o["gamma"].tolist()) == set(hb.GAMMAS) and float(o["dy"].float().abs().max()) == 3 and float(o["pre"].float().abs().max()) == 4
    assert len(set(o["stats"][..., 0].flatten().tolist())) == min(4, B * G) and len(set(o["stats"][..., 1].flatten().tolist())) == 3
    # the largest |sum| in units of its lsb: gamma dz x^ is a multiple of 1/4 and at most 2 * 3 * 4 (a group), dz x^ of 1/2 and at most 12 (a channel)
    assert HW * cpg * 24 * 4 < 2 ** 24 and B * HW * 12 * 2 < 2 ** 24
    r = hb.gn_bwd64(o["x"], o["dy"], o["gamma"], o["beta"], o["stats"], 0)
    for k in ("s1", "s2", "dgamma", "dbeta"):
        assert torch.equal(r[k].float().double(), r[k]), k
    if case in hb.GN_POW2_CASES:
        n = HW * cpg
        assert n & (n - 1) == 0
        for pre in (None, o["pre"]):
            want = r["dx"] if pre is None else r["dx"] + pre.double()
            assert torch.equal(hb.gn_dx_fp32_kernel_order(o["x"], o["dy"], o["gamma"], o["stats"], pre), want.to(torch.bfloat16))
    else:
        got = hb.gn_dx_fp32_kernel_order(o["x"], o["dy"], o["gamma"], o["stats"])
        assert float(((got.double() - r["dx"]).abs() / hb.rounded_bound(r["dx"], r["slack"]).clamp_min(1e-300)).max()) <= 1


@pytest.mark.parametrize("M,C", hb.LN_CASES, ids=LN_IDS)
def test_layernorm_exact_operands_are_exact_in_fp32(M, C):
    o = hb.ln_exact_operands(M, C)
    x = o["x"].float()
    assert bool((x.abs() == o["a"][:, None]).all()) and bool((x.sum(dim=1) == 0).all()) and set(o["a"].tolist()) <= {1.0, 2.0, 4.0}
    assert C * 2 * 3 * 2 < 2 ** 24 and M * 3 < 2 ** 24
    r = hb.ln_bwd64(o["x"], o["dy"], o["gamma"], 0.0)
    assert torch.equal(r["xh"].abs(), torch.ones(M, C, dtype=torch.float64)) and torch.equal(r["rstd"], 1.0 / o["a"].double())
    for pre in (None, o["pre"]):
        want = r["dx"] if pre is None else r["dx"] + pre.double()
        got = hb.ln_dx_fp32_kernel_order(o["x"], o["dy"], o["gamma"], 0.0, pre)
        if C in hb.LN_POW2_WIDTHS:
            assert C & (C - 1) == 0 and torch.equal(got, want.to(torch.bfloat16))
        else:
            assert float(((got.double() - want).abs() / hb.rounded_bound(want, r["slack"]).clamp_min(1e-300)).max()) <= 1


# ----------------------------------------------------------------------------- the geometry the depth functions are computed from
def test_backward_cases_have_the_geometry_they_are_there_for():
    """(PL, chunks, pixels per chunk) as norm.h gn_two_kernel_geometry computes them for groupnorm_bwd_launch's target of 512, and the
    depths that follow; LayerNorm: 16 rows per wave, every instantiation on both sides of its boundary."""
    geo = {c: hn.two_kernel_geometry(c[0], c[1] + c[2], c[3]) for c in hb.GN_CASES}
    assert geo[(1, 320, 0, 1000)] == (6, 63, 16)
    assert geo[(2, 128, 0, 4100)] == (16, 64, 65)
    assert geo[(1, 1280, 640, 1024)] == (1, 64, 16)
    assert geo[(1, 64, 0, 5)] == (5, 1, 5)
    assert geo[(3, 1280, 768, 1)] == (1, 1, 1) and (1280 + 768) // 8 == 256
    assert geo[(1, 256, 0, 1024)] == (8, 64, 16)
    assert geo[(2, 64, 64, 64)] == (16, 4, 16)
    depth = {c: hb.gn_bwd_depth(c[0], c[1] + c[2], c[3]) for c in hb.GN_CASES}
    assert depth == {(1, 320, 0, 1000): 3 + 6 + 63, (2, 128, 0, 4100): 5 + 16 + 128, (1, 1280, 640, 1024): 16 + 1 + 64, (1, 64, 0, 5): 1 + 5 + 1,
                     (3, 1280, 768, 1): 1 + 1 + 3, (1, 256, 0, 1024): 2 + 8 + 64, (2, 64, 64, 64): 1 + 16 + 8}
    assert hb.ln_rows_per_wave() == 16 and [hb.ln_bwd_depth(m) for m, _ in hb.LN_CASES] == [21, 21, 23, 22, 24, 21, 22, 25, 23]
    assert [hb.ln_instantiation(c) for _, c in hb.LN_CASES] == [1, 1, 1, 2, 2, 4, 4, 1, 4]


# ----------------------------------------------------------------------------- the reference alone passes leg B
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("kind", hb.GN_KINDS)
@pytest.mark.parametrize("case", hb.GN_CASES, ids=hn.case_id)
def test_fp32_groupnorm_backward_passes_the_conditioning_leg(case, kind, silu):
    """dx: torch's fp32 group_norm(+silu) autograd rounded to bf16, under the evaluation rows' rule against fp64 autograd.  dgamma, dbeta: the
    sums a kernel forms, in plain fp32 from the handed statistics, within (D + 4) u sum|terms| of fp64 at those statistics."""
    B, C0, C1, HW = case
    C = C0 + C1
    x = hb.gn_input(case, kind)
    gamma, beta = hn.affine(C)
    dy = hb.randn_bf16((B, HW, C), 71)
    stats = hb.stats64_as_fp32(x, EPS)
    ax, _, _ = hb.gn_autograd64(x, dy, gamma, beta, EPS, silu)
    xin = x.float().permute(0, 2, 1).requires_grad_(True)
    y = torch.nn.functional.group_norm(xin, G, gamma, beta, EPS)
    (tx,) = torch.autograd.grad(torch.nn.functional.silu(y) if silu else y, xin, dy.float().permute(0, 2, 1))
    tx = tx.permute(0, 2, 1).to(torch.bfloat16)
    figs = hn.output_figures(tx, ax)
    assert hn.output_ok(figs), figs
    if kind == "const":
        cf = hn.output_figures(hb.const_slices(tx, B, C), hb.const_slices(ax, B, C))
        assert hn.output_ok(cf), cf
    r = hb.gn_bwd64(x, dy, gamma, beta, stats, silu)
    assert hn.rel(r["dx"], ax) < 1e-5, "fp64 at the rounded statistics is fp64 autograd up to that rounding"
    D = hb.gn_bwd_depth(B, C, HW)
    pg, pb = hb.gn_sums_fp32(x, dy, gamma, beta, stats, silu)
    rg, rb = hb.sum_ratio(pg, r["dgamma"], r["tg"], D)[0], hb.sum_ratio(pb, r["dbeta"], r["tb"], D)[0]
    assert rg <= 1 and rb <= 1, (rg, rb)


def test_a_mean_rounded_to_fp32_is_the_kernels_operand():
    """Why dgamma is compared with fp64 at the handed statistics: ten elements a group at |mean| / std = 64, no SiLU.  The same fp32 sums are
    well inside (D + 4) u sum|terms| of fp64 at the fp32 mean they were computed from, and outside it against fp64 autograd, whose mean has
    not been rounded."""
    B, C0, C1, HW = case = (1, 64, 0, 5)
    x = hb.gn_input(case, "R64")
    gamma, beta = hn.affine(C0)
    dy = hb.randn_bf16((B, HW, C0), 71)
    stats = hb.stats64_as_fp32(x, EPS)
    r = hb.gn_bwd64(x, dy, gamma, beta, stats, 0)
    _, ag, _ = hb.gn_autograd64(x, dy, gamma, beta, EPS, 0)
    pg, _ = hb.gn_sums_fp32(x, dy, gamma, beta, stats, 0)
    D = hb.gn_bwd_depth(B, C0, HW)
    assert hb.sum_ratio(pg, r["dgamma"], r["tg"], D)[0] <= 0.5 and hb.sum_ratio(pg, ag, r["tg"], D)[0] > 1


@pytest.mark.parametrize("M,C", hb.LN_CASES, ids=LN_IDS)
def test_fp32_layernorm_backward_passes_the_conditioning_leg(M, C):
    """dx: torch's fp32 layer_norm autograd rounded to bf16 under the evaluation rows' rule; dgamma, dbeta: the sums a kernel forms, in plain fp32"""
    o = hb.ln_offset_operands(M, C)
    x = o["x"].double()
    R = x.mean(dim=1).abs() / x.std(dim=1, unbiased=False).clamp_min(1e-30)
    live = ~o["const"]
    assert bool((x[o["const"]] == hn.CONST_VALUE).all()) and int(o["const"].sum()) == (hb.LN_CONST_ROWS if M > hb.LN_CONST_ROWS else 0)
    assert float(R[live].min()) >= 0.9 * 8 and float(R[live].max()) <= 1.1 * 64
    r = hb.ln_bwd64(o["x"], o["dy"], o["gamma"], hb.LN_EPS)
    if bool(o["const"].any()):
        gd = o["gamma"].double() * o["dy"].double()[o["const"]]
        want = (gd - gd.mean(dim=1, keepdim=True)) * hn.f32(hb.LN_EPS) ** -0.5
        assert torch.allclose(r["dx"][o["const"]], want, rtol=1e-12, atol=0) and not bool(r["xh"][o["const"]].any())
    tx, _, _ = hb.torch_fp32_ln_bwd(o["x"], o["dy"], o["gamma"], hb.LN_EPS)
    figs = hn.output_figures(tx, r["dx"])
    assert hn.output_ok(figs), figs
    D = hb.ln_bwd_depth(M)
    pg, pb = hb.ln_sums_fp32(o["x"], o["dy"], hb.LN_EPS)
    rg, rb = hb.sum_ratio(pg, r["dgamma"], r["tg"], D)[0], hb.sum_ratio(pb, r["dbeta"], r["tb"], D)[0]
    assert rg <= 1 and rb <= 1, (rg, rb)


# ----------------------------------------------------------------------------- the pointwise sweeps
def test_the_sweep_is_every_finite_bf16_value():
    v = hb.bf16_sweep()
    assert v.numel() == 65285 and v.numel() % 256 == 5 and len(set(v.view(torch.int16).tolist())) == 65280
    f = v.float()
    assert float(f.max()) == 2.0 ** 127 * (2 - 2.0 ** -7) and float(f.min()) == -float(f.max()) and int((f == 0).sum()) == 3
    assert float(f[f > 0].min()) == 2.0 ** -133 and torch.equal(v[:5], v[-5:])
    for N2 in hb.GEGLU_WIDTHS:
        assert (hb.geglu_rows(N2) * (N2 // 16)) % 256 != 0 and hb.geglu_rows(N2) * (N2 // 2) >= v.numel()


def _smallest_power_of_two(k):
    p = 1
    while p < k:
        p *= 2
    return p


def test_fp32_activations_set_K():
    """K of (half a bf16 ulp) + K u |ref| + 2^-133: torch's fp32 evaluation of the kernels' formulas passes with the recorded CPU_K_*, the
    smallest power of two that does; the device gets 4 x that.  leaky_relu is bit-equal to bf16(fp64) already in fp32."""
    sweep = hb.bf16_sweep()
    n = sweep.numel()
    worst = 0.0
    for kind in (hb.ACT_SILU, hb.ACT_LEAKY, hb.ACT_TANH):
        ref = hb.act_fwd64(kind, sweep)
        got = hb.act_fwd_fp32(kind, sweep)
        k, odd = hb.measured_k(got, ref)
        assert odd == 0
        worst = max(worst, k)
        if kind == hb.ACT_LEAKY:
            assert torch.equal(got, ref.to(torch.bfloat16))
    assert abs(worst - hb.CPU_K_FWD_MEASURED) <= 0.01 * max(worst, 1) and hb.CPU_K_FWD == _smallest_power_of_two(worst) and hb.K_FWD == 4 * hb.CPU_K_FWD
    worst = 0.0
    dyb = hb.cycle_like(hb.DY_CYCLE, n)
    for kind in (hb.ACT_SILU, hb.ACT_LEAKY, hb.ACT_TANH):
        for ref_f32 in (0, 1):
            for dy_f32 in (0, 1):
                r = sweep.float() * hb.F32_FORM if ref_f32 else sweep
                d = dyb.float() * hb.F32_FORM if dy_f32 else dyb
                for scale in hb.SCALES:
                    inside = r.double().abs() < 2.0 ** 64 if kind == hb.ACT_TANH else None
                    k, odd = hb.measured_k(hb.act_bwd_fp32(kind, r, d, scale), hb.act_bwd_ref64(kind, r, d, scale), inside)
                    assert odd == 0
                    worst = max(worst, k)
    assert abs(worst - hb.CPU_K_BWD_MEASURED) <= 0.01 * max(worst, 1) and hb.CPU_K_BWD == _smallest_power_of_two(worst) and hb.K_BWD == 4 * hb.CPU_K_BWD


@pytest.mark.parametrize("N2", hb.GEGLU_WIDTHS)
def test_fp32_geglu_formulas_pass_their_bounds(N2):
    """geglu_fwd_kernel's and geglu_bwd_kernel's formulas in fp32 on the CPU (erf_as_f restated; libm's exp for the hardware's)"""
    v, g, d = hb.geglu_operands(N2)
    ry = v.double() * hb.gelu64(g)
    rdv, rdg = d.double() * hb.gelu64(g), d.double() * v.double() * hb.dgelu64(g)
    dv, dg = hb.geglu_bwd_fp32(v, g, d)
    assert hb.worst_over_bound(hb.geglu_fwd_fp32(v, g), ry, hb.geglu_fwd_bound(v, g, ry)) <= 1
    assert hb.worst_over_bound(dv, rdv, hb.geglu_dv_bound(d, g, rdv)) <= 1
    assert hb.worst_over_bound(dg, rdg, hb.geglu_dg_bound(d, v, rdg)) <= 1
    # what the bounds are there for: gelu_erf_f itself (the GEMM epilogues') misses the forward bound below -3.5, by its documented
    # 5.5e-7 absolute, and returns -7.3e-9 |g| beyond its clamp (2^P(4 sqrt 2) / 2 per unit of |g|; the bound allows 1e-8)
    e = hb.gelu_erf_f_fp32(g).double()
    assert float((e - hb.gelu64(g)).abs()[g.float().abs() < 8].max()) < 5.5e-7
    far = g.float() < -1e6
    tail = e[far] / g.double()[far].abs()
    assert bool(((tail > -1e-8) & (tail < -7e-9)).all())
