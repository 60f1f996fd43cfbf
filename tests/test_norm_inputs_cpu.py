"""The conditions that keep tests/test_gpu_norm_stats.py honest, checked from the reference alone (no GPU, no library): the inputs are
as hard as they claim, and torch's own fp32 GroupNorm meets every bound the HIP kernels are held to.  If the reference cannot meet a
bound, the bound's derivation is wrong -- not the inputs."""
import pytest
import torch

from tests import helpers_norm as hn

EPS = 1e-5
STAT_CASES = hn.TWO_KERNEL_CASES + hn.ONE_SLAB_CASES + hn.GROUP_QUAD_CASES + [(B, C, 0, HW) for B, C, HW in hn.FOLD_CASES]


def _depth(case):
    """the smallest D a HIP path is given for the shape: the reference is held to the tightest bound any kernel is"""
    B, C0, C1, HW = case
    d = [hn.two_kernel_depth(B, C0 + C1, HW)]
    if case in hn.ONE_SLAB_CASES:
        d.append(hn.one_slab_depth(C0 + C1, HW))
    if case in hn.GROUP_QUAD_CASES:
        d.append(hn.group_quad_depth(B, C0 + C1, HW))
    return min(d)


@pytest.mark.parametrize("case", STAT_CASES, ids=hn.case_id)
def test_exact_sum_cases_are_exact_in_fp32(case):
    B, C0, C1, HW = case
    C = C0 + C1
    assert (C // hn.G) * HW * 9 < 2 ** 24
    x = hn.exact_input(B, C, HW)
    assert torch.equal(x.float(), x.float().round()) and float(x.float().abs().max()) == 3.0
    _, var, _ = hn.stats64(x)
    assert float(var.min()) > 0.5, "no constant group in the exact-sum data"
    # Leg A from the reference.  Its mean bound is that of ONE division of an exact sum, which is what every HIP path does; torch's
    # native_group_norm updates a running mean (Welford) and never holds that sum, so its mean is held to leg B's bound and the
    # division rule is checked on what it describes: torch's fp32 sums (another order than any kernel's, exact all the same).
    st = hn.torch_fp32_stats(x, EPS)
    xg = hn._grouped(x.float())
    n = float(HW * (C // hn.G))
    s, q = xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))
    assert torch.equal(s.double(), hn._grouped(x.double()).sum(dim=(1, 3))) and torch.equal(q.double(), hn._grouped(x.double()).pow(2).sum(dim=(1, 3)))
    mean = s / n
    one_pass = torch.stack([mean, torch.rsqrt(torch.clamp(q / n - mean * mean, min=0.0) + EPS)], dim=-1)
    r = hn.exact_leg(one_pass, x, EPS, True, _depth(case))
    assert r["mean"] <= 1 and r["rstd"] <= 1, r
    st_div = torch.stack([mean, st[..., 1]], dim=-1)
    for one_pass_rule in (True, False):
        r = hn.exact_leg(st_div, x, EPS, one_pass_rule, _depth(case))
        assert r["mean"] <= 1 and r["rstd"] <= 1, (one_pass_rule, r)
    r = hn.conditioning_leg(st, x, EPS, False, _depth(case))
    assert r["var"] <= 1 and r["mean"] <= 1, r


def test_producer_cases_are_exact_in_fp32():
    for C, HW, _ in hn.PRODUCER_CASES:
        assert (C // hn.G) * HW * 9 < 2 ** 24
        a, w, bias, out = hn.producer_operands(C, HW, 0)
        assert torch.equal(a.reshape(out.shape), out) and not bias.any() and torch.equal(w.float(), torch.eye(C))


def _pairwise_sum(t):
    """fp32 sum over the last dim as a pairwise tree (zero padding to a power of two adds nothing): ceil(log2 n) dependent additions"""
    n = t.shape[-1]
    t = torch.nn.functional.pad(t, (0, (1 << (n - 1).bit_length()) - n))
    while t.shape[-1] > 1:
        h = t.shape[-1] // 2
        t = t[..., :h] + t[..., h:]
    return t[..., 0]


def _check_offset_groups(x, R):
    mean, var, _ = hn.stats64(x)
    Rg = mean.abs() / var.sqrt()
    assert 0.9 * R <= float(Rg.min()) and float(Rg.max()) <= 1.1 * R, (R, float(Rg.min()), float(Rg.max()))
    xg = hn._grouped(x.float())
    B = x.shape[0]
    distinct = min(len(torch.unique(xg[b, :, g, :])) for b in range(B) for g in range(hn.G))
    assert distinct >= 3, distinct
    sign = torch.sign(mean)
    assert torch.equal(sign, hn.group_signs().expand_as(sign)), "the sign of the offset alternates by group"


@pytest.mark.parametrize("R", hn.OFFSETS)
@pytest.mark.parametrize("case", STAT_CASES, ids=hn.case_id)
def test_offset_cases_reach_their_condition_number(case, R):
    B, C0, C1, HW = case
    _check_offset_groups(hn.offset_input(B, C0 + C1, HW, R), R)


@pytest.mark.parametrize("R", hn.OFFSETS)
def test_producer_offset_comes_from_the_bias(R):
    for C, HW, _ in hn.PRODUCER_CASES:
        a, w, bias, out = hn.producer_operands(C, HW, R)
        assert float(a.float().abs().max()) < 8 and float(bias.abs().min()) == R      # the GEMM's operand carries no offset
        _check_offset_groups(out, R)


@pytest.mark.parametrize("R", hn.OFFSETS)
@pytest.mark.parametrize("case", STAT_CASES, ids=hn.case_id)
def test_torch_fp32_statistics_pass_the_conditioning_leg(case, R):
    """torch.native_group_norm sits inside the bound the one-pass paths are given, on every case.  It keeps a running mean and centred sum
    whose updates round at the size of x, so its own constant grows with R (K = err / u: 6.5, 54, 55 at R = 8, 32, 64 on the ten
    elements of (1, 64, 0, 5), where the kappa = 1 bound is 2 (12 + 4) = 32; 5, 15, 32 on (8, 264, 248, 16)): the bound WITHOUT kappa is
    not its bound.  That one is held by a plain fp32 two-pass restatement (mean, then the mean of the centred squares: what the one-slab
    and group-quad kernels do) whose order is stated -- a pairwise tree, log2(n) additions deep; torch's own reductions have an order
    and a depth of their own -- under the smallest D any path has for the shape."""
    B, C0, C1, HW = case
    x = hn.offset_input(B, C0 + C1, HW, R)
    r = hn.conditioning_leg(hn.torch_fp32_stats(x, EPS), x, EPS, True, _depth(case))
    assert r["var"] <= 1 and r["mean"] <= 1, r
    n = HW * ((C0 + C1) // hn.G)
    xg = hn._grouped(x.float()).permute(0, 2, 1, 3).reshape(B, hn.G, n)
    mean = _pairwise_sum(xg) / n
    var = _pairwise_sum((xg - mean[..., None]).pow(2)) / n
    assert (n - 1).bit_length() <= _depth(case)                   # the tree is no deeper than the chain the bound is computed for
    two_pass = torch.stack([mean, torch.rsqrt(var + EPS)], dim=-1)
    r = hn.conditioning_leg(two_pass, x, EPS, False, _depth(case))
    assert r["var"] <= 1 and r["mean"] <= 1, r


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("kind", ["R8", "R32", "R64", "const"])
@pytest.mark.parametrize("case", STAT_CASES, ids=hn.case_id)
def test_torch_fp32_groupnorm_passes_the_output_leg(case, kind, silu):
    B, C0, C1, HW = case
    C = C0 + C1
    x = hn.constant_input(B, C, HW) if kind == "const" else hn.offset_input(B, C, HW, int(kind[1:]))
    gamma, beta = hn.affine(C)
    ref = hn.groupnorm64(x, gamma, beta, EPS, silu)
    figs = hn.output_figures(hn.torch_fp32_groupnorm(x, gamma, beta, EPS, silu), ref)
    assert hn.output_ok(figs), figs
    assert 1e-3 < figs[1] < 2.5e-3, figs          # the yardstick is bf16's rounding (2^-9 / sqrt(3) ~ 1.1e-3 .. 2^-8 / sqrt(3))


@pytest.mark.parametrize("case", STAT_CASES, ids=hn.case_id)
def test_constant_groups_normalise_to_beta_exactly(case):
    B, C0, C1, HW = case
    C = C0 + C1
    cpg = C // hn.G
    x = hn.constant_input(B, C, HW)
    gamma, beta = hn.affine(C)
    assert float(beta.abs().min()) >= 0.25 and float(gamma.min()) >= 0.75
    mean, var, _ = hn.stats64(x)
    mask = hn.constant_mask(B)
    assert torch.equal(var == 0, mask) and bool((mean[mask] == hn.CONST_VALUE).all())
    # the sum of a constant group is exact in fp32 as well (n * 201 < 2^24): its fp32 mean is the constant itself
    assert cpg * HW * 201 < 2 ** 24
    ref = hn._grouped(hn.groupnorm64(x, gamma, beta, EPS, 0))
    for g in hn.CONST_GROUPS:
        want = beta[g * cpg:(g + 1) * cpg].double().expand(HW, cpg)
        assert torch.equal(ref[B - 1, :, g, :], want)


def test_two_kernel_cases_have_the_geometry_they_are_there_for():
    """64 chunks at PL = 6; ragged chunks with a short last one; PL = 16; 256-pixel chunks; HW below PL -- as norm.h computes them."""
    geo = {c: hn.two_kernel_geometry(c[0], c[1] + c[2], c[3]) for c in hn.TWO_KERNEL_CASES}
    assert geo[(1, 320, 0, 4096)] == (6, 64, 64)
    assert geo[(1, 320, 0, 1000)] == (6, 63, 16)             # 62 * 16 + 8: the 8-, 4- and 1-unrolled loops all see a tail
    assert geo[(1, 128, 0, 2470)] == (16, 64, 39)            # 63 * 39 + 13
    assert geo[(2, 128, 0, 4100)] == (16, 64, 65)            # 63 * 65 + 5
    assert geo[(1, 128, 0, 16384)] == (16, 64, 256)
    assert geo[(1, 512, 0, 4096)] == (4, 64, 64)
    assert geo[(1, 1280, 640, 1024)] == (1, 64, 16) and (21 * 60 < 1280 < 22 * 60)
    assert geo[(1, 64, 0, 5)] == (5, 1, 5)


def test_group_quad_cases_have_the_geometry_their_depth_is_computed_from():
    """(groups per block, threads, pixel lanes, UNITS) as norm.hip gn_select computes them"""
    assert hn.group_quad_geometry(8, 512, 16) == (2, 256, 32, 4) and hn.group_quad_depth(8, 512, 16) == 4 + 2 + 32 + 4
    assert hn.group_quad_geometry(8, 1920, 256) == (2, 512, 17, 16) and hn.group_quad_depth(8, 1920, 256) == 16 + 2 + 17 + 15
