"""GroupNorm statistics of every path against fp64, at hard inputs and sizes (the inputs, references and bounds: tests/helpers_norm.py;
the conditions that keep them honest: tests/test_norm_inputs_cpu.py).

gn_select (norm.hip) sends a GroupNorm down one of four paths.  The one-slab kernel (census gn_small), the group-quad kernel (gn_mid)
and the Winograd prologue centre on the mean (two passes); the two-kernel path (gn_stats) and the producer statistics (gn_pre,
gn_folded) form sum(x^2) / n - mean^2 in fp32 from raw (sum, sum of squares) records (one pass), which loses 1 + R^2,
R = |mean| / std.  Legs, as the docstrings below name them:
  A  exact-sum data (integers in [-3, 3]: every fp32 sum is exact in any order, so a disagreement is a wrong element set);
  B  offset data at R = 8, 32, 64: the variance within Higham's bound for the path's summation depth D, times kappa_g = 1 + R_g^2 on the
     one-pass paths; the measured constant K = err / (u kappa_g) is printed;
  C  the output under the evaluation rows' rule: rel L2 against fp64 <= 3 x the rel L2 of fp64 rounded once to bf16;
  D  two paths over one tensor agree within the sum of their bounds;
  E  the backward pass fed by these statistics, against fp64 autograd.
Every test asserts through the census that the path it names ran, and prints each figure on a "groupnorm parity" line before asserting
it (profiles/groupnorm_stats_parity.txt holds one run's lines)."""
import pytest
import torch
import torch.nn.functional as F

from difashion_amd import _lib
from tests import gpu_util as gu
from tests import helpers_norm as hn
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

G = hn.G
EPS = 1e-5
GN_KEYS = ("gn_pre", "gn_stats", "gn_small", "gn_mid", "gn_folded")
DEPTH = {"gn_stats": lambda B, Cc, HW: hn.two_kernel_depth(B, Cc, HW), "gn_small": lambda B, Cc, HW: hn.one_slab_depth(Cc, HW),
         "gn_mid": lambda B, Cc, HW: hn.group_quad_depth(B, Cc, HW)}
PATH_CASES = ([("gn_stats", c) for c in hn.TWO_KERNEL_CASES] + [("gn_small", c) for c in hn.ONE_SLAB_CASES] +
              [("gn_mid", c) for c in hn.GROUP_QUAD_CASES])
PATH_IDS = [f"{p}-{hn.case_id(c)}" for p, c in PATH_CASES]


def _say(*parts):
    print("groupnorm parity", *parts)


def _gn_census():
    return {k: v for k, v in _lib.census().items() if k in GN_KEYS}


def _assert_ran(want):
    """exactly the GroupNorm launches `want` ({census key: count}) since the last census_reset()"""
    got = _gn_census()
    assert got == {k: want.get(k, 0) for k in GN_KEYS}, (got, want)
    return " ".join(f"{k}={v}" for k, v in got.items() if v)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _groupnorm_stats(x, C0, C1, gamma, beta, eps, silu):
    """dfh_groupnorm_stats over x [B][HW][C0 + C1] split into its two sources -> (out bf16 [B][HW][C], stats fp32 [B][G][2]), both on the CPU"""
    B, HW, Cc = x.shape
    s0, s1 = _dev(x[..., :C0]), (_dev(x[..., C0:]) if C1 else None)
    gm, bt = _dev(gamma), _dev(beta)
    out = torch.full((B, HW, Cc), float("nan"), dtype=torch.bfloat16, device=DEV)
    part = torch.zeros(B * 64 * G * 2, device=DEV)
    stats = torch.full((B, G, 2), float("nan"), device=DEV)
    _lib.census_reset()
    _lib.call("dfh_groupnorm_stats", _lib.ptr(s0), C0, _lib.ptr(s1), C1, B, HW, G, _lib.ptr(gm), _lib.ptr(bt), eps, silu, _lib.ptr(out),
              _lib.ptr(part), _lib.ptr(stats), gu.stream())
    torch.cuda.synchronize()
    return out.cpu(), stats.cpu()


def _fmt_out(figs):
    e, y, m, finite = figs
    return f"rel_l2 {e:.3e} yardstick {y:.3e} ratio {e / y:.2f} max_rel {m:.2e} finite {finite}"


def _fmt_b(r):
    return (f"R_g {r['R'][0]:.1f}..{r['R'][1]:.1f} rstd_err {r['rstd_err']:.2e} var_err/bound {r['var']:.3f} mean_err/bound {r['mean']:.3f} "
            f"K {r['K']:.2f}")


def _constant_slices(t, B, Cc):
    """the constant groups of the last image out of t [B][HW][C]: [HW][2][cpg]"""
    return t.reshape(t.shape[0], t.shape[1], G, Cc // G)[B - 1][:, list(hn.CONST_GROUPS), :]


def _output_leg(tag, got, x, gamma, beta, eps, silu, const=False):
    """Leg C over the whole tensor and, const, over the constant groups alone (there the fp64 result is beta / silu(beta))."""
    ref = hn.groupnorm64(x, gamma, beta, eps, silu)
    figs = hn.output_figures(got, ref)
    _say(tag, f"silu={silu}", _fmt_out(figs))
    ok = hn.output_ok(figs)
    if const:
        B, _, Cc = x.shape
        cf = hn.output_figures(_constant_slices(got, B, Cc), _constant_slices(ref, B, Cc))
        _say(tag, f"silu={silu} constant groups", _fmt_out(cf))
        ok = ok and hn.output_ok(cf)
    assert ok, (tag, silu, figs)


# ----------------------------------------------------------------------------- dfh_groupnorm_stats: the three paths gn_select picks by shape
@pytest.mark.parametrize("path,case", PATH_CASES, ids=PATH_IDS)
def test_exact_sums_give_exact_statistics(path, case):
    """Leg A.  D per case: hn.two_kernel_depth / one_slab_depth / group_quad_depth (derivations there)."""
    B, C0, C1, HW = case
    Cc = C0 + C1
    x = hn.exact_input(B, Cc, HW)
    gamma, beta = hn.affine(Cc)
    out, stats = _groupnorm_stats(x, C0, C1, gamma, beta, EPS, 0)
    cen = _assert_ran({path: 1})
    D = DEPTH[path](B, Cc, HW)
    r = hn.exact_leg(stats, x, EPS, path in hn.ONE_PASS, D)
    _say("A", path, hn.case_id(case), f"exact D={D} mean_err/bound {r['mean']:.3f} rstd_err/bound {r['rstd']:.3f} census {cen}")
    if path == "gn_stats":
        PL, chunks, ppc = hn.two_kernel_geometry(B, Cc, HW)
        _say("A", path, hn.case_id(case), f"PL={PL} chunks={chunks} pix_per_chunk={ppc} last_chunk={HW - (chunks - 1) * ppc}")
    assert r["mean"] <= 1 and r["rstd"] <= 1, r
    _output_leg(f"C {path} {hn.case_id(case)} exact", out, x, gamma, beta, EPS, 0)


@pytest.mark.parametrize("R", hn.OFFSETS)
@pytest.mark.parametrize("path,case", PATH_CASES, ids=PATH_IDS)
def test_offset_data_statistics_and_output(path, case, R):
    """Legs B and C on randn + R * sign_g, with and without SiLU."""
    B, C0, C1, HW = case
    Cc = C0 + C1
    x = hn.offset_input(B, Cc, HW, R)
    gamma, beta = hn.affine(Cc)
    D = DEPTH[path](B, Cc, HW)
    for silu in (0, 1):
        out, stats = _groupnorm_stats(x, C0, C1, gamma, beta, EPS, silu)
        cen = _assert_ran({path: 1})
        if silu == 0:
            r = hn.conditioning_leg(stats, x, EPS, path in hn.ONE_PASS, D)
            _say("B", path, hn.case_id(case), f"R={R} D={D}", _fmt_b(r), f"census {cen}")
            assert r["var"] <= 1 and r["mean"] <= 1, r
        _output_leg(f"C {path} {hn.case_id(case)} R={R}", out, x, gamma, beta, EPS, silu)


@pytest.mark.parametrize("path,case", PATH_CASES, ids=PATH_IDS)
def test_constant_groups_come_out_as_beta(path, case):
    """Groups 0 and 17 of the last image hold 3.140625 everywhere: variance 0, the one-pass difference is rounding noise on either side of
    zero and the clamp decides.  The output there is beta (silu(beta)); the other groups (R = 8) keep leg B."""
    B, C0, C1, HW = case
    Cc = C0 + C1
    x = hn.constant_input(B, Cc, HW)
    gamma, beta = hn.affine(Cc)
    D = DEPTH[path](B, Cc, HW)
    for silu in (0, 1):
        out, stats = _groupnorm_stats(x, C0, C1, gamma, beta, EPS, silu)
        cen = _assert_ran({path: 1})
        if silu == 0:
            mask = hn.constant_mask(B)
            cs = stats[mask]
            _say("B", path, hn.case_id(case), f"const D={D} constant groups: mean - c {float((cs[:, 0].double() - hn.CONST_VALUE).abs().max()):.2e} "
                 f"rstd {float(cs[:, 1].min()):.1f}..{float(cs[:, 1].max()):.1f} (eps^-1/2 = {hn.f32(EPS) ** -0.5:.1f})")
            assert bool(torch.isfinite(stats).all())
            r = hn.conditioning_leg(stats, x, EPS, path in hn.ONE_PASS, D, skip=mask)
            _say("B", path, hn.case_id(case), f"const D={D}", _fmt_b(r), f"census {cen}")
            assert r["var"] <= 1 and r["mean"] <= 1, r
        _output_leg(f"C {path} {hn.case_id(case)} const", out, x, gamma, beta, EPS, silu, const=True)


# ----------------------------------------------------------------------------- producer statistics: dfh_gemm_gstat -> dfh_groupnorm_pre / dfh_groupnorm_fold
def _one_hot_rows(Cc):
    """[32][C] bf16: row n picks channel n * cpg + n % cpg, one channel of every group"""
    cpg = Cc // G
    cols = torch.tensor([n * cpg + n % cpg for n in range(G)])
    w = torch.zeros(G, Cc)
    w[torch.arange(G), cols] = 1.0
    return w.to(torch.bfloat16), cols


def _fold(x, gamma, beta, eps, w, bias, pre=None, chunks=0):
    """dfh_groupnorm_fold -> (Wimg bf16 [B][N][C], rv fp32 [B][N]) on the device"""
    B, HW, Cc = x.shape
    N = w.shape[0]
    wimg = torch.full((B, N, Cc), float("nan"), dtype=torch.bfloat16, device=DEV)
    rv = torch.full((B, N), float("nan"), device=DEV)
    part = torch.zeros(B * 64 * G * 2, device=DEV)
    keep = (_dev(x), _dev(gamma), _dev(beta), _dev(w), _dev(bias))
    _lib.census_reset()
    _lib.call("dfh_groupnorm_fold", _lib.ptr(keep[0]), B, HW, Cc, G, _lib.ptr(keep[1]), _lib.ptr(keep[2]), eps, _lib.ptr(pre), chunks,
              _lib.ptr(part), _lib.ptr(keep[3]), Cc, N, _lib.ptr(keep[4]), _lib.ptr(wimg), _lib.ptr(rv), gu.stream())
    torch.cuda.synchronize()
    return wimg, rv


def _bf16_ulp(v):
    """the spacing of bf16 at |v| (fp64 tensor)"""
    return torch.exp2(torch.floor(torch.log2(v.abs())) - 7)


def _fold_one_hot_leg(tag, x, eps, D, pre=None, chunks=0):
    """With W a set of one-hot rows, beta = 0 and no bias: Wimg[i][n][c_n] = bf16(gamma rstd) within one bf16 ulp of the fp64 value, every
    other weight 0, and -rv / Wimg is the group mean within leg B's mean bound."""
    B, HW, Cc = x.shape
    gamma, _ = hn.affine(Cc)
    w, cols = _one_hot_rows(Cc)
    wimg, rv = _fold(x, gamma, torch.zeros(Cc), eps, w, None, pre, chunks)
    wimg, rv = wimg.cpu().double(), rv.cpu().double()
    mean64, var64, amax = hn.stats64(x)
    picked = wimg[:, torch.arange(G), cols]                                     # [B][G]
    want = (gamma[cols].double() * (var64 + hn.f32(eps)).rsqrt()).to(torch.bfloat16).double()
    ulps = float(((picked - want).abs() / _bf16_ulp(want)).max())
    rest = wimg.clone()
    rest[:, torch.arange(G), cols] = 0
    merr = float(((-rv / picked - mean64).abs() / ((D + 2) * hn.U * amax)).max())
    _say(tag, f"one-hot D={D} Wimg_ulps {ulps:.2f} mean_err/bound {merr:.3f} stray_weights {int((rest != 0).sum())}")
    assert ulps <= 1 and merr <= 1 and not rest.any(), (ulps, merr)


@pytest.mark.parametrize("Cc,HW,tile", hn.PRODUCER_CASES, ids=[f"{c}-{hw}-tile{t}" for c, hw, t in hn.PRODUCER_CASES])
def test_producer_statistics_from_the_gemm_epilogue(Cc, HW, tile):
    """A linear C -> C (identity weights; the offset comes from the bias, so the epilogue sums the offset values) writes the
    (sum, sum of squares) records of its own bf16 output; dfh_groupnorm_pre and dfh_groupnorm_fold normalise from them.
    R = 0: legs A (the records equal torch's sums exactly).  R = 8, 32, 64: legs B, C and D (against dfh_groupnorm_stats of the same
    tensor, which takes the two-kernel or the one-slab path by its shape).  D = 64 + 4 + cpg + HW / rows (hn.producer_depth)."""
    B, cpg = hn.PRODUCER_B, Cc // G
    M = B * HW
    gamma, beta = hn.affine(Cc)
    gm, bt = _dev(gamma), _dev(beta)
    for R in (0,) + hn.OFFSETS:
        a, w, bias, want = hn.producer_operands(Cc, HW, R)
        gst = torch.full((B * G * (HW // 128) * 2,), float("nan"), dtype=torch.float32, device=DEV)
        _lib.census_reset()
        out, rows = gu.gemm(force_tile=tile, gstat=gst, gstat_cpg=cpg, gstat_hw=HW, M=M, N=Cc, W=_dev(w), ldw=Cc, a0=_dev(a), a0_c=Cc,
                            bias=_dev(bias))
        assert rows == (128 if tile == 10 else 256) and _lib.census()["gstat_written"] == 1, (rows, _lib.census())
        assert torch.equal(out.cpu().view(B, HW, Cc), want), "the GEMM's output is the test data, bit for bit"
        chunks = HW // rows
        D = hn.producer_depth(Cc, HW, rows)
        tag = f"gn_pre {Cc}->{Cc}@{HW} tile{tile} R={R}"
        got = gst[:B * G * chunks * 2].view(B, G, chunks, 2).cpu()
        if R == 0:
            y = want.double().view(B, chunks, rows, G, cpg)
            ref = torch.stack([y.sum(dim=(2, 4)), (y * y).sum(dim=(2, 4))], dim=-1).permute(0, 2, 1, 3).float()
            _say("A", tag, f"records differ in {int((got != ref).sum())} of {ref.numel()}")
            assert torch.equal(got, ref)
        assert bool(torch.isfinite(got).all())
        for silu in (0, 1):
            o_pre = torch.full((B, HW, Cc), float("nan"), dtype=torch.bfloat16, device=DEV)
            stats = torch.full((B, G, 2), float("nan"), device=DEV)
            _lib.census_reset()
            _lib.call("dfh_groupnorm_pre", _lib.ptr(out), Cc, B, HW, G, _lib.ptr(gm), _lib.ptr(bt), EPS, silu, _lib.ptr(o_pre), _lib.ptr(gst), chunks,
                      _lib.ptr(stats), gu.stream())
            torch.cuda.synchronize()
            cen = _assert_ran({"gn_pre": 1})
            stats = stats.cpu()
            if silu == 0 and R == 0:
                r = hn.exact_leg(stats, want, EPS, True, D)
                _say("A", tag, f"exact D={D} mean_err/bound {r['mean']:.3f} rstd_err/bound {r['rstd']:.3f} census {cen}")
                assert r["mean"] <= 1 and r["rstd"] <= 1, r
            if silu == 0 and R:
                rb = hn.conditioning_leg(stats, want, EPS, True, D)
                _say("B", tag, f"D={D}", _fmt_b(rb), f"census {cen}")
                assert rb["var"] <= 1 and rb["mean"] <= 1, rb
                # leg D: the same tensor through dfh_groupnorm_stats
                _, st2 = _groupnorm_stats(want, Cc, 0, gamma, beta, EPS, 0)
                other = next(k for k, v in _gn_census().items() if v)
                cen2 = _assert_ran({other: 1})
                assert other in ("gn_stats", "gn_small")
                D2 = DEPTH[other](B, Cc, HW)
                mean64, var64, amax = hn.stats64(want)
                kap = 1 + mean64 * mean64 / var64
                bound = 2 * (D + 4) * hn.U * kap + 2 * (D2 + 4) * hn.U * (kap if other in hn.ONE_PASS else 1.0)
                v1, v2 = stats[..., 1].double().pow(-2), st2[..., 1].double().pow(-2)
                dv = float(((v1 - v2).abs() / var64 / bound).max())
                dm = float(((stats[..., 0].double() - st2[..., 0].double()).abs() / ((D + D2 + 4) * hn.U * amax)).max())
                _say("D", tag, f"against {other} (D={D2}): var_diff/bound {dv:.3f} mean_diff/bound {dm:.3f} census {cen2}")
                assert dv <= 1 and dm <= 1, (dv, dm)
            _output_leg(f"C {tag}", o_pre.cpu(), want, gamma, beta, EPS, silu)
        # dfh_groupnorm_fold with the producer's records: the one-hot leg, and (offset data) a random projection under the 3 x rule
        _fold_one_hot_leg(f"A/B gn_folded(pre) {Cc}->{Cc}@{HW} tile{tile} R={R}", want, 1e-6, D, pre=gst, chunks=chunks)
        _assert_ran({"gn_folded": 1})
        if R:
            gen = torch.Generator().manual_seed(31)
            pw = (0.06 * torch.randn(Cc, Cc, generator=gen)).to(torch.bfloat16)
            pb = 0.3 * torch.randn(Cc, generator=gen)
            wimg, rv = _fold(want, gamma, beta, 1e-6, pw, pb, pre=gst, chunks=chunks)
            cen = _assert_ran({"gn_folded": 1})
            proj = gu.gemm(M=M, N=Cc, W=wimg, ldw=Cc, a0=out, a0_c=Cc, rowvec=rv, rv_ld=Cc, rv_off=0, rows_per_b=HW, w_img_stride=Cc * Cc)
            ref = hn.groupnorm64(want, gamma, beta, 1e-6, 0) @ pw.double().t() + pb.double()
            figs = hn.output_figures(proj.cpu().view(B, HW, Cc), ref)
            _say("C", f"gn_folded(pre) {Cc}->{Cc}@{HW} tile{tile} R={R} projection", _fmt_out(figs), f"census {cen}")
            assert hn.output_ok(figs), figs


def test_producer_statistics_of_constant_groups():
    """Constant groups through the epilogue (tile 21, 320 channels, 1024 pixels): the bias is 0 on groups 0 and 17 and the operand holds
    3.140625 there in the last image; R = 8 elsewhere."""
    Cc, HW, tile, B = 320, 1024, 21, hn.PRODUCER_B
    cpg, M = Cc // G, hn.PRODUCER_B * HW
    a, w, bias, _ = hn.producer_operands(Cc, HW, 8)
    a = a.clone().view(B, HW, G, cpg)
    bias = bias.clone().view(G, cpg)
    for g in hn.CONST_GROUPS:
        a[B - 1, :, g, :] = hn.CONST_VALUE
        bias[g] = 0.0
    a, bias = a.view(M, Cc), bias.view(Cc)
    want = (a.float() + bias).to(torch.bfloat16).view(B, HW, Cc)
    gamma, beta = hn.affine(Cc)
    gst = torch.full((B * G * (HW // 128) * 2,), float("nan"), dtype=torch.float32, device=DEV)
    out, rows = gu.gemm(force_tile=tile, gstat=gst, gstat_cpg=cpg, gstat_hw=HW, M=M, N=Cc, W=_dev(w), ldw=Cc, a0=_dev(a), a0_c=Cc, bias=_dev(bias))
    assert rows == 256 and torch.equal(out.cpu().view(B, HW, Cc), want)
    mask = hn.constant_mask(B)
    _, var64, _ = hn.stats64(want)
    assert torch.equal(var64 == 0, mask)
    gm, bt = _dev(gamma), _dev(beta)
    D = hn.producer_depth(Cc, HW, rows)
    for silu in (0, 1):
        o_pre = torch.full((B, HW, Cc), float("nan"), dtype=torch.bfloat16, device=DEV)
        stats = torch.full((B, G, 2), float("nan"), device=DEV)
        _lib.census_reset()
        _lib.call("dfh_groupnorm_pre", _lib.ptr(out), Cc, B, HW, G, _lib.ptr(gm), _lib.ptr(bt), EPS, silu, _lib.ptr(o_pre), _lib.ptr(gst), HW // rows,
                  _lib.ptr(stats), gu.stream())
        torch.cuda.synchronize()
        cen = _assert_ran({"gn_pre": 1})
        if silu == 0:
            r = hn.conditioning_leg(stats.cpu(), want, EPS, True, D, skip=mask)
            _say("B", f"gn_pre {Cc}@{HW} tile{tile} const D={D}", _fmt_b(r), f"census {cen}")
            assert r["var"] <= 1 and r["mean"] <= 1, r
        _output_leg(f"C gn_pre {Cc}@{HW} tile{tile} const", o_pre.cpu(), want, gamma, beta, EPS, silu, const=True)


# ----------------------------------------------------------------------------- dfh_groupnorm_fold summing the tensor itself (gn_stats + gn_folded)
@pytest.mark.parametrize("B,Cc,HW", hn.FOLD_CASES, ids=[hn.case_id(c) for c in hn.FOLD_CASES])
def test_fold_statistics_and_projection(B, Cc, HW):
    """dfh_groupnorm_fold with pre = NULL runs gn_stats_kernel itself, whatever the shape.  One-hot rows read its rstd and mean back
    (legs A and B); with a random W the folded projection Wimg . x + rv agrees with fp64 W . GN(x) + bias under the 3 x rule (leg C)."""
    D = hn.two_kernel_depth(B, Cc, HW)
    tagc = f"gn_folded {hn.case_id((B, Cc, HW))}"
    data = [("exact", hn.exact_input(B, Cc, HW))] + [(f"R={R}", hn.offset_input(B, Cc, HW, R)) for R in hn.OFFSETS]
    for name, x in data:
        _fold_one_hot_leg(f"A/B {tagc} {name}", x, 1e-6, D)
        _assert_ran({"gn_stats": 1, "gn_folded": 1})
    gamma, beta = hn.affine(Cc)
    gen = torch.Generator().manual_seed(23)
    w = (0.06 * torch.randn(Cc, Cc, generator=gen)).to(torch.bfloat16)
    bias = 0.3 * torch.randn(Cc, generator=gen)
    for name, x in data[1:] + [("const", hn.constant_input(B, Cc, HW))]:
        wimg, rv = _fold(x, gamma, beta, 1e-6, w, bias)
        cen = _assert_ran({"gn_stats": 1, "gn_folded": 1})
        xd = _dev(x)
        if HW % 128 == 0:          # per-image weights in one launch (images of whole row tiles)
            out = gu.gemm(M=B * HW, N=Cc, W=wimg, ldw=Cc, a0=xd.view(B * HW, Cc), a0_c=Cc, rowvec=rv, rv_ld=Cc, rv_off=0, rows_per_b=HW,
                          w_img_stride=Cc * Cc).view(B, HW, Cc)
        else:                      # ... else image by image, each with its own weights and row vector
            out = torch.stack([gu.gemm(M=HW, N=Cc, W=wimg[i], ldw=Cc, a0=xd[i], a0_c=Cc, rowvec=rv[i:i + 1].contiguous(), rv_ld=Cc, rv_off=0,
                                       rows_per_b=HW) for i in range(B)])
        ref = hn.groupnorm64(x, gamma, beta, 1e-6, 0) @ w.double().t() + bias.double()
        figs = hn.output_figures(out.cpu(), ref)
        _say("C", tagc, name, "projection", _fmt_out(figs), f"census {cen}")
        assert hn.output_ok(figs), figs


# ----------------------------------------------------------------------------- dfh_groupnorm_fp8
@pytest.mark.parametrize("case", [(1, 320, 0, 4096), (1, 320, 0, 1000), (2, 128, 0, 2470)], ids=hn.case_id)
def test_fp8_output_on_hard_inputs(case):
    """test_groupnorm_fp8_output_is_the_normalised_value_under_the_static_scale's rule (no NaN, rel L2 <= 4e-2 of the normalised value
    without affine, eps 1e-6, scale 14) on the offset and constant-group data, against fp64; two-kernel path and one-slab path."""
    B, Cc, _, HW = case
    path = "gn_small" if case in hn.ONE_SLAB_CASES else "gn_stats"
    for name, x in [(f"R={R}", hn.offset_input(B, Cc, HW, R)) for R in hn.OFFSETS] + [("const", hn.constant_input(B, Cc, HW))]:
        xd = _dev(x)
        q = torch.full((B, HW, Cc), 0x7f, dtype=torch.uint8, device=DEV)
        part = torch.zeros(B * 64 * G * 2, device=DEV)
        _lib.census_reset()
        _lib.call("dfh_groupnorm_fp8", _lib.ptr(xd), B, HW, Cc, G, 1e-6, 14.0, _lib.ptr(q), _lib.ptr(part), gu.stream())
        torch.cuda.synchronize()
        cen = _assert_ran({path: 1})
        got = q.view(torch.float8_e4m3fn).float().cpu() / 14.0
        ref = hn.groupnorm64(x, None, None, 1e-6, 0, affine_on=False)
        e = hn.rel(got, ref)
        _say("C", f"fp8 {path} {hn.case_id(case)} {name} rel_l2 {e:.3e} nan {int(torch.isnan(got).sum())} census {cen}")
        assert not torch.isnan(got).any() and e <= 4e-2, e


# ----------------------------------------------------------------------------- the Winograd prologue against the two-launch path
@pytest.mark.parametrize("B,C0,C1,H,W", [(3, 1280, 640, 8, 8), (2, 128, 128, 4, 6)])
def test_winograd_prologue_agrees_with_groupnorm_then_transform(B, C0, C1, H, W):
    """Leg D on R = 32 data: V = B^T silu(GroupNorm(concat)) B from gn_wino_input_kernel (its own two-pass statistics, no census key: no
    GroupNorm launch is counted) against dfh_groupnorm (two-kernel / one-slab by shape) + dfh_wino_input, under
    test_groupnorm_silu_fused_into_the_winograd_input_transform's 2e-3; and both against the fp64 result rounded once."""
    Cc, HW = C0 + C1, H * W
    assert _lib.raw().dfh_gn_wino_input_ok(C0, C1, G, H, W)
    x = hn.offset_input(B, Cc, HW, 32)
    gamma, beta = hn.affine(Cc)
    s0, s1, gm, bt = _dev(x[..., :C0]), _dev(x[..., C0:]), _dev(gamma), _dev(beta)
    mt = B * (H // 2) * (W // 2)
    Vf = torch.full((16, mt, Cc), float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.census_reset()
    _lib.call("dfh_gn_wino_input", _lib.ptr(s0), C0, _lib.ptr(s1), C1, _lib.ptr(gm), _lib.ptr(bt), EPS, G, _lib.ptr(Vf), B, H, W, gu.stream())
    torch.cuda.synchronize()
    _assert_ran({})
    gn = torch.empty(B, HW, Cc, dtype=torch.bfloat16, device=DEV)
    part = torch.zeros(B * 64 * G * 2, device=DEV)
    Vu = torch.full_like(Vf, float("nan"))
    _lib.call("dfh_groupnorm", _lib.ptr(s0), C0, _lib.ptr(s1), C1, B, HW, G, _lib.ptr(gm), _lib.ptr(bt), EPS, 1, _lib.ptr(gn), _lib.ptr(part), gu.stream())
    _lib.call("dfh_wino_input", _lib.ptr(gn), _lib.ptr(Vu), B, H, W, Cc, gu.stream())
    torch.cuda.synchronize()
    other = next(k for k, v in _gn_census().items() if v)
    cen = _assert_ran({other: 1})
    ref = hn.groupnorm64(x, gamma, beta, EPS, 1).to(torch.bfloat16).double().view(B, H, W, Cc).permute(0, 3, 1, 2)
    BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1.]], dtype=torch.float64)
    patches = F.pad(ref, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)
    Vref = torch.einsum("ij,bcyxjk,lk->ilbyxc", BT, patches, BT).reshape(16, mt, Cc)
    d, ef, eu = hn.rel(Vf.cpu(), Vu.cpu()), hn.rel(Vf.cpu(), Vref), hn.rel(Vu.cpu(), Vref)
    _say("D", f"wino {B}x{C0}+{C1}x{H}x{W} R=32 fused vs {other} + transform {d:.3e}; vs fp64: fused {ef:.3e} two-launch {eu:.3e} census {cen}")
    assert bool(torch.isfinite(Vf.float()).all()) and d <= 2e-3 and ef <= 2e-3, (d, ef)


# ----------------------------------------------------------------------------- backward
@pytest.mark.parametrize("case", hn.BACKWARD_CASES, ids=hn.case_id)
def test_backward_from_one_pass_statistics(case):
    """Leg E: dfh_groupnorm_bwd fed by dfh_groupnorm_stats (two-kernel path) on R = 32 data, against fp64 autograd; tolerances of
    test_groupnorm_backward (tests/test_gpu_backward.py), unchanged."""
    B, C0, C1, HW = case
    Cc, silu = C0 + C1, 1
    x = hn.offset_input(B, Cc, HW, 32)
    gamma, beta = hn.affine(Cc)
    gen = torch.Generator().manual_seed(29)
    dy = torch.randn(B, HW, Cc, generator=gen).to(torch.bfloat16)
    pre0 = torch.randn(B, HW, C0, generator=gen).to(torch.bfloat16)            # existing gradient contents to accumulate into
    s0, s1, gm, bt, dyd = _dev(x[..., :C0]), (_dev(x[..., C0:]) if C1 else None), _dev(gamma), _dev(beta), _dev(dy)
    out = torch.empty(B, HW, Cc, dtype=torch.bfloat16, device=DEV)
    part = torch.zeros(B * 64 * G * 2, device=DEV)
    stats = torch.full((B, G, 2), float("nan"), device=DEV)
    _lib.census_reset()
    _lib.call("dfh_groupnorm_stats", _lib.ptr(s0), C0, _lib.ptr(s1), C1, B, HW, G, _lib.ptr(gm), _lib.ptr(bt), EPS, silu, _lib.ptr(out),
              _lib.ptr(part), _lib.ptr(stats), gu.stream())
    cen = _assert_ran({"gn_stats": 1})
    dx0, dx1 = _dev(pre0).clone(), (torch.empty(B, HW, C1, dtype=torch.bfloat16, device=DEV) if C1 else None)
    dg, db = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    _lib.call("dfh_groupnorm_bwd", _lib.ptr(s0), C0, _lib.ptr(s1), C1, _lib.ptr(dyd), B, HW, G, _lib.ptr(gm), _lib.ptr(bt), _lib.ptr(stats), silu,
              _lib.ptr(dx0), 1, _lib.ptr(dx1), 0, _lib.ptr(dg), _lib.ptr(db), _lib.ptr(part), gu.stream())
    torch.cuda.synchronize()
    xin = x.double().permute(0, 2, 1).requires_grad_(True)                     # [B][C][HW]
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.silu(F.group_norm(xin, G, gr, br, hn.f32(EPS)))
    rx, rg, rb = torch.autograd.grad(y, (xin, gr, br), dy.double().permute(0, 2, 1))
    rx = rx.permute(0, 2, 1)
    got0 = dx0.cpu().float() - pre0.float()
    e0 = gu.rel_err(got0, rx[..., :C0])
    e1 = gu.rel_err(dx1.cpu(), rx[..., C0:]) if C1 else 0.0
    eg, eb = gu.rel_err(dg.cpu(), rg), gu.rel_err(db.cpu(), rb)
    _say("E", f"gn_stats {hn.case_id(case)} R=32 dx0 {e0:.3e} dx1 {e1:.3e} dgamma {eg:.3e} dbeta {eb:.3e} census {cen}")
    gu.assert_close_bf16(got0, rx[..., :C0], "gn dx0 (accumulated)", rel=2e-2, max_rel=5e-2)
    if C1:
        gu.assert_close_bf16(dx1.cpu(), rx[..., C0:], "gn dx1", rel=8e-3, max_rel=4e-2)
    assert eg < 2e-3 and eb < 2e-3, (eg, eb)
