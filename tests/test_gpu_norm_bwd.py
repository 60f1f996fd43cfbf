"""dfh_groupnorm_bwd and dfh_layernorm_bwd against fp64, on exact data and at hard inputs, in every call form of the training walk (the
inputs, references and bounds: tests/helpers_norm_bwd.py; the conditions that keep them honest: tests/test_norm_bwd_inputs_cpu.py).
Legs, as the docstrings below name them:
  A  exact data: every operand and every sum is a small dyadic rational, exact in fp32 in any order, atomics included.  dbeta and dgamma
     are bit-equal to fp64; the chunk records gn_bwd_stats_kernel leaves in `partial` sum exactly to the fp64 group sums (this is what sees
     a pixel counted twice or never); dx is bit-equal to bf16(fp64) where n is a power of two and within the correctly-rounded bound elsewhere.
     GroupNorm is HANDED its statistics (mean in -1, 0, 1, 2, rstd in 0.5, 1, 2); LayerNorm gets rows of +-a with eps = 0.
  B  conditioning: |mean| / std = 8, 32, 64 and constant groups / rows.  dx under the evaluation rows' rule against fp64 autograd; dgamma
     and dbeta per channel within (D + 4) u sum|terms| of fp64 on the operands the kernel received.
Every case runs with (acc0, acc1) / accumulate in every combination, into buffers that hold NaN where the kernel must overwrite, between
guard rows of a sentinel.  Each figure is printed on a "norm bwd parity" line before it is asserted (profiles/norm_bwd_parity.txt holds one
run's lines)."""
import pytest
import torch

from difashion_amd import _lib
from tests import gpu_util as gu
from tests import helpers_norm as hn
from tests import helpers_norm_bwd as hb
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

G = hn.G
EPS = 1e-5


def _say(*parts):
    print("norm bwd parity", *parts)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _guarded(rows, cols, pre):
    """a bf16 [rows + 2][cols] device buffer: sentinel rows around `pre` (accumulate) or NaN (overwrite) -> (buffer, the view to hand over)"""
    buf = torch.full((rows + 2, cols), hb.SENTINEL, dtype=torch.bfloat16, device=DEV)
    buf[1:-1] = float("nan") if pre is None else pre.reshape(rows, cols).to(DEV)
    return buf, buf[1:-1]


def _unguard(buf, what):
    """the guards are untouched and no NaN survives -> the inner rows on the CPU"""
    b = buf.cpu()
    assert bool((b[0] == hb.SENTINEL).all()) and bool((b[-1] == hb.SENTINEL).all()), f"{what}: a guard row was written"
    assert not bool(torch.isnan(b[1:-1].float()).any()), f"{what}: NaN left in the gradient"
    return b[1:-1]


def _gn_bwd(x, dy, gamma, beta, stats, silu, C0, C1, acc0, acc1, pre, dg0=0.0, db0=0.0):
    """dfh_groupnorm_bwd -> (dx bf16 [B][HW][C] on the CPU, dgamma, dbeta fp32 [C], partial fp32 [B][G][chunks][2])"""
    B, HW, Cc = x.shape
    s0, s1 = _dev(x[..., :C0]), (_dev(x[..., C0:]) if C1 else None)
    b0, v0 = _guarded(B * HW, C0, pre[..., :C0] if acc0 else None)
    b1, v1 = _guarded(B * HW, C1, pre[..., C0:] if acc1 else None) if C1 else (None, None)
    keep = (_dev(dy), _dev(gamma), _dev(beta), _dev(stats))
    dg, db = torch.full((Cc,), dg0, device=DEV), torch.full((Cc,), db0, device=DEV)
    part = torch.full((B * 64 * G * 2,), float("nan"), device=DEV)
    _lib.call("dfh_groupnorm_bwd", _lib.ptr(s0), C0, _lib.ptr(s1), C1, _lib.ptr(keep[0]), B, HW, G, _lib.ptr(keep[1]), _lib.ptr(keep[2]),
              _lib.ptr(keep[3]), silu, _lib.ptr(v0), acc0, _lib.ptr(v1), acc1, _lib.ptr(dg), _lib.ptr(db), _lib.ptr(part), gu.stream())
    torch.cuda.synchronize()
    dx = _unguard(b0, "dx0").view(B, HW, C0)
    if C1:
        dx = torch.cat([dx, _unguard(b1, "dx1").view(B, HW, C1)], dim=-1)
    chunks = hn.two_kernel_geometry(B, Cc, HW)[1]
    return dx, dg.cpu(), db.cpu(), part[:B * G * chunks * 2].view(B, G, chunks, 2).cpu()


def _want(ref_dx, pre, C0, acc0, acc1):
    """the fp64 value the buffers must hold: pre + dx on the sources that accumulate"""
    w = ref_dx.clone()
    if acc0:
        w[..., :C0] += pre[..., :C0].double()
    if acc1:
        w[..., C0:] += pre[..., C0:].double()
    return w


# ----------------------------------------------------------------------------- dfh_groupnorm_bwd
@pytest.mark.parametrize("case", hb.GN_CASES, ids=hn.case_id)
def test_groupnorm_backward_is_exact_on_exact_data(case):
    """Leg A, silu = 0, every call form."""
    B, C0, C1, HW = case
    Cc = C0 + C1
    o = hb.gn_exact_operands(B, Cc, HW)
    r = hb.gn_bwd64(o["x"], o["dy"], o["gamma"], o["beta"], o["stats"], 0)
    PL, chunks, ppc = hn.two_kernel_geometry(B, Cc, HW)
    tag = hn.case_id(case)
    _say("A gn", tag, f"PL={PL} chunks={chunks} pix_per_chunk={ppc} last_chunk={HW - (chunks - 1) * ppc} n={HW * (Cc // G)}")
    for acc0, acc1 in hb.call_forms(C1):
        dx, dg, db, part = _gn_bwd(o["x"], o["dy"], o["gamma"], o["beta"], o["stats"], 0, C0, C1, acc0, acc1, o["pre"], dg0=-2.0, db0=3.0)
        form = f"acc=({acc0},{acc1})"
        nb, ng = int((db.double() != r["dbeta"] + 3.0).sum()), int((dg.double() != r["dgamma"] - 2.0).sum())
        sums = part.double().sum(dim=2)
        n1, n2 = int((sums[..., 0] != r["s1"]).sum()), int((sums[..., 1] != r["s2"]).sum())
        _say("A gn", tag, form, f"dbeta differs in {nb} dgamma in {ng} of {Cc}; partial sums differ: s1 {n1} s2 {n2} of {B * G}")
        assert nb == 0 and ng == 0, "dbeta / dgamma are exact sums (on top of the 3.0 / -2.0 the buffers held)"
        assert bool(torch.isfinite(part).all()) and n1 == 0 and n2 == 0, "the chunk records sum exactly to the fp64 group sums"
        want = _want(r["dx"], o["pre"], C0, acc0, acc1)
        if case in hb.GN_POW2_CASES:
            nd = int((dx != want.to(torch.bfloat16)).sum())
            _say("A gn", tag, form, f"dx differs from bf16(fp64) in {nd} of {dx.numel()}")
            assert nd == 0
        else:
            worst = float(((dx.double() - want).abs() / hb.rounded_bound(want, r["slack"]).clamp_min(1e-300)).max())
            _say("A gn", tag, form, f"dx err / rounded bound {worst:.3f}")
            assert worst <= 1


@pytest.mark.parametrize("kind", hb.GN_KINDS)
@pytest.mark.parametrize("case", hb.GN_CASES, ids=hn.case_id)
def test_groupnorm_backward_on_badly_conditioned_data(case, kind):
    """Leg B, silu in (0, 1), every call form; statistics from fp64 rounded to fp32."""
    B, C0, C1, HW = case
    Cc = C0 + C1
    x = hb.gn_input(case, kind)
    gamma, beta = hn.affine(Cc)
    dy, pre = hb.randn_bf16((B, HW, Cc), 71), hb.randn_bf16((B, HW, Cc), 72)
    stats = hb.stats64_as_fp32(x, EPS)
    D = hb.gn_bwd_depth(B, Cc, HW)
    tag = f"{hn.case_id(case)} {kind}"
    for silu in (0, 1):
        ax, ag, ab = hb.gn_autograd64(x, dy, gamma, beta, EPS, silu)
        r = hb.gn_bwd64(x, dy, gamma, beta, stats, silu)
        _say("B gn", tag, f"silu={silu} D={D} fp64 at the handed statistics vs fp64 autograd: dx {hn.rel(r['dx'], ax):.1e} dgamma {hn.rel(r['dgamma'], ag):.1e} "
             f"dbeta {hn.rel(r['dbeta'], ab):.1e}")
        for acc0, acc1 in hb.call_forms(C1):
            dx, dg, db, _ = _gn_bwd(x, dy, gamma, beta, stats, silu, C0, C1, acc0, acc1, pre)
            form = f"silu={silu} acc=({acc0},{acc1})"
            want = _want(ax, pre, C0, acc0, acc1)
            figs = hn.output_figures(dx, want)
            rg, kg = hb.sum_ratio(dg, r["dgamma"], r["tg"], D)
            rb, kb = hb.sum_ratio(db, r["dbeta"], r["tb"], D)
            _say("B gn", tag, form, f"dx rel_l2 {figs[0]:.3e} yardstick {figs[1]:.3e} ratio {figs[0] / figs[1]:.2f} max_rel {figs[2]:.2e} finite {figs[3]}; "
                 f"dgamma err/bound {rg:.3f} (K {kg:.2f}) dbeta err/bound {rb:.3f} (K {kb:.2f})")
            ok = hn.output_ok(figs)
            if kind == "const":
                cf = hn.output_figures(hb.const_slices(dx, B, Cc), hb.const_slices(want, B, Cc))
                _say("B gn", tag, form, f"constant groups: dx rel_l2 {cf[0]:.3e} yardstick {cf[1]:.3e} ratio {cf[0] / cf[1]:.2f} max_rel {cf[2]:.2e} finite {cf[3]}")
                ok = ok and hn.output_ok(cf)
            assert ok, (tag, form, figs)
            assert rg <= 1 and rb <= 1, (tag, form, rg, rb)


# ----------------------------------------------------------------------------- dfh_layernorm_bwd
def _ln_bwd(x, dy, gamma, eps, accumulate, pre, dg0=0.0, db0=0.0):
    M, C = x.shape
    buf, view = _guarded(M, C, pre if accumulate else None)
    keep = (_dev(x), _dev(dy), _dev(gamma))
    dg, db = torch.full((C,), dg0, device=DEV), torch.full((C,), db0, device=DEV)
    _lib.call("dfh_layernorm_bwd", _lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(keep[2]), _lib.ptr(view), accumulate, _lib.ptr(dg), _lib.ptr(db), M, C,
              eps, gu.stream())
    torch.cuda.synchronize()
    return _unguard(buf, "dx"), dg.cpu(), db.cpu()


@pytest.mark.parametrize("M,C", hb.LN_CASES, ids=[f"{m}x{c}" for m, c in hb.LN_CASES])
def test_layernorm_backward_is_exact_on_exact_data(M, C):
    """Leg A, eps = 0: rows of +-a with a in 1, 2, 4, so mean = 0, the variance is a^2 and x^ = +-1 -- given that the device's rsqrtf
    returns exactly 1, 0.5, 0.25 for 1, 4, 16.  It does (profiles/norm_bwd_parity.txt: dgamma, which sums dy x^ over rows of every a, is
    bit-equal on every case, which it could not be with an rstd off by an ulp), so dgamma and the power-of-two dx are held bit-equal."""
    o = hb.ln_exact_operands(M, C)
    r = hb.ln_bwd64(o["x"], o["dy"], o["gamma"], 0.0)
    assert torch.equal(r["rstd"], 1.0 / o["a"].double())
    tag = f"{M}x{C} kernel<{hb.ln_instantiation(C)}>"
    for accumulate in (0, 1):
        dx, dg, db = _ln_bwd(o["x"], o["dy"], o["gamma"], 0.0, accumulate, o["pre"], dg0=-2.0, db0=3.0)
        nb, ng = int((db.double() != r["dbeta"] + 3.0).sum()), int((dg.double() != r["dgamma"] - 2.0).sum())
        _say("A ln", tag, f"accumulate={accumulate} dbeta differs in {nb} dgamma in {ng} of {C} (rsqrtf exact at 1, 4, 16: {ng == 0})")
        assert nb == 0 and ng == 0
        want = r["dx"] + o["pre"].double() if accumulate else r["dx"]
        if C in hb.LN_POW2_WIDTHS:
            nd = int((dx != want.to(torch.bfloat16)).sum())
            _say("A ln", tag, f"accumulate={accumulate} dx differs from bf16(fp64) in {nd} of {dx.numel()}")
            assert nd == 0
        else:
            worst = float(((dx.double() - want).abs() / hb.rounded_bound(want, r["slack"]).clamp_min(1e-300)).max())
            _say("A ln", tag, f"accumulate={accumulate} dx err / rounded bound {worst:.3f}")
            assert worst <= 1


@pytest.mark.parametrize("M,C", hb.LN_CASES, ids=[f"{m}x{c}" for m, c in hb.LN_CASES])
def test_layernorm_backward_on_badly_conditioned_rows(M, C):
    """Leg B, eps = 1e-5: rows at |mean| / std = 8, 32, 64 in turn and two constant rows (mean exact, x^ = 0, rstd = eps^-1/2,
    dx = rstd (gamma dy - mean(gamma dy)))."""
    o = hb.ln_offset_operands(M, C)
    r = hb.ln_bwd64(o["x"], o["dy"], o["gamma"], hb.LN_EPS)
    D = hb.ln_bwd_depth(M)
    tag = f"{M}x{C} kernel<{hb.ln_instantiation(C)}>"
    for accumulate in (0, 1):
        dx, dg, db = _ln_bwd(o["x"], o["dy"], o["gamma"], hb.LN_EPS, accumulate, o["pre"])
        want = r["dx"] + o["pre"].double() if accumulate else r["dx"]
        figs = hn.output_figures(dx, want)
        rg, kg = hb.sum_ratio(dg, r["dgamma"], r["tg"], D)
        rb, kb = hb.sum_ratio(db, r["dbeta"], r["tb"], D)
        _say("B ln", tag, f"accumulate={accumulate} D={D} dx rel_l2 {figs[0]:.3e} yardstick {figs[1]:.3e} ratio {figs[0] / figs[1]:.2f} max_rel {figs[2]:.2e} "
             f"finite {figs[3]}; dgamma err/bound {rg:.3f} (K {kg:.2f}) dbeta err/bound {rb:.3f} (K {kb:.2f})")
        ok = hn.output_ok(figs)
        if bool(o["const"].any()):
            cf = hn.output_figures(dx[o["const"]], want[o["const"]])
            _say("B ln", tag, f"accumulate={accumulate} constant rows: dx rel_l2 {cf[0]:.3e} yardstick {cf[1]:.3e} ratio {cf[0] / cf[1]:.2f} max_rel {cf[2]:.2e}")
            ok = ok and hn.output_ok(cf)
        assert ok, (tag, accumulate, figs)
        assert rg <= 1 and rb <= 1, (tag, accumulate, rg, rb)
