"""The pointwise and layout kernels of the training step (bwd_elementwise.hip) against fp64, op by op through the C ABI.  The activation
and GEGLU kernels sweep EVERY finite bf16 value (65 280 bit patterns, plus five so the length is ragged against the 256-thread block):
tails, subnormals, the zero of gelu' / silu', signed zeros.  The layout kernels move integers under power-of-two scales and are held
bit-equal.  Inputs, references and bounds: tests/helpers_norm_bwd.py (K of the activation bound is set from torch's fp32 evaluation in
tests/test_norm_bwd_inputs_cpu.py).  Each figure is printed on a "pointwise parity" line before it is asserted
(profiles/norm_bwd_parity.txt holds one run's lines)."""
import pytest
import torch

from difashion_amd import _lib
from tests import gpu_util as gu
from tests import helpers_norm as hn
from tests import helpers_norm_bwd as hb
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

U = hn.U


def _say(*parts):
    print("pointwise parity", *parts)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _nan_bf16(n):
    return torch.full((n,), float("nan"), dtype=torch.bfloat16, device=DEV)


def _act_bound(ref64, K):
    return hb.half_ulp_bf16(ref64) + K * U * ref64.abs() + hb.BF16_TINY


# ----------------------------------------------------------------------------- dfh_act_fwd / dfh_act_bwd
@pytest.mark.parametrize("kind", [hb.ACT_SILU, hb.ACT_LEAKY, hb.ACT_TANH], ids=["silu", "leaky_relu", "tanh"])
def test_activation_forward_over_every_finite_bf16(kind):
    """leaky_relu is bit-equal to bf16(fp64); silu and tanh within half a bf16 ulp + K_FWD u |ref| + 2^-133."""
    x = hb.bf16_sweep()
    xd, y = _dev(x), _nan_bf16(x.numel())
    _lib.call("dfh_act_fwd", _lib.ptr(xd), _lib.ptr(y), x.numel(), kind, gu.stream())
    torch.cuda.synchronize()
    y = y.cpu()
    ref = hb.act_fwd64(kind, x)
    k, odd = hb.measured_k(y, ref)
    differ = int((y.double() != ref.to(torch.bfloat16).double()).sum())
    _say(f"act_fwd kind={kind} n={x.numel()} differs from bf16(fp64) in {differ}; measured K {k:.2f} (K_FWD {hb.K_FWD}); not comparable {odd}")
    assert not bool(torch.isnan(y.float()).any())
    if kind == hb.ACT_LEAKY:
        assert differ == 0
    assert odd == 0 and bool(hb.within(y, ref, _act_bound(ref, hb.K_FWD)).all())


@pytest.mark.parametrize("kind", [hb.ACT_SILU, hb.ACT_LEAKY, hb.ACT_TANH], ids=["silu", "leaky_relu", "tanh"])
def test_activation_backward_over_every_finite_bf16(kind):
    """dpre = dy * scale * slope(ref) in the four operand forms (ref and dy each as bf16 or as fp32: the fp32 forms hold 0.75 x the sweep,
    which no bf16 holds, so a kernel that read the wrong operand is off by a quarter), scale in (1, 0.5, 1/3), dy cycling through five
    magnitudes.  Within half a bf16 ulp + K_BWD u |ref| + 2^-133 of fp64.  tanh takes its slope 1 - r^2 from the OUTPUT, |r| <= 1: beyond
    2^64 the square leaves fp32 and the kernel returns -+inf by the format's range, which is asserted as that."""
    sweep = hb.bf16_sweep()
    n = sweep.numel()
    dyb = hb.cycle_like(hb.DY_CYCLE, n)
    worst = 0.0
    for ref_f32 in (0, 1):
        for dy_f32 in (0, 1):
            r = sweep.float() * hb.F32_FORM if ref_f32 else sweep
            d = dyb.float() * hb.F32_FORM if dy_f32 else dyb
            rd, dd = _dev(r), _dev(d)
            for scale in hb.SCALES:
                out = _nan_bf16(n)
                _lib.call("dfh_act_bwd", _lib.ptr(None if ref_f32 else rd), _lib.ptr(rd if ref_f32 else None), _lib.ptr(None if dy_f32 else dd),
                          _lib.ptr(dd if dy_f32 else None), _lib.ptr(out), n, kind, scale, gu.stream())
                torch.cuda.synchronize()
                out = out.cpu()
                ref = hb.act_bwd_ref64(kind, r, d, scale)
                inside = r.double().abs() < 2.0 ** 64 if kind == hb.ACT_TANH else torch.ones(n, dtype=torch.bool)
                k, odd = hb.measured_k(out, ref, inside)
                worst = max(worst, k)
                _say(f"act_bwd kind={kind} ref={'f32' if ref_f32 else 'bf16'} dy={'f32' if dy_f32 else 'bf16'} scale={scale:.4f} measured K {k:.2f} "
                     f"(K_BWD {hb.K_BWD}); not comparable {odd}")
                assert not bool(torch.isnan(out.float()).any())
                assert odd == 0 and bool(hb.within(out, ref, _act_bound(ref, hb.K_BWD))[inside].all())
                if kind == hb.ACT_TANH:
                    assert bool((out.double()[~inside] == -torch.sign(d.double()[~inside]) * float("inf")).all())
                    if not ref_f32:
                        assert bool((out.float()[sweep.float().abs() == 1.0] == 0).all()), "tanh: r = +-1 gives 0"
                if kind == hb.ACT_LEAKY and not ref_f32:
                    z = sweep.float() == 0
                    assert int(z.sum()) >= 2 and torch.equal(out[z], (d.double()[z] * hn.f32(scale) * hb.LEAKY_SLOPE).to(torch.bfloat16)), "r = +-0: slope 0.01"
    _say(f"act_bwd kind={kind} worst measured K over the twelve forms {worst:.2f}")


# ----------------------------------------------------------------------------- dfh_geglu_fwd / dfh_geglu_bwd
def _geglu(v, g, d, N2):
    """the packed layout (16 values then 16 gates per 32 columns) -> (y, dv, dg) bf16 [M][N2 / 2] on the CPU, standard column order"""
    M = v.shape[0]
    vcol, gcol = hb.geglu_packed_cols(N2)
    pre = torch.empty((M, N2), dtype=torch.bfloat16)
    pre[:, vcol], pre[:, gcol] = v, g
    pred, dd = _dev(pre), _dev(d)
    y = torch.full((M, N2 // 2), float("nan"), dtype=torch.bfloat16, device=DEV)
    dpre = torch.full((M, N2), float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.call("dfh_geglu_fwd", _lib.ptr(pred), _lib.ptr(y), M, N2, gu.stream())
    _lib.call("dfh_geglu_bwd", _lib.ptr(pred), _lib.ptr(dd), _lib.ptr(dpre), M, N2, gu.stream())
    torch.cuda.synchronize()
    dpre = dpre.cpu()
    return y.cpu(), dpre[:, vcol], dpre[:, gcol]


@pytest.mark.parametrize("N2", hb.GEGLU_WIDTHS)
def test_geglu_over_every_finite_bf16_gate(N2):
    """Gate = the sweep, value cycling through (1, -0.375, 96, 2^-20), dy through five integers; M rows so that the thread count is ragged
    against the block.  Forward within half an ulp + 4 u |ref| + 1e-8 |v| max(1, |g|); dv + 1e-7 |d| min(|g|, 6); dg + 2e-7 |d v|."""
    v, g, d = hb.geglu_operands(N2)
    M = v.shape[0]
    assert (M * (N2 // 16)) % 256 != 0
    y, dv, dg = _geglu(v, g, d, N2)
    ry = v.double() * hb.gelu64(g)
    rdv, rdg = d.double() * hb.gelu64(g), d.double() * v.double() * hb.dgelu64(g)
    wy = hb.worst_over_bound(y, ry, hb.geglu_fwd_bound(v, g, ry))
    wv = hb.worst_over_bound(dv, rdv, hb.geglu_dv_bound(d, g, rdv))
    wg = hb.worst_over_bound(dg, rdg, hb.geglu_dg_bound(d, v, rdg))
    nan = int(torch.isnan(y.float()).sum() + torch.isnan(dv.float()).sum() + torch.isnan(dg.float()).sum())
    _say(f"geglu N2={N2} M={M} threads={M * (N2 // 16)} worst err/bound: fwd {wy:.3f} dv {wv:.3f} dg {wg:.3f}; NaN {nan}")
    assert nan == 0 and wy <= 1 and wv <= 1 and wg <= 1


def test_geglu_forward_and_backward_agree():
    """With v = 1 and dy = 1 the forward's y and the backward's dv are both gelu(g): they agree within the two half ulps and the sum of
    the two absolute terms."""
    N2 = 32
    _, g, _ = hb.geglu_operands(N2)
    one = torch.ones_like(g)
    y, dv, _ = _geglu(one, g, one, N2)
    ref = hb.gelu64(g)
    bound = hb.geglu_fwd_bound(one, g, ref) + hb.geglu_dv_bound(one, g, ref)
    diff = (y.double() - dv.double()).abs()
    ok = (y.double() == dv.double()) | (diff <= bound)
    ratio = torch.where(y.double() == dv.double(), torch.zeros_like(diff), diff / bound)
    _say(f"geglu fwd vs bwd: y != dv in {int((y != dv).sum())} of {g.numel()}, worst |y - dv| / bound {float(ratio.nan_to_num(nan=float('inf')).max()):.3f}")
    assert bool(ok.all())


# ----------------------------------------------------------------------------- the exact layout kernels
def _ints(lo, hi, shape, seed, dtype=torch.float32):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def test_add_bf16_both_modes_and_the_length_it_refuses():
    n = 8 * 333                                        # 333 vectors: ragged against the block
    src, dst0 = _ints(-64, 64, (n,), 81, torch.bfloat16), _ints(-64, 64, (n,), 82, torch.bfloat16)
    for accumulate in (0, 1):
        dst, s = _dev(dst0).clone(), _dev(src)
        _lib.call("dfh_add_bf16", _lib.ptr(dst), _lib.ptr(s), n, accumulate, gu.stream())
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu(), (dst0.float() + src.float()).to(torch.bfloat16) if accumulate else src)
    with pytest.raises(_lib.DfhError, match="length must be a multiple of 8"):
        _lib.call("dfh_add_bf16", _lib.ptr(dst), _lib.ptr(s), n - 3, 0, gu.stream())


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_nhwc_to_nchw_f32_drops_the_padding_channels(scale, accumulate):
    B, HW, Cp, C = 2, 37, 8, 5
    src, dst0 = _ints(-100, 100, (B, HW, Cp), 83, torch.bfloat16), _ints(-9, 9, (B, C, HW), 84)
    dst = _dev(dst0).clone() if accumulate else torch.full((B, C, HW), float("nan"), device=DEV)
    s = _dev(src)
    _lib.call("dfh_nhwc_to_nchw_f32", _lib.ptr(s), _lib.ptr(dst), B, HW, Cp, C, scale, accumulate, gu.stream())
    torch.cuda.synchronize()
    want = scale * src[..., :C].float().permute(0, 2, 1)
    assert torch.equal(dst.cpu(), dst0 + want if accumulate else want)


def test_assemble_bwd_masks_the_rows_without_a_mutual_condition():
    rows, CL = 7, 48
    dx = _ints(-50, 50, (rows, 2 * CL), 85)
    real = torch.tensor([1, 0, 1, 1, 0, 0, 1], dtype=torch.uint8)
    out = torch.full((rows, CL), float("nan"), device=DEV)
    keep = (_dev(dx), _dev(real))
    _lib.call("dfh_assemble_bwd", _lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(out), rows, CL, 0.5, gu.stream())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.where(real[:, None] != 0, 0.5 * dx[:, :CL], torch.zeros(rows, CL)))


@pytest.mark.parametrize("geglu", [0, 1])
def test_unpack_vector_adds_the_packed_rows(geglu):
    N, off = 320, 24                                   # more than one block
    g, grad0 = _ints(-1000, 1000, (off + N + 8,), 86), _ints(-9, 9, (N,), 87)
    grad, gd = _dev(grad0).clone(), _dev(g)
    _lib.call("dfh_unpack_vector", _lib.ptr(gd), _lib.ptr(grad), N, off, geglu, gu.stream())
    torch.cuda.synchronize()
    rows = torch.tensor([hb.geglu_row_of(i, N) if geglu else i for i in range(N)])
    assert torch.equal(grad.cpu(), grad0 + g[off + rows])


@pytest.mark.parametrize("rows,L", [(4, 64), (3, 50)])
def test_mse_bwd_with_and_without_weights_and_device_scale(rows, L):
    """d pred = w[row] * loss_scale * scale_dev * 2 / (rows L) * (pred - target) on integer data: bit-equal to fp64 when rows * L and the
    weights are powers of two, else within 4 u (the weight times the scale, the division and the last product round)."""
    pow2 = (rows * L) & (rows * L - 1) == 0
    pred, target = _ints(-40, 40, (rows, L), 88), _ints(-40, 40, (rows, L), 89)
    w = torch.tensor([0.5, 2.0, 1.0, 4.0][:rows]) if pow2 else torch.tensor([0.3, 1.7, 1.1][:rows])
    sdev = torch.tensor([0.5])
    keep = (_dev(pred), _dev(target), _dev(w), _dev(sdev))
    for use_w in (0, 1):
        for use_s in (0, 1):
            out = torch.full((rows, L), float("nan"), device=DEV)
            _lib.call("dfh_mse_bwd", _lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(keep[2] if use_w else None), _lib.ptr(out), rows, L, 4.0,
                      _lib.ptr(keep[3] if use_s else None), gu.stream())
            torch.cuda.synchronize()
            ww = (w.double() if use_w else torch.ones(rows, dtype=torch.float64)) * 4.0 * (0.5 if use_s else 1.0) * 2.0 / (rows * L)
            ref = ww[:, None] * (pred.double() - target.double())
            err = float(((out.cpu().double() - ref).abs() / (U * ref.abs()).clamp_min(1e-300)).max())
            _say(f"mse_bwd rows={rows} L={L} w={use_w} scale_dev={use_s} worst err {err:.2f} u")
            assert err == 0 if pow2 else err <= 4
