"""-m gpu: op-level parity of the HIP kernels, called through the C ABI, against torch fp32
references on identical (bf16-rounded) operands.  Tolerances are stated per test."""
import ctypes as C
import math

import os

import pytest
import torch
import torch.nn.functional as F

from difashion_amd import _lib
from oracle import glue_ref, sched_ref, unet_ref
from tests import gpu_util as gu
from tests import helpers_norm as hn
from tests.gpu_util import DEV, bf, rnd

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- GEMM (linear / 1x1 conv)
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 9, 10, 21])  # every tile / pipeline-depth variant of gemm.hip; 6 / 9 = gemm_wide.hip (256x160 / 256x128); 10 = eight-wave 128x160; 21 = 256x320 eight-wave, 64-deep k-steps
@pytest.mark.parametrize("order", [-1, 2, 3])     # tile enumeration: heuristic / n-major / m-major (placement never changes results)
@pytest.mark.parametrize("M,N,K", [(300, 320, 320), (128, 160, 64), (77 * 3, 64, 768), (16, 1280, 200), (4, 256, 2048)])
def test_gemm_plain(tile, order, M, N, K):
    a, w = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=0.05))
    bias = rnd(N, seed=3)
    res = bf(rnd(M, N, seed=4))
    out = gu.gemm(M=M, N=N, W=w, ldw=K, a0=a, a0_c=K, bias=bias, resid=res, force_tile=tile, force_order=order)
    ref = a.float() @ w.float().T + bias + res.float()
    gu.assert_close_bf16(out, ref, f"gemm {M}x{N}x{K} tile{tile} order{order}")


@pytest.mark.parametrize("split", [2, 5])
def test_gemm_splitk_matches_single_pass(split):
    M, N, K = 200, 320, 1280
    a, w = bf(rnd(M, K, seed=5)), bf(rnd(N, K, seed=6, scale=0.05))
    bias = rnd(N, seed=7)
    ref = a.float() @ w.float().T + bias
    out = gu.gemm(M=M, N=N, W=w, ldw=K, a0=a, a0_c=K, bias=bias, force_split=split)
    gu.assert_close_bf16(out, ref, f"split{split}")
    out32 = gu.gemm(M=M, N=N, W=w, ldw=K, a0=a, a0_c=K, bias=bias, force_split=split, out_mode=2)
    assert gu.rel_err(out32, ref) < 2e-5      # fp32 output: only accumulation order differs


@pytest.mark.parametrize("M,N,C0,C1,tile,split", [
    (256, 160, 192, 96, 0, 0),        # ragged segment lengths: the general k-step iterator
    (300, 320, 256, 64, 10, 0),       # whole 64-channel slices: the lean k-loop re-bases its A pointers where segment 0 ends
    (300, 320, 256, 64, 21, 0),       # ... on the 256 x 320 tile ([GEGLU output | h2] of the folded ff.net.2 . proj_out linear)
    (200, 160, 128, 320, 10, 3),      # split-K: the second and third slice START inside segment 1
    (520, 640, 1280, 320, 0, 0),
])
def test_gemm_two_sources_is_channel_concat(M, N, C0, C1, tile, split):
    """K segments = torch.cat([h, skip], dim=1) feeding a 1x1 conv (up-path resnet shortcut) / a folded pair of linears."""
    a0, a1 = bf(rnd(M, C0, seed=8)), bf(rnd(M, C1, seed=9))
    w = bf(rnd(N, C0 + C1, seed=10, scale=0.05))
    bias, res = rnd(N, seed=11), bf(rnd(M, N, seed=12))
    out = gu.gemm(M=M, N=N, W=w, ldw=C0 + C1, a0=a0, a0_c=C0, a1=a1, a1_c=C1, bias=bias, resid=res, force_tile=tile, force_split=split)
    ref = torch.cat([a0, a1], 1).float() @ w.float().T + bias + res.float()
    gu.assert_close_bf16(out, ref, "concat")


@pytest.mark.parametrize("tile", [0, 6, 9, 21])
@pytest.mark.parametrize("act,fn", [(1, F.silu), (2, lambda x: F.leaky_relu(x, 0.01)), (3, torch.tanh)])
def test_gemm_activations_and_rowvec(act, fn, tile):
    B, rows, N, K = 3, 40, 128, 96
    M = B * rows
    a, w = bf(rnd(M, K, seed=11)), bf(rnd(N, K, seed=12, scale=0.1))
    bias = rnd(N, seed=13)
    rv = rnd(B, 3 * N, seed=14)
    out = gu.gemm(M=M, N=N, W=w, ldw=K, a0=a, a0_c=K, bias=bias, rowvec=rv, rv_ld=3 * N, rv_off=N, rows_per_b=rows, act=act, force_tile=tile)
    ref = fn(a.float() @ w.float().T + bias + rv[:, N:2 * N].repeat_interleave(rows, 0))
    gu.assert_close_bf16(out, ref, f"act{act}")


@pytest.mark.parametrize("M,C,tile", [(200, 64, 0), (300, 40, 0), (300, 40, 6), (520, 80, 6), (300, 64, 9), (700, 80, 9), (256, 16, 9),
                                         (300, 64, 23), (700, 96, 23), (520, 320, 23)])     # 23 = 256 x 256 eight-wave GEGLU tile
def test_gemm_geglu_epilogue(M, C, tile):
    """FeedForward GEGLU: proj -> chunk(2) -> a * gelu(gate); weights/bias interleaved by dfh_pack_*."""
    x = bf(rnd(M, C, seed=15))
    w = rnd(8 * C, C, seed=16, scale=0.1)
    b = rnd(8 * C, seed=17, scale=0.5)
    wp = torch.empty((8 * C, C), dtype=torch.bfloat16, device=DEV)
    bp = torch.empty(8 * C, dtype=torch.float32, device=DEV)
    _lib.call("dfh_pack_matrix", _lib.ptr(w), _lib.ptr(wp), 8 * C, C, C, 0, 0, 1, gu.stream())
    _lib.call("dfh_pack_vector", _lib.ptr(b), _lib.ptr(bp), 8 * C, 0, 1, 0, gu.stream())
    out = gu.gemm(M=M, N=8 * C, W=wp, ldw=C, a0=x, a0_c=C, bias=bp, act=4, force_tile=tile)
    h = x.float() @ bf(w).float().T + b
    a, gate = h.chunk(2, -1)
    gu.assert_close_bf16(out, a * F.gelu(gate), "geglu")


@pytest.mark.parametrize("M,C,ptile,resid", [(700, 320, 10, True), (700, 320, 6, True), (700, 320, 21, True), (1000, 640, 10, False), (300, 128, 5, True),
                                              (520, 64, 3, False), (4096, 1280, 0, True)])
def test_layernorm_folded_into_the_surrounding_gemms(M, C, ptile, resid):
    """dfh_gemm_ln / dfh_ln_fold: the producer GEMM (proj_in / to_out + residual) leaves per-row (mean, centred sum of squares) records
    of its bf16 output per column tile; the consumers (q|k, V^T, GEGLU input projection) run on the RAW rows with gamma folded into
    their weights and fix the rows up in the epilogue.  Checked: the records against torch on the producer's own output; every
    consumer against fp32 LayerNorm -> linear of the same bf16 operands (the tolerance of the unfolded kernels) and against the
    unfolded kernel path (dfh_layernorm + dfh_gemm) -- rows with a large common offset included (mean >> std: the case where a
    naive sum / sum-of-squares variance would cancel)."""
    x = bf(rnd(M, C, seed=51) + 3.0)
    w1 = bf(rnd(C, C, seed=52, scale=0.05))
    b1 = rnd(C, seed=53)
    res = bf(rnd(M, C, seed=54) * 2.0 + torch.linspace(-20, 20, M, device=DEV)[:, None]) if resid else None
    # --- producer
    d = gu.gemm_desc(M=M, N=C, W=w1, ldw=C, a0=x, a0_c=C, bias=b1, resid=res, force_tile=ptile)
    h = d.keep_out
    st = torch.full((8 * M * 2 + 16,), float("nan"), dtype=torch.float32, device=DEV)
    import ctypes
    bn = ctypes.c_int(0)
    _lib.call("dfh_gemm_ln", ctypes.byref(d), _lib.ptr(st), ctypes.byref(bn), None, 0, 0, 0.0, None, gu.stream())
    torch.cuda.synchronize()
    bn = bn.value
    assert bn in (64, 128, 160, 320) and C % bn == 0, bn
    parts = C // bn
    href = x.float() @ w1.float().T + b1 + (res.float() if resid else 0)
    gu.assert_close_bf16(h, href, "producer output")
    rec = st[:parts * M * 2].view(parts, M, 2)
    hp = h.float().view(M, parts, bn).transpose(0, 1)                         # [parts][M][bn]
    mean_t = hp.mean(-1)
    m2_t = ((hp - mean_t[..., None]) ** 2).sum(-1)
    torch.testing.assert_close(rec[..., 0], mean_t, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rec[..., 1], m2_t, rtol=1e-4, atol=1e-4)
    # --- consumers
    gamma, beta = 1.0 + 0.2 * rnd(C, seed=55), 0.3 * rnd(C, seed=56)
    ln = F.layer_norm(h.float(), (C,), gamma, beta, 1e-5)
    y_ln = torch.empty_like(h)
    _lib.call("dfh_layernorm", _lib.ptr(h), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(y_ln), M, C, 1e-5, gu.stream())

    def fold(w, bias):
        N = w.shape[0]
        wf = torch.empty_like(w)
        s, b = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
        _lib.call("dfh_ln_fold", _lib.ptr(w), C, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(bias), _lib.ptr(wf), _lib.ptr(s), _lib.ptr(b), N, C,
                  gu.stream())
        return wf, s, b

    def consume(wf, s, b, **kw):
        dd = gu.gemm_desc(M=M, W=wf, ldw=C, a0=h, a0_c=C, bias=b, **kw)
        _lib.call("dfh_gemm_ln", ctypes.byref(dd), None, None, _lib.ptr(st), parts, bn, 1e-5, _lib.ptr(s), gu.stream())
        torch.cuda.synchronize()
        return dd.keep_out

    # q|k: N = 2C, plain bf16 rows
    wq = bf(rnd(2 * C, C, seed=57, scale=0.05))
    wf, s, b = fold(wq, None)
    torch.testing.assert_close(wf.float(), bf(wq.float() * gamma).float(), rtol=0, atol=0)
    torch.testing.assert_close(s, wf.float().sum(1), rtol=1e-5, atol=1e-5)
    got = consume(wf, s, b, N=2 * C)
    gu.assert_close_bf16(got, ln @ wq.float().T, "folded q|k")
    plain = gu.gemm(M=M, N=2 * C, W=wq, ldw=C, a0=y_ln, a0_c=C)
    assert gu.rel_err(got, plain) < 8e-3
    # V^T: transposed per batch of rows
    if M % 4 == 0:
        rows = M // 4
        wv = bf(rnd(C, C, seed=58, scale=0.05))
        wf, s, b = fold(wv, None)
        out = torch.zeros((4, C, rows), dtype=torch.bfloat16, device=DEV)
        consume(wf, s, b, N=C, out=out, ld_out=rows, out_mode=1, rows_per_b=rows)
        gu.assert_close_bf16(out, (ln @ wv.float().T).view(4, rows, C).transpose(1, 2), "folded V^T")
    # GEGLU input projection: packed (interleaved) rows + bias
    wg, bg = rnd(8 * C, C, seed=59, scale=0.05), rnd(8 * C, seed=60, scale=0.5)
    wp = torch.empty((8 * C, C), dtype=torch.bfloat16, device=DEV)
    bp = torch.empty(8 * C, dtype=torch.float32, device=DEV)
    _lib.call("dfh_pack_matrix", _lib.ptr(wg), _lib.ptr(wp), 8 * C, C, C, 0, 0, 1, gu.stream())
    _lib.call("dfh_pack_vector", _lib.ptr(bg), _lib.ptr(bp), 8 * C, 0, 1, 0, gu.stream())
    wf, s, b = fold(wp, bp)
    got = consume(wf, s, b, N=8 * C, act=4)
    hh = ln @ bf(wg).float().T + bg
    av, gate = hh.chunk(2, -1)
    gu.assert_close_bf16(got, av * F.gelu(gate), "folded GEGLU")
    if (8 * C) % 256 == 0:                                   # the 256 x 256 eight-wave GEGLU tile implements the fix-up too
        got23 = consume(wf, s, b, N=8 * C, act=4, force_tile=23)
        gu.assert_close_bf16(got23, av * F.gelu(gate), "folded GEGLU, 256 x 256 tile")


def test_gemm_transposed_outputs():
    """OUT_BF16_T feeds attention's V^T (ragged 77 keys padded to 80); OUT_F32_T is conv_out's NCHW."""
    B, T, N, K = 3, 77, 64, 128
    a, w = bf(rnd(B * T, K, seed=18)), bf(rnd(N, K, seed=19, scale=0.1))
    out = torch.zeros((B, N, 80), dtype=torch.bfloat16, device=DEV)
    gu.gemm(M=B * T, N=N, W=w, ldw=K, a0=a, a0_c=K, out=out, ld_out=80, out_mode=1, rows_per_b=T)
    ref = (a.float() @ w.float().T).view(B, T, N).transpose(1, 2)
    gu.assert_close_bf16(out[:, :, :T], ref, "bf16_T")
    assert float(out[:, :, T:].abs().max()) == 0.0
    out32 = torch.zeros((B, N, T), dtype=torch.float32, device=DEV)
    gu.gemm(M=B * T, N=N, W=w, ldw=K, a0=a, a0_c=K, out=out32, ld_out=T, out_mode=3, rows_per_b=T)
    assert gu.rel_err(out32, ref) < 2e-5


@pytest.mark.parametrize("B,rows,N,K,tile", [(3, 256, 160, 128, 0), (2, 1024, 320, 320, 10), (5, 64, 64, 64, 0), (2, 136, 96, 64, 4)])
def test_gemm_transposed_output_staged_through_lds(B, rows, N, K, tile):
    """V^T for the self-attention: tiles that lie inside one batch element leave as 16-byte pieces of the [channel][pixel] rows
    (staged transposed through LDS); tiles that straddle two batch elements (rows = 64 < the 128-row tile; rows = 136) take the
    element-wise path.  Row pitch larger than the row count (the walk pads to 8 keys)."""
    a, w = bf(rnd(B * rows, K, seed=91)), bf(rnd(N, K, seed=92, scale=0.1))
    ld = rows + 8
    out = torch.zeros((B, N, ld), dtype=torch.bfloat16, device=DEV)
    gu.gemm(M=B * rows, N=N, W=w, ldw=K, a0=a, a0_c=K, out=out, ld_out=ld, out_mode=1, rows_per_b=rows, force_tile=tile)
    ref = (a.float() @ w.float().T).view(B, rows, N).transpose(1, 2)
    gu.assert_close_bf16(out[:, :, :rows], ref, "bf16_T staged")
    assert float(out[:, :, rows:].abs().max()) == 0.0


@pytest.mark.parametrize("B,rows,C", [(2, 1024, 320), (3, 256, 160), (2, 136, 128), (5, 64, 256)])
def test_gemm_second_transposed_destination(B, rows, C):
    """dfh_gemm_out2: q | k (columns 0 .. 2C, row-major) and V^T (columns 2C .. 3C, transposed per batch element) from ONE launch over
    the shared rows -- against the two separate launches (bit for bit: same products, same order) and the fp32 reference; batch
    elements smaller than / not a multiple of the row tile (the element-wise transposed path)."""
    import ctypes
    M, K = B * rows, C
    a, w = bf(rnd(M, K, seed=95)), bf(rnd(3 * C, K, seed=96, scale=0.08))
    ld = rows + 8
    qk = torch.zeros((M, 2 * C), dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros((B, C, ld), dtype=torch.bfloat16, device=DEV)
    d = gu.gemm_desc(M=M, N=3 * C, W=w, ldw=K, a0=a, a0_c=K, out=qk, ld_out=2 * C, rows_per_b=rows)
    _lib.call("dfh_gemm_out2", ctypes.byref(d), _lib.ptr(vt), ld, 2 * C, gu.stream())
    torch.cuda.synchronize()
    ref = a.float() @ w.float().T
    gu.assert_close_bf16(qk, ref[:, :2 * C], "q|k part")
    gu.assert_close_bf16(vt[:, :, :rows], ref[:, 2 * C:].view(B, rows, C).transpose(1, 2), "V^T part")
    assert float(vt[:, :, rows:].abs().max()) == 0.0
    qk2 = gu.gemm(M=M, N=2 * C, W=w[:2 * C].contiguous(), ldw=K, a0=a, a0_c=K)
    vt2 = torch.zeros_like(vt)
    gu.gemm(M=M, N=C, W=w[2 * C:].contiguous(), ldw=K, a0=a, a0_c=K, out=vt2, ld_out=ld, out_mode=1, rows_per_b=rows)
    assert torch.equal(qk, qk2) and torch.equal(vt, vt2)


# ----------------------------------------------------------------------------- conv3x3 as implicit GEMM
@pytest.mark.parametrize("cin,cout,H,stride,ups", [
    (64, 160, 16, 1, 0), (32, 64, 8, 1, 0), (320, 320, 16, 1, 0), (64, 64, 16, 2, 0), (64, 128, 8, 1, 1),
    (8, 64, 16, 1, 0),      # conv_in shape class (8 input channels, difashion.py:83-93)
    (64, 4, 16, 1, 0),      # conv_out shape class
    (128, 128, 2, 1, 0),    # 2x2 level of the tiny configs: every tap hits padding somewhere
])
@pytest.mark.parametrize("glds", [0, 1, 4, 6, 9, 10, 21])   # here: forced tile variant (0 = heuristic, 1 = 256x160 ring, 4 = 128x160 2-stage, 6 = wide)
def test_conv3x3(cin, cout, H, stride, ups, glds):
    B = 2
    x = bf(rnd(B, cin, H, H, seed=20))
    w = rnd(cout, cin, 3, 3, seed=21, scale=0.05)
    bias = rnd(cout, seed=22)
    Ho = H * 2 if ups else H // stride
    out = gu.gemm(M=B * Ho * Ho, N=cout, W=gu.pack_conv(w), ldw=9 * cin, conv_src=gu.nhwc(x), conv_c=cin, batch=B,
                  Hin=H, Win=H, stride=stride, upsample=ups, bias=bias, force_tile=glds)
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if ups else x.float()
    ref = F.conv2d(xin, bf(w).float(), bias, stride=stride, padding=1)
    gu.assert_close_bf16(gu.nchw(out.view(B, Ho, Ho, cout)), ref, f"conv {cin}->{cout}@{H} s{stride} u{ups}")


def _phase_weights_ref(wb):
    """Summed taps per output phase of conv3x3(upsample2x(x)): [4][O][4 * I] from the bf16-rounded OIHW weights, fp32 sums."""
    O, I = wb.shape[:2]
    grp = {0: ([0], [1, 2]), 1: ([0, 1], [2])}          # phase -> (taps on source offset 0, taps on source offset 1)
    out = torch.zeros(4, O, 4, I, device=wb.device)
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    for ky in grp[py][a]:
                        for kx in grp[px][b]:
                            out[py * 2 + px, :, a * 2 + b] += wb[:, :, ky, kx]
    return out.reshape(4, O, 4 * I)


@pytest.mark.parametrize("B,cin,cout,H,W", [(2, 64, 128, 8, 8), (3, 128, 160, 5, 7), (2, 320, 320, 16, 16), (16, 64, 64, 8, 8),
                                            (1, 72, 40, 4, 4), (2, 64, 96, 1, 1),
                                            (16, 64, 320, 32, 32)])      # 4 planes x 64 tiles: the 256 x 320 tile
def test_upsample_conv_as_four_phase_planes(B, cin, cout, H, W):
    """Upsample2D (nearest 2x, then conv3x3; diffusers, the up-block upsamplers) as four 2x2 convs over the source image with summed taps:
    the summed weights are the exact fp32 tap sums rounded once, and the launch equals the conv over the upsampled image computed with
    those same weights (exact up to accumulation order) -- and the reference conv with the original weights to bf16 weight rounding."""
    x = bf(rnd(B, cin, H, W, seed=26))
    w = rnd(cout, cin, 3, 3, seed=27, scale=0.05)
    bias = rnd(cout, seed=28)
    packed = gu.pack_conv(w)
    wp = torch.empty(4, cout, 4 * cin, dtype=torch.bfloat16, device=gu.DEV)
    _lib.call("dfh_ups_phase_fold", _lib.ptr(packed), 9 * cin, _lib.ptr(wp), cout, cin, gu.stream())
    ref_w = _phase_weights_ref(bf(w).float())
    assert torch.equal(wp, bf(ref_w)), "phase weights are the fp32 tap sums, rounded once"
    out = torch.empty(B, 2 * H, 2 * W, cout, dtype=torch.bfloat16, device=gu.DEV)
    z = gu.zero_page()
    _lib.call("dfh_conv_up2x", _lib.ptr(gu.nhwc(x)), B, H, W, cin, _lib.ptr(wp), cout, _lib.ptr(bias), _lib.ptr(out), _lib.ptr(z), gu.stream())
    # the same arithmetic in torch: each phase is a 2x2 conv of the (zero-padded) source with the rounded summed weights
    xp = F.pad(x.float(), (1, 1, 1, 1))
    ref = torch.empty(B, cout, 2 * H, 2 * W, device=gu.DEV)
    for py in (0, 1):
        for px in (0, 1):
            k = wp[py * 2 + px].float().view(cout, 2, 2, cin).permute(0, 3, 1, 2).contiguous()
            ref[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], k, bias)
    gu.assert_close_bf16(gu.nchw(out), ref, f"phase conv {cin}->{cout}@{H}x{W}")
    full = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), bf(w).float(), bias, padding=1)
    assert gu.rel_err(gu.nchw(out).float(), full) < 6e-3, "against the 3x3 conv over the upsampled image (summed weights rounded once more)"


@pytest.mark.parametrize("B,cin,cout,H,W,resid,temb", [(2, 64, 128, 8, 8, False, True), (3, 128, 160, 6, 10, True, False), (2, 320, 320, 16, 16, True, True),
                                                          (16, 64, 64, 8, 8, False, False), (1, 72, 40, 4, 4, True, True), (2, 64, 96, 2, 2, False, True),
                                                          (4, 256, 320, 8, 8, True, True),
                                                          (16, 64, 1280, 16, 16, True, True)])     # 16 planes x 16 tiles: the 256 x 320 tile
def test_conv3x3_winograd(B, cin, cout, H, W, resid, temb):
    """Winograd F(2x2, 3x3) conv (input transform, batched GEMM over the 16 transform-domain planes, output transform with bias /
    time-embedding row / residual) against F.conv2d on the same bf16 operands.  U, V and M are rounded to bf16, so the bound is looser than
    the direct kernel's (whose only error is the output rounding): rel L2 <= 1e-2 (measured 5e-3)."""
    x = bf(rnd(B, cin, H, W, seed=32))
    w = rnd(cout, cin, 3, 3, seed=33, scale=0.05)
    bias = rnd(cout, seed=34)
    rv = rnd(B, 3 * cout, seed=35) if temb else None
    res = bf(rnd(B, H, W, cout, seed=36)) if resid else None
    packed = gu.pack_conv(w)
    U = torch.empty(16, cout, cin, dtype=torch.bfloat16, device=gu.DEV)
    blocked = _lib.raw().dfh_wino_blocked(cout, cin)          # 16 x 64 blocks where the batched GEMM reads them (N % 160 == 0, C % 64 == 0)
    _lib.call("dfh_wino_weights", _lib.ptr(packed), 9 * cin, _lib.ptr(U), cout, cin, blocked, gu.stream())
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1.]], device=gu.DEV)
    Uref = torch.einsum("ij,ncjk,lk->ilnc", G, bf(w).float(), G).reshape(16, cout, cin)
    Urow = U.view(16, cout // 16, cin // 64, 16, 64).permute(0, 1, 3, 2, 4).reshape(16, cout, cin) if blocked else U
    assert torch.equal(Urow, bf(Uref)) or gu.rel_err(Urow.float(), Uref) < 3e-3, "U = G g G^T of the bf16 taps"
    nbytes = _lib.raw().dfh_conv3x3_wino_scratch_bytes(B, H, W, cin, cout)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=gu.DEV)
    out = torch.empty(B, H, W, cout, dtype=torch.bfloat16, device=gu.DEV)
    z = gu.zero_page()
    _lib.call("dfh_conv3x3_wino", _lib.ptr(gu.nhwc(x)), B, H, W, cin, _lib.ptr(U), blocked, cout, _lib.ptr(bias), _lib.ptr(rv) if temb else None,
              3 * cout if temb else 0, cout if temb else 0, _lib.ptr(res) if resid else None, _lib.ptr(out), _lib.ptr(scratch), nbytes,
              _lib.ptr(z), gu.stream())
    ref = F.conv2d(x.float(), bf(w).float(), bias, padding=1)
    if temb:
        ref = ref + rv[:, cout:2 * cout, None, None]
    if resid:
        ref = ref + gu.nchw(res).float()
    gu.assert_close_bf16(gu.nchw(out), ref, f"winograd conv {cin}->{cout}@{H}x{W}", rel=1e-2, max_rel=4e-2)


@pytest.mark.parametrize("B,C0,C1,H,W", [(2, 1280, 0, 16, 16), (3, 1280, 640, 8, 8), (2, 640, 0, 16, 16), (16, 1280, 1280, 8, 8), (2, 128, 128, 4, 6)])
def test_groupnorm_silu_fused_into_the_winograd_input_transform(B, C0, C1, H, W):
    """V = B^T silu(GroupNorm(concat(x0, x1))) B from one launch (gn_wino_input_kernel) against the two-launch path (dfh_groupnorm, then
    dfh_wino_input) and against torch: the statistics are summed in a different order, so single bf16 roundings of the normalised tensor may
    differ -- rel L2 <= 2e-3 between the two, and the unfused transform is exact on its input."""
    G, C = 32, C0 + C1
    assert _lib.raw().dfh_gn_wino_input_ok(C0, C1, G, H, W)
    x0 = bf(rnd(B, H, W, C0, seed=40)); x1 = bf(rnd(B, H, W, C1, seed=41, scale=2.0)) if C1 else None
    gamma = 1.0 + 0.1 * rnd(C, seed=42); beta = 0.1 * rnd(C, seed=43)
    mt = B * (H // 2) * (W // 2)
    Vf = torch.empty(16, mt, C, dtype=torch.bfloat16, device=gu.DEV)
    _lib.call("dfh_gn_wino_input", _lib.ptr(x0), C0, _lib.ptr(x1) if C1 else None, C1, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, G, _lib.ptr(Vf),
              B, H, W, gu.stream())
    xcat = torch.cat([x0, x1], dim=-1) if C1 else x0
    gref = bf(F.silu(F.group_norm(gu.nchw(xcat).float(), G, gamma, beta, 1e-5)))           # what the GroupNorm kernel writes
    Vu = torch.empty_like(Vf)
    _lib.call("dfh_wino_input", _lib.ptr(gu.nhwc(gref)), _lib.ptr(Vu), B, H, W, C, gu.stream())
    BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1.]], device=gu.DEV)
    patches = F.pad(gref.float(), (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)                 # [B][C][TH][TW][4][4]
    Vref = torch.einsum("ij,bcyxjk,lk->ilbyxc", BT, patches, BT).reshape(16, mt, C)
    assert torch.equal(Vu, bf(Vref)), "the input transform is exact in fp32 on bf16 inputs (sums of four)"
    assert gu.rel_err(Vf.float(), Vref) <= 2e-3


@pytest.mark.parametrize("B,C,H,W,temb", [(2, 1280, 16, 16, True), (16, 1280, 8, 8, True), (3, 640, 8, 8, False), (2, 128, 4, 6, True)])
def test_winograd_chain_rebuilds_the_tensor_between_two_convs(B, C, H, W, temb):
    """dfh_gn_wino_input_chain: V2 from conv1's transform-domain planes (output transform + bias + time-embedding row, GroupNorm + SiLU,
    input transform in one launch) against the materialised path (torch output transform rounded to bf16 -> dfh_gn_wino_input)."""
    G = 32
    mt = B * (H // 2) * (W // 2)
    Mp = bf(rnd(16, mt, C, seed=70))
    bias = rnd(C, seed=71)
    rv = rnd(B, 2 * C, seed=72) if temb else None
    gamma = 1.0 + 0.1 * rnd(C, seed=73); beta = 0.1 * rnd(C, seed=74)
    Vc = torch.empty(16, mt, C, dtype=torch.bfloat16, device=gu.DEV)
    _lib.call("dfh_gn_wino_input_chain", _lib.ptr(Mp), _lib.ptr(bias), _lib.ptr(rv) if temb else None, 2 * C if temb else 0, C if temb else 0, C,
              _lib.ptr(gamma), _lib.ptr(beta), 1e-5, G, _lib.ptr(Vc), B, H, W, gu.stream())
    AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1.]], device=gu.DEV)
    m = Mp.float().view(4, 4, B, H // 2, W // 2, C)
    y = torch.einsum("ij,jkbyxc,lk->byixlc", AT, m, AT).reshape(B, H, W, C) + bias          # [b][2 ty + i][2 tx + l][c]
    if temb:
        y = y + rv[:, C:2 * C][:, None, None, :]
    h1 = bf(y)
    Vm = torch.empty_like(Vc)
    _lib.call("dfh_gn_wino_input", _lib.ptr(h1), C, None, 0, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, G, _lib.ptr(Vm), B, H, W, gu.stream())
    assert gu.rel_err(Vc.float(), Vm.float()) <= 2e-3


@pytest.mark.parametrize("nb,M,N,K,tile", [(16, 1024, 1280, 1280, 0), (4, 300, 160, 64, 0), (3, 128, 128, 192, 5), (16, 256, 320, 320, 10)])
def test_gemm_batched_planes_in_one_launch(nb, M, N, K, tile):
    """grid.y planes of independent GEMMs (dfh_gemm_batched) equal nb separate launches bit for bit."""
    a = bf(rnd(nb, M, K, seed=29)); w = bf(rnd(nb, N, K, seed=30, scale=0.05)); bias = rnd(N, seed=31)
    out = torch.empty(nb, M, N, dtype=torch.bfloat16, device=gu.DEV)
    d = gu.gemm_desc(M=M, N=N, W=w, ldw=K, a0=a, a0_c=K, bias=bias, out=out, ld_out=N, force_tile=tile)
    _lib.call("dfh_gemm_batched", C.byref(d), nb, M * K, N * K, M * N, gu.stream())
    for z in range(nb):
        one = gu.gemm(M=M, N=N, W=w[z], ldw=K, a0=a[z], a0_c=K, bias=bias, force_tile=tile if tile else 10 if N % 160 == 0 else 5, force_split=1)
        ref = a[z].float() @ w[z].float().t() + bias
        gu.assert_close_bf16(out[z], ref, f"batched plane {z}")
        assert torch.equal(out[z], one.view(M, N)), f"plane {z} differs from its own launch"


@pytest.mark.parametrize("tile", [0, 1, 6, 10, 21])
@pytest.mark.parametrize("cin,H,W", [(64, 12, 20), (128, 5, 3), (192, 16, 1)])
def test_conv3x3_lean_tap_staging_on_non_square_inputs(cin, H, W, tile):
    """The lean tap staging (centre-pixel offset + 9-bit validity mask per staging piece) on inputs whose height and
    width differ, incl. one-pixel-wide images where most taps of every pixel are padding; 3 images so that tiles straddle
    image boundaries."""
    B, cout = 3, 96
    x = bf(rnd(B, cin, H, W, seed=23))
    w = rnd(cout, cin, 3, 3, seed=24, scale=0.05)
    bias = rnd(cout, seed=25)
    out = gu.gemm(M=B * H * W, N=cout, W=gu.pack_conv(w), ldw=9 * cin, conv_src=gu.nhwc(x), conv_c=cin, batch=B,
                  Hin=H, Win=W, stride=1, upsample=0, bias=bias, force_tile=tile)
    ref = F.conv2d(x.float(), bf(w).float(), bias, padding=1)
    gu.assert_close_bf16(gu.nchw(out.view(B, H, W, cout)), ref, f"conv {cin}->{cout}@{H}x{W} tile{tile}")


@pytest.mark.parametrize("kind,cin,cout,H,B,tile", [
    ("conv", 64, 320, 32, 2, 6),      # 3x3 conv on the wide kernel: 4 row tiles per image, cpg 10 (16 groups per column tile)
    ("conv", 32, 640, 16, 3, 6),      # one row tile per image, cpg 20
    ("conv", 64, 320, 32, 2, 21),     # the 256 x 320 tile: all 32 groups of a row tile in one workgroup
    ("conv", 32, 640, 16, 3, 21),
    ("linear", 320, 320, 32, 2, 6),   # proj_out shape class: linear + residual
    ("conv", 64, 640, 32, 2, 10),     # round 5: the eight-wave 128 x 160 tile (the 32x32-level producers): 128-row chunks, cpg 20
    ("conv", 32, 320, 16, 3, 10),     # ... two chunks per image, cpg 10
    ("linear", 640, 640, 32, 2, 10),  # ... the LEAN instantiation (plain segment) + residual
])
def test_gemm_writes_groupnorm_statistics_for_its_consumer(kind, cin, cout, H, B, tile):
    """The 256-row epilogues and (round 5) the staged epilogue of the eight-wave 128 x 160 tile write, per (image, group, row tile), the sum and the sum of squares of the bf16 outputs (dfh_gemm_gstat);
    dfh_groupnorm_pre normalises from them in ONE launch.  Checked: the partials against torch sums of the GEMM's own output, and
    the normalised tensor against plain dfh_groupnorm of that output (same statistics up to summation order) and against
    F.group_norm; a launch on a kernel that cannot produce them reports written = 0."""
    G, HW = 32, H * H
    M, cpg = B * HW, cout // 32
    bias = rnd(cout, seed=41)
    res = bf(rnd(M, cout, seed=42))
    gst = torch.full((B * G * (HW // 128) * 2,), float("nan"), dtype=torch.float32, device=DEV)      # room for 128-row chunks
    if kind == "conv":
        x = bf(rnd(B, cin, H, H, seed=43))
        w = rnd(cout, cin, 3, 3, seed=44, scale=0.05)
        temb = rnd(B, 2 * cout, seed=45)
        kw = dict(M=M, N=cout, W=gu.pack_conv(w), ldw=9 * cin, conv_src=gu.nhwc(x), conv_c=cin, batch=B, Hin=H, Win=H, bias=bias,
                  rowvec=temb, rv_ld=2 * cout, rv_off=cout, rows_per_b=HW)
    else:
        a = bf(rnd(M, cin, seed=43))
        w = bf(rnd(cout, cin, seed=44, scale=0.05))
        kw = dict(M=M, N=cout, W=w, ldw=cin, a0=a, a0_c=cin, bias=bias, resid=res)
    out, rows = gu.gemm(force_tile=tile, gstat=gst, gstat_cpg=cpg, gstat_hw=HW, **kw)
    assert rows == (128 if tile == 10 else 256), rows
    chunks = HW // rows
    y = out.float().view(B, chunks, rows, G, cpg)
    ref = torch.stack([y.sum(dim=(2, 4)), (y * y).sum(dim=(2, 4))], dim=-1).permute(0, 2, 1, 3)     # [B][G][chunks][2]
    got = gst[:B * G * chunks * 2].view(B, G, chunks, 2)
    assert torch.allclose(got, ref, rtol=2e-5, atol=1e-2), float((got - ref).abs().max())
    gamma, beta = rnd(cout, seed=46) + 1.0, rnd(cout, seed=47)
    o_pre = torch.empty(M, cout, dtype=torch.bfloat16, device=DEV)
    stats = torch.empty(B * G * 2, dtype=torch.float32, device=DEV)
    _lib.call("dfh_groupnorm_pre", _lib.ptr(out), cout, B, HW, G, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, 1, _lib.ptr(o_pre),
              _lib.ptr(gst), chunks, _lib.ptr(stats), gu.stream())
    o_two = torch.empty_like(o_pre)
    part = torch.empty(B * 64 * 64 * 2, dtype=torch.float32, device=DEV)
    _lib.call("dfh_groupnorm", _lib.ptr(out), cout, None, 0, B, HW, G, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, 1, _lib.ptr(o_two),
              _lib.ptr(part), gu.stream())
    torch.cuda.synchronize()
    assert float((o_pre.float() - o_two.float()).abs().max()) <= 2e-2       # one bf16 step at |y| ~ 2-4: summation order only
    xr = gu.nchw(out.float().view(B, H, H, cout))
    gref = F.silu(F.group_norm(xr, G, gamma, beta, 1e-5))
    gu.assert_close_bf16(gu.nchw(o_pre.view(B, H, H, cout)), gref, "groupnorm from producer statistics")
    mean = xr.view(B, G, -1).mean(-1)
    assert torch.allclose(stats.view(B, G, 2)[..., 0], mean, atol=1e-3)
    # rstd, which the backward pass trusts: the one-pass variance against fp64 of the GEMM's own output, within Higham's bound for the
    # epilogue's summation depth times kappa_g = 1 + mean^2 / var (tests/helpers_norm.py; tests/test_gpu_norm_stats.py leg B)
    rb = hn.conditioning_leg(stats.cpu(), out.cpu().view(B, HW, cout), 1e-5, True, hn.producer_depth(cout, HW, rows))
    print(f"groupnorm parity B gn_pre {kind} {cin}->{cout}@{HW} tile{tile} R_g {rb['R'][0]:.2f}..{rb['R'][1]:.2f} rstd_err {rb['rstd_err']:.2e} "
          f"var_err/bound {rb['var']:.3f} mean_err/bound {rb['mean']:.3f} K {rb['K']:.2f}")
    assert rb["var"] <= 1 and rb["mean"] <= 1, rb
    # bit-identical reruns (fixed summation orders), and a launch that runs on a kernel without the statistics epilogue must say so
    g1 = gst.clone()
    gu.gemm(force_tile=tile, gstat=gst, gstat_cpg=cpg, gstat_hw=HW, **kw)
    assert torch.equal(gst[:B * G * chunks * 2], g1[:B * G * chunks * 2])
    _, w2 = gu.gemm(force_tile=5, gstat=gst, gstat_cpg=cpg, gstat_hw=HW, **kw)      # the four-wave 128 x 128 tile
    assert not w2


@pytest.mark.parametrize("tile", [0, 6, 9, 21])
def test_conv3x3_with_fused_shortcut_and_temb(tile):
    """ResnetBlock2D tail: conv2(h) + conv_shortcut(cat(x, skip)) + biases, and conv1 + time embedding."""
    B, H, c0, c1, cout = 2, 8, 64, 32, 96
    h = bf(rnd(B, cout, H, H, seed=23))
    x0, x1 = bf(rnd(B, c0, H, H, seed=24)), bf(rnd(B, c1, H, H, seed=25))
    w2 = rnd(cout, cout, 3, 3, seed=26, scale=0.05)
    ws = rnd(cout, c0 + c1, 1, 1, seed=27, scale=0.1)
    b2, bs = rnd(cout, seed=28), rnd(cout, seed=29)
    K = 9 * cout + c0 + c1
    W = torch.empty((cout, K), dtype=torch.bfloat16, device=DEV)
    _lib.call("dfh_pack_conv3x3", _lib.ptr(w2), _lib.ptr(W), cout, cout, K, 0, gu.stream())
    _lib.call("dfh_pack_matrix", _lib.ptr(ws.reshape(cout, -1).contiguous()), _lib.ptr(W), cout, c0 + c1, K, 0, 9 * cout, 0, gu.stream())
    bias = torch.empty(cout, device=DEV)
    _lib.call("dfh_pack_vector", _lib.ptr(b2), _lib.ptr(bias), cout, 0, 0, 0, gu.stream())
    _lib.call("dfh_pack_vector", _lib.ptr(bs), _lib.ptr(bias), cout, 0, 0, 1, gu.stream())
    M = B * H * H
    out = gu.gemm(M=M, N=cout, W=W, ldw=K, conv_src=gu.nhwc(h), conv_c=cout, batch=B, Hin=H, Win=H,
                  a0=gu.nhwc(x0).view(M, c0), a0_c=c0, a1=gu.nhwc(x1).view(M, c1), a1_c=c1, bias=bias, force_tile=tile)
    ref = F.conv2d(h.float(), bf(w2).float(), b2, padding=1) + F.conv2d(torch.cat([x0, x1], 1).float(), bf(ws).float(), bs)
    gu.assert_close_bf16(gu.nchw(out.view(B, H, H, cout)), ref, "conv2+shortcut")
    temb = rnd(B, 2 * cout, seed=30)
    out = gu.gemm(M=M, N=cout, W=gu.pack_conv(w2), ldw=9 * cout, conv_src=gu.nhwc(h), conv_c=cout, batch=B, Hin=H, Win=H,
                  bias=b2, rowvec=temb, rv_ld=2 * cout, rv_off=cout, rows_per_b=H * H, force_tile=tile)
    ref = F.conv2d(h.float(), bf(w2).float(), b2, padding=1) + temb[:, cout:, None, None]
    gu.assert_close_bf16(gu.nchw(out.view(B, H, H, cout)), ref, "conv1+temb")


# ----------------------------------------------------------------------------- normalisation
# B = 8 / 16 cases: the smallest shapes that reach each gn_mid_kernel instantiation (groups of 16+ channels that straddle the two sources
# keep the one-slab kernel out; B * (G / gq) >= 128 picks gq = 2 at B = 8 and gq = 4 at B = 16): <4>, <8>, <16> at 512 threads,
# <24, 512>, and <16> with gq = 4
_GN_MID_CASES = [(8, 264, 248, 16, 1, 1e-5), (8, 264, 248, 256, 1, 1e-5), (8, 1280, 640, 256, 1, 1e-5), (8, 1280, 1280, 256, 1, 1e-5),
                 (16, 1280, 640, 64, 1, 1e-5)]


@pytest.mark.parametrize("B,C0,C1,HW,silu,eps", [(3, 320, 0, 256, 1, 1e-5), (3, 640, 320, 64, 1, 1e-5), (3, 1280, 1280, 16, 1, 1e-5),
                                                 (3, 64, 0, 4, 0, 1e-6), (3, 32, 32, 256, 1, 1e-5), (3, 1280, 640, 64, 0, 1e-6)] + _GN_MID_CASES)
def test_groupnorm_silu(B, C0, C1, HW, silu, eps):
    G = 32
    C = C0 + C1
    H = int(math.isqrt(HW))
    x0 = bf(rnd(B, C0, H, H, seed=31) * 2 + 0.7)
    x1 = bf(rnd(B, C1, H, H, seed=32) - 0.4) if C1 else None
    gamma, beta = rnd(C, seed=33) * 0.3 + 1, rnd(C, seed=34) * 0.2
    out = torch.empty((B, HW, C), dtype=torch.bfloat16, device=DEV)
    part = torch.empty(B * 64 * G * 2, device=DEV)
    s0, s1 = gu.nhwc(x0), (gu.nhwc(x1) if C1 else None)      # keep the NHWC copies alive across the launch
    _lib.census_reset()
    _lib.call("dfh_groupnorm", _lib.ptr(s0), C0, _lib.ptr(s1), C1, B, HW, G,
              _lib.ptr(gamma), _lib.ptr(beta), eps, silu, _lib.ptr(out), _lib.ptr(part), gu.stream())
    torch.cuda.synchronize()
    if (B, C0, C1, HW, silu, eps) in _GN_MID_CASES:
        assert _lib.census()["gn_mid"] == 1, _lib.census()
    xin = torch.cat([x0, x1], 1).float() if C1 else x0.float()
    ref = F.group_norm(xin, G, gamma, beta, eps)
    ref = F.silu(ref) if silu else ref
    gu.assert_close_bf16(gu.nchw(out.view(B, H, H, C)), ref, f"groupnorm C={C} HW={HW}", rel=5e-3, max_rel=2e-2)


@pytest.mark.parametrize("M,C", [(300, 320), (64, 1280), (37, 32), (128, 640)])
def test_layernorm(M, C):
    x = bf(rnd(M, C, seed=35) * 3 + 1.5)
    gamma, beta = rnd(C, seed=36) * 0.3 + 1, rnd(C, seed=37) * 0.2
    y = torch.empty_like(x)
    _lib.call("dfh_layernorm", _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(y), M, C, 1e-5, gu.stream())
    torch.cuda.synchronize()
    gu.assert_close_bf16(y, F.layer_norm(x.float(), (C,), gamma, beta, 1e-5), "layernorm", rel=5e-3, max_rel=2e-2)


# ----------------------------------------------------------------------------- attention
def _attention(q, k, v, heads):
    """q [B][Nq][C], k/v [B][Nk][C] bf16 -> O via the HIP kernel (V handed over transposed + padded)."""
    B, Nq, Cc = q.shape
    Nk = k.shape[1]
    ld = (Nk + 7) // 8 * 8
    vt = torch.full((B, Cc, ld), float("nan"), dtype=torch.bfloat16, device=DEV)   # padding must be ignored
    vt[:, :, :Nk] = v.transpose(1, 2)
    o = torch.empty_like(q)
    d = Cc // heads
    _lib.call("dfh_attention", _lib.ptr(q), Cc, _lib.ptr(k), Cc, _lib.ptr(vt), ld, _lib.ptr(o), Cc, B, heads, d, Nq, Nk,
              d ** -0.5, gu.stream())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("d,heads", [(40, 8), (80, 8), (160, 8), (32, 2), (64, 5), (128, 2)])
@pytest.mark.parametrize("Nq,Nk", [(256, 256), (64, 64), (200, 77), (4, 4), (1024, 1024)])
def test_attention(d, heads, Nq, Nk):
    B, Cc = 2, d * heads
    q, k, v = bf(rnd(B, Nq, Cc, seed=40)), bf(rnd(B, Nk, Cc, seed=41)), bf(rnd(B, Nk, Cc, seed=42))
    o = _attention(q, k, v, heads)
    qh, kh, vh = (t.float().view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Nq, Cc)
    # P is rounded to bf16 before the PV MFMA: rel error budget ~2^-8 on top of the output rounding
    gu.assert_close_bf16(o, ref, f"attention d={d} {Nq}x{Nk}", rel=1e-2, max_rel=4e-2)


def test_attention_online_softmax_rescale_is_exercised():
    """A late key tile carries a much larger score than the first: the running max must jump and the
    accumulated O / l be rescaled (guide rule 26: force the rare branch)."""
    B, heads, d, N = 1, 1, 64, 256
    q, k, v = bf(rnd(B, N, d, seed=43)), bf(rnd(B, N, d, seed=44)), bf(rnd(B, N, d, seed=45))
    k[:, 200] = q[:, 7] * 6.0      # spike: key 200 (4th tile) aligned with query 7
    o = _attention(q, k, v, heads)
    ref = F.scaled_dot_product_attention(q.float()[:, None], k.float()[:, None], v.float()[:, None])[:, 0]
    gu.assert_close_bf16(o, ref, "rescale", rel=1e-2, max_rel=4e-2)


@pytest.mark.parametrize("d,heads", [(40, 8), (80, 4), (64, 5)])
@pytest.mark.parametrize("Nq,Nk", [(256, 64), (512, 77), (300, 200), (2048, 2048), (512, 640), (1024, 129), (1030, 1100)])
def test_attention_x32_shapes(d, heads, Nq, Nk):
    """The 32x32x16 kernel (attention_x32.hip) takes d = 40 / 80 with Nq >= 256, Nk >= 64: full tiles, ragged key
    tails in the first / second / a later LDS buffer (masked through the spare contraction slot), ragged query blocks."""
    B, Cc = 2, d * heads
    q, k, v = bf(rnd(B, Nq, Cc, seed=60)), bf(rnd(B, Nk, Cc, seed=61)), bf(rnd(B, Nk, Cc, seed=62))
    o = _attention(q, k, v, heads)
    qh, kh, vh = (t.float().view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Nq, Cc)
    gu.assert_close_bf16(o, ref, f"attention_x32 d={d} {Nq}x{Nk}", rel=1e-2, max_rel=4e-2)


@pytest.mark.parametrize("d,heads", [(40, 8), (80, 4)])
@pytest.mark.parametrize("B,Nq,Nk,gain", [(8, 4096, 77, 1.0), (2, 300, 13, 1.0), (3, 1024, 128, 1.0), (2, 512, 65, 4.0), (16, 1024, 77, 1.0)])
def test_attention_short_key_ranges_stream_query_blocks(d, heads, B, Nq, Nk, gain):
    """attention_xs_kernel (attention_x32.hip): cross-attention over <= 128 keys -- K / V^T staged once, every wave walks several query
    blocks (B = 8 / 16 at 4096 / 1024 queries: two and more blocks per wave), one or two key tiles, ragged tails incl. a second tile of
    ONE key, ragged query blocks, and scores whose maximum moves in the second tile (gain 4, one aligned key beyond key 64)."""
    Cc = d * heads
    q, k, v = bf(rnd(B, Nq, Cc, seed=70) * gain), bf(rnd(B, Nk, Cc, seed=71) * gain), bf(rnd(B, Nk, Cc, seed=72))
    if Nk > 64:
        k[:, Nk - 1] = q[:, 5] * 3.0       # the LAST key dominates query 5: the running offset is raised in tile 1
    from difashion_amd import _lib as L
    L.census_reset()
    o = _attention(q, k, v, heads)
    assert L.census()["attention_x32"] == (1 if Nk >= 64 else 0)      # fewer than 64 keys: the 16x16 kernel
    qh, kh, vh = (t.float().view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Nq, Cc)
    gu.assert_close_bf16(o, ref, f"attention_xs d={d} {Nq}x{Nk}", rel=1.5e-2 if gain > 1 else 1e-2, max_rel=0.12 if gain > 1 else 4e-2)


@pytest.mark.parametrize("d", [40, 80])
@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_attention_x32_running_max_moves(d, gain):
    """Keys of a late tile carry far larger scores than the first tile for some queries, far smaller for the rest
    (guide rule 26: force the rare rescale branch); gain 4 puts the running max near 60 log2 units, where its bf16
    rounding (it rides in a contraction slot of Q) is 0.25 -- the result must not depend on that rounding."""
    B, heads, N = 1, 2, 512
    Cc = d * heads
    q, k, v = bf(rnd(B, N, Cc, seed=63) * gain), bf(rnd(B, N, Cc, seed=64) * gain), bf(rnd(B, N, Cc, seed=65))
    k[:, 300] = q[:, 7] * 3.0          # key 300 (tile 4) aligned with query 7, both heads
    k[:, 450] = q[:, 260] * 5.0        # key 450 (tile 7) aligned with query 260 (second wave)
    o = _attention(q, k, v, heads)
    qh, kh, vh = (t.float().view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, N, Cc)
    # gain 4: near one-hot rows over scores of ~+-70 log2 units -- the standalone op re-rounds Q after its pre-scale by
    # scale * log2(e) (2^-9 relative per element, i.e. ~0.03 log2 units on such scores); inside the U-Net the scale is folded
    # into the to_q projection's epilogue instead (one rounding)
    gu.assert_close_bf16(o, ref, f"x32 rescale d={d} gain={gain}", rel=1.5e-2, max_rel=6e-2 if gain == 1.0 else 0.12)


@pytest.mark.parametrize("d", [40, 80])
def test_attention_x32_poisoned_fast_pass_is_repeated(d):
    """One key of a tile after the first scores more than 100 log2 units above everything the first tile held: the fast pass's
    unchecked exp leaves a denominator of >= 2^100, the workgroup raises its poison flag and repeats the pass in the exact
    deferred-max form (attention_x32.hip, `pass`).  The precondition is checked on the CPU in float64 before the kernel runs."""
    B, heads, N = 1, 2, 512
    Cc = d * heads
    q, k, v = bf(rnd(B, N, Cc, seed=63)), bf(rnd(B, N, Cc, seed=64)), bf(rnd(B, N, Cc, seed=65))
    k[:, 300] = q[:, 7] * 16.0         # key 300 (tile 4) aligned with query 7, both heads
    s7 = torch.einsum("hd,nhd->hn", q[0, 7].double().cpu().view(heads, d), k[0].double().cpu().view(N, heads, d)) \
        * d ** -0.5 * math.log2(math.e)
    jump = s7[:, 300] - s7[:, :64].max(dim=1).values
    assert (jump > 100).all(), f"planted score only {jump.tolist()} log2 units above tile 0: the fast pass would not be poisoned"
    o = _attention(q, k, v, heads)
    assert torch.isfinite(o.float()).all()
    qh, kh, vh = (t.float().view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, N, Cc)
    gu.assert_close_bf16(o, ref, f"x32 poison re-run d={d}", rel=1.5e-2, max_rel=0.12)


def test_attention_x32_matches_the_16x16_kernel_lse():
    """Training reads the forward's log-sum-exp: both kernels must report the same one."""
    B, heads, d, N = 1, 2, 40, 512
    Cc = d * heads
    q, k, v = bf(rnd(B, N, Cc, seed=66)), bf(rnd(B, N, Cc, seed=67)), bf(rnd(B, N, Cc, seed=68))
    vt = v.transpose(1, 2).contiguous()
    o = torch.empty_like(q)
    lse = torch.empty((B, heads, N), device=DEV)
    _lib.call("dfh_attention_lse", _lib.ptr(q), Cc, _lib.ptr(k), Cc, _lib.ptr(vt), N, _lib.ptr(o), Cc, B, heads, d, N, N,
              d ** -0.5, _lib.ptr(lse), gu.stream())
    torch.cuda.synchronize()
    qh, kh = (t.float().view(B, -1, heads, d).transpose(1, 2) for t in (q, k))
    ref = torch.logsumexp(qh @ kh.transpose(-1, -2) * d ** -0.5, dim=-1) * 1.4426950408889634     # log2 domain
    assert (lse - ref).abs().max().item() <= 2e-2


# ----------------------------------------------------------------------------- small kernels
def test_timestep_embedding():
    t = torch.tensor([0.0, 1.0, 481.0, 999.0], device=DEV)
    out = torch.empty((4, 320), dtype=torch.bfloat16, device=DEV)
    _lib.call("dfh_timestep_embedding", _lib.ptr(t), _lib.ptr(out), 4, 320, gu.stream())
    torch.cuda.synchronize()
    ref = unet_ref.timestep_embedding(t.cpu(), 320)
    assert gu.max_err(out.cpu(), ref) <= 2 ** -8     # bf16 rounding of values in [-1, 1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nchw_to_nhwc(dtype):
    x = rnd(3, 8, 16, 16, seed=50).to(dtype)
    out = torch.empty((3, 256, 8), dtype=torch.bfloat16, device=DEV)
    _lib.call("dfh_nchw_to_nhwc_bf16", _lib.ptr(x), int(dtype == torch.bfloat16), _lib.ptr(out), 3, 8, 256, gu.stream())
    torch.cuda.synchronize()
    assert torch.equal(out.view(3, 16, 16, 8), gu.nhwc(bf(x)))


def test_weight_packers_are_exact():
    w = rnd(24, 16, 3, 3, seed=51)
    assert torch.equal(gu.pack_conv(w), bf(w.permute(0, 2, 3, 1).reshape(24, -1)))


# ----------------------------------------------------------------------------- DiFashion glue kernels (bit-exact fp32)
def test_mutual_reduce_sampling_and_training_bit_exact():
    from difashion_amd.pipeline import sampling_tables, training_tables
    olists = torch.tensor([[0, 0, 5, 6], [7, 0, 0, 0], [1, 2, 3, 0]])
    L = 4 * 16 * 16
    given = rnd(12, 4, 16, 16, seed=52)
    gen = rnd(6, 4, 16, 16, seed=53)
    tab, wt = (t.to(DEV) for t in sampling_tables(olists))     # named: never take pointers of temporaries
    out = torch.empty((6, L), dtype=torch.bfloat16, device=DEV)
    out32 = torch.empty((6, L), device=DEV)
    _lib.call("dfh_mutual_reduce", _lib.ptr(gen), _lib.ptr(given), _lib.ptr(tab), _lib.ptr(wt),
              _lib.ptr(out), _lib.ptr(out32), 6, 4, L, gu.stream())
    torch.cuda.synchronize()
    ref = glue_ref.mutual_sum(olists, given.cpu(), gen.cpu())
    assert torch.equal(out32.cpu().view_as(ref), ref)
    assert torch.equal(out.cpu().view_as(ref), bf(ref))
    tab, wt = (t.to(DEV) for t in training_tables(8, 4))
    noisy = rnd(8, 4, 16, 16, seed=54)
    o32 = torch.empty((8, L), device=DEV)
    o16 = torch.empty((8, L), dtype=torch.bfloat16, device=DEV)
    _lib.call("dfh_mutual_reduce", _lib.ptr(noisy), None, _lib.ptr(tab), _lib.ptr(wt), _lib.ptr(o16),
              _lib.ptr(o32), 8, 4, L, gu.stream())
    torch.cuda.synchronize()
    ref = glue_ref.mutual_mean(noisy.cpu(), 4)
    assert torch.equal(o32.cpu().view_as(ref), ref)


def test_assemble_input_bit_exact():
    Fn, CL = 3, 4 * 8 * 8
    lat, mut, hist = rnd(Fn, 4, 8, 8, seed=55), rnd(Fn, 4, 8, 8, seed=56), rnd(Fn, 4, 8, 8, seed=57)
    null = rnd(4, 8, 8, seed=58)
    mreal = torch.tensor([1, 1, 0, 0], dtype=torch.uint8, device=DEV)
    hreal = torch.tensor([1, 0, 0, 0], dtype=torch.uint8, device=DEV)
    x = torch.empty((4 * Fn, 8, 8, 8), device=DEV)
    _lib.call("dfh_assemble_input", _lib.ptr(lat), _lib.ptr(mut), _lib.ptr(hist), _lib.ptr(null), _lib.ptr(mreal),
              _lib.ptr(hreal), _lib.ptr(x), 4, Fn, CL, float(1 - 0.1), 0.1, 0, gu.stream())
    torch.cuda.synchronize()
    nulls = null[None].expand(Fn, -1, -1, -1)
    mstack = torch.cat([mut, mut, nulls, nulls])
    hstack = torch.cat([hist, nulls, nulls, nulls])
    ref = torch.cat([(1 - 0.1) * torch.cat([lat] * 4) + 0.1 * mstack, hstack], dim=1)   # difashion.py:514-515
    assert torch.equal(x, ref)


@pytest.mark.parametrize("mode,name,R", [(1, "full", 4), (2, "cate_hist", 3), (3, "cate_mutual", 3), (4, "cate", 2),
                                         (5, "hist", 2), (6, "mutual", 2), (0, "none", 1)])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_cfg_combine_and_ddim_step_match_oracle(mode, name, R, pred):
    from difashion_amd.schedulers import DDIMScheduler
    Fn = 3
    eps_all = rnd(R * Fn, 4, 8, 8, seed=59)
    lat = rnd(Fn, 4, 8, 8, seed=60)
    sc, sh, sm = 12.0, 4.0, 5.0
    ref_s = sched_ref.DDIMRef(prediction_type=pred)
    ref_s.set_timesteps(50)
    s = DDIMScheduler(prediction_type=pred)
    s.set_timesteps(50)
    for t in (981, 501, 21, 1):
        eps_ref = glue_ref.cfg_combine(name, eps_all.cpu(), sc, sh, sm)
        prev_ref = ref_s.step(eps_ref, t, lat.cpu(), eta=0.0, return_dict=False)[0]
        x = lat.clone()
        eps_out = torch.empty_like(lat)
        k = s.step_coef(t, 0.0)
        _lib.call("dfh_cfg_step", _lib.ptr(eps_all), _lib.ptr(x), _lib.ptr(eps_out), None, x.numel(), mode, sc, sh, sm,
                  C.byref(k), gu.stream())
        torch.cuda.synchronize()
        assert torch.equal(eps_out.cpu(), eps_ref)                       # guidance combine: bit-exact
        torch.testing.assert_close(x.cpu(), prev_ref, rtol=2e-6, atol=2e-6)   # fp32 update, <= 2 ulp-ish
        torch.testing.assert_close(s.step(eps_ref.to(DEV), t, lat, return_dict=False)[0].cpu(), prev_ref, rtol=2e-6, atol=2e-6)


def test_ddim_eta_noise_and_scheduler_api():
    import inspect
    from difashion_amd.schedulers import DDIMScheduler, PNDMScheduler
    s, r = DDIMScheduler(), sched_ref.DDIMRef()
    s.set_timesteps(50, device=DEV)
    r.set_timesteps(50)
    assert s.timesteps.tolist() == r.timesteps.tolist() and s.timesteps.device.type == "cuda"
    assert {"eta", "generator"} <= set(inspect.signature(s.step).parameters)          # difashion.py:665-673
    assert not ({"eta", "generator"} & set(inspect.signature(PNDMScheduler().step).parameters))
    eps, x, z = rnd(2, 4, 8, 8, seed=61), rnd(2, 4, 8, 8, seed=62), rnd(2, 4, 8, 8, seed=63)
    got = s.step(eps, s.timesteps[3], x, eta=0.7, variance_noise=z).prev_sample
    ref = r.step(eps.cpu(), 921, x.cpu(), eta=0.7, variance_noise=z.cpu())["prev_sample"]
    torch.testing.assert_close(got.cpu(), ref, rtol=3e-6, atol=3e-6)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_add_noise_velocity_and_pndm_match_oracle(pred):
    """PNDM / PLMS is the scheduler the reference instantiates (difashion.py:64) and ``prediction_type`` the switch it branches on
    (:241-247): both settings through the whole 11-entry PLMS list (warm-up step, 2-, 3- and 4-term blends)."""
    from difashion_amd.schedulers import DDIMScheduler, PNDMScheduler
    s, r = DDIMScheduler(), sched_ref.DDIMRef()
    x0, n = rnd(6, 4, 8, 8, seed=64), rnd(6, 4, 8, 8, seed=65)
    t = torch.tensor([0, 1, 500, 999, 37, 640], device=DEV)
    assert torch.equal(s.add_noise(x0, n, t).cpu(), r.add_noise(x0.cpu(), n.cpu(), t.cpu()))
    assert torch.equal(s.get_velocity(x0, n, t).cpu(), r.get_velocity(x0.cpu(), n.cpu(), t.cpu()))
    p, pr = PNDMScheduler(prediction_type=pred), sched_ref.PNDMRef(prediction_type=pred)
    p.set_timesteps(10, device=DEV)
    pr.set_timesteps(10)
    assert p.timesteps.tolist() == pr.timesteps.tolist()
    x, xr = rnd(2, 4, 8, 8, seed=66), None
    xr = x.cpu().clone()
    for i, tt in enumerate(pr.timesteps.tolist()):
        e = rnd(2, 4, 8, 8, seed=70 + i)
        x = p.step(e, tt, x, return_dict=False)[0]
        xr = pr.step(e.cpu(), tt, xr, return_dict=False)[0]
        torch.testing.assert_close(x.cpu(), xr, rtol=2e-5, atol=2e-5)


def test_mse_rows():
    a, b = rnd(5, 4, 16, 16, seed=67), rnd(5, 4, 16, 16, seed=68)
    out = torch.empty(5, device=DEV)
    _lib.call("dfh_mse_rows", _lib.ptr(a), _lib.ptr(b), _lib.ptr(out), 5, 1024, gu.stream())
    torch.cuda.synchronize()
    torch.testing.assert_close(out, ((a - b) ** 2).mean(dim=(1, 2, 3)), rtol=1e-5, atol=1e-7)


def test_error_reporting_is_loud():
    with pytest.raises(_lib.DfhError, match="multiple of 4"):
        gu.gemm(M=8, N=6, W=bf(rnd(6, 64)), ldw=64, a0=bf(rnd(8, 64)), a0_c=64)
    with pytest.raises(_lib.DfhError, match="unsupported head dim"):
        q = bf(rnd(1, 16, 48))
        _lib.call("dfh_attention", _lib.ptr(q), 48, _lib.ptr(q), 48, _lib.ptr(q), 16, _lib.ptr(q), 48, 1, 1, 48, 16, 16, 1.0, gu.stream())


# ----------------------------------------------------------------------------- fp8 linears (BASELINE configs[4])
def _fp8_dequant(q, scale):
    return q.view(torch.float8_e4m3fn).float() * scale[:, None]


def test_fp8_row_quantiser_matches_torch_e4m3():
    x = bf(rnd(70, 192, seed=80) * 3)
    x[5] = 0                                                   # an all-zero row keeps scale 1
    q = torch.empty((70, 192), dtype=torch.uint8, device=DEV)
    sc = torch.empty(70, device=DEV)
    _lib.call("dfh_quantize_rows_fp8", _lib.ptr(x), 192, _lib.ptr(q), _lib.ptr(sc), 70, 192, gu.stream())
    torch.cuda.synchronize()
    want_sc = x.float().abs().amax(dim=1) / 448.0
    want_sc[5] = 1.0
    torch.testing.assert_close(sc, want_sc, rtol=1e-6, atol=0)
    want_q = (x.float() * (1.0 / want_sc)[:, None]).to(torch.float8_e4m3fn)  # x * (1 / scale) as the kernel does; OCP e4m3fn, RNE
    got_f, want_f = q.view(torch.float8_e4m3fn).float(), want_q.float()
    diff = got_f != want_f            # v_cvt_pk_fp8_f32 vs torch's converter: the same OCP grid; a tie may break the other way
    assert float(diff.float().mean()) <= 5e-3 and bool(((got_f - want_f).abs() <= 0.126 * want_f.abs())[diff].all())
    assert float(got_f.abs().max()) == 448.0 and not torch.isnan(got_f).any()
    assert gu.rel_err(_fp8_dequant(q, sc), x.float()) <= 4e-2                  # 3 mantissa bits: 2^-4 relative per element


@pytest.mark.parametrize("M,C", [(300, 320), (64, 1280), (128, 640)])
def test_layernorm_fp8_matches_layernorm_then_quantise(M, C):
    x = bf(rnd(M, C, seed=81) * 3 + 1.5)
    gamma, beta = rnd(C, seed=82) * 0.3 + 1, rnd(C, seed=83) * 0.2
    q = torch.empty((M, C), dtype=torch.uint8, device=DEV)
    sc = torch.empty(M, device=DEV)
    _lib.call("dfh_layernorm_fp8", _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(q), _lib.ptr(sc), M, C, 1e-5, gu.stream())
    torch.cuda.synchronize()
    ref = F.layer_norm(x.float(), (C,), gamma, beta, 1e-5)
    assert gu.rel_err(_fp8_dequant(q, sc), ref) <= 4e-2
    torch.testing.assert_close(sc, bf(ref).float().abs().amax(dim=1) / 448.0, rtol=2e-2, atol=1e-6)


def _fp8_desc(**kw):
    """Zero-initialised dfh_gemm_fp8_desc with the given fields; tensors are kept alive on the returned object."""
    d = _lib.Fp8GemmDesc()
    d.keep = []
    for k, v in kw.items():
        if torch.is_tensor(v):
            d.keep.append(v)
            v = v.data_ptr()
        setattr(d, k, v)
    z = gu.zero_page()
    d.keep.append(z)
    d.zero_page = z.data_ptr()
    return d


def _fp8_gemm(x, w, bias=None, resid=None, act=0, out_mode=0, rows_per_b=0, amax=None):
    """x [M][K], w [N][K] bf16 -> quantised by the library -> dfh_gemm_fp8; returns (out, dequantised x, dequantised w)."""
    M, K = x.shape
    N = w.shape[0]
    xq, wq = torch.empty((M, K), dtype=torch.uint8, device=DEV), torch.empty((N, K), dtype=torch.uint8, device=DEV)
    xs, ws = torch.empty(M, device=DEV), torch.empty(N, device=DEV)
    _lib.call("dfh_quantize_rows_fp8", _lib.ptr(x), K, _lib.ptr(xq), _lib.ptr(xs), M, K, gu.stream())
    _lib.call("dfh_quantize_rows_fp8", _lib.ptr(w), K, _lib.ptr(wq), _lib.ptr(ws), N, K, gu.stream())
    n_out = N // 2 if act == 4 else N
    if out_mode == 1:
        nb = M // rows_per_b
        out = torch.full((nb, N, rows_per_b), float("nan"), dtype=torch.bfloat16, device=DEV)
        ld = rows_per_b
    else:
        out = torch.full((M, n_out), float("nan"), dtype=torch.bfloat16, device=DEV)
        ld = n_out
    kw = dict(A=xq, sA=xs, W=wq, sW=ws, M=M, N=N, K=K, ld_res=N, act=act, out=out, ld_out=ld, out_mode=out_mode, rows_per_b=rows_per_b)
    if bias is not None:
        kw["bias"] = bias
    if resid is not None:
        kw["resid"] = resid
    if amax is not None:
        kw["amax"] = amax
    d = _fp8_desc(**kw)
    _lib.call("dfh_gemm_fp8", C.byref(d), gu.stream())
    torch.cuda.synchronize()
    return out, _fp8_dequant(xq, xs), _fp8_dequant(wq, ws)


def _e4m3_random(shape, seed):
    """Random e4m3 bytes (finite: no NaN pattern 0x7f / 0xff) and their float values."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, shape, generator=g, dtype=torch.int32)
    q = torch.where((q & 0x7f) == 0x7f, q - 9, q).to(torch.uint8).to(DEV)
    return q, q.view(torch.float8_e4m3fn).float()


def _mx_dequant(q, sx):
    """q [M][K] e4m3 bytes, sx [K / 32][M] E8M0 bytes -> fp32 values."""
    M, K = q.shape
    scale = torch.exp2(sx.float() - 127.0).t().contiguous()              # [M][K / 32]
    return q.view(torch.float8_e4m3fn).float() * scale.repeat_interleave(32, dim=1)


@pytest.mark.parametrize("M,N,K", [(256, 160, 64), (384, 320, 320), (1000, 128, 256), (16384, 320, 1280), (4096, 1280, 5120), (68, 64, 128)])
def test_gemm_fp8_block_scaled_operand(M, N, K):
    """The E8M0 block scales of the activations go through the MFMA's own scale operand (one byte per lane = per row and 32 contraction
    elements, staged per k-step by LDS-DMA from the [K / 32][M] layout).  Random e4m3 bytes and random scales 2^-6 .. 2^6 that differ
    for every (row, block): a scale applied to the wrong row, the wrong k-half or the wrong k-step cannot pass.  Exact arithmetic apart
    from accumulation order and the bf16 output rounding."""
    xq, xf = _e4m3_random((M, K), 101)
    wq, wf = _e4m3_random((N, K), 102)
    xf, wf = xf * 2.0 ** -4, wf * 2.0 ** -6
    sx = torch.randint(121, 134, (K // 32, M), generator=torch.Generator().manual_seed(103), dtype=torch.int32).to(torch.uint8).to(DEV)
    ws = torch.rand(N, generator=torch.Generator().manual_seed(104)).to(DEV) * 2.0 ** -6 + 2.0 ** -7
    bias, resid = rnd(N, seed=105), bf(rnd(M, N, seed=106))
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    d = _fp8_desc(A=xq, sx=sx, sa_mul=2.0 ** -4, W=wq, sW=ws, M=M, N=N, K=K, bias=bias, resid=resid, ld_res=N, out=out, ld_out=N)
    _lib.call("dfh_gemm_fp8", C.byref(d), gu.stream())
    torch.cuda.synchronize()
    xd = _mx_dequant(xq, sx) * 2.0 ** -4
    ref = (xd.double() @ (wq.view(torch.float8_e4m3fn).double() * ws.double()[:, None]).t()).float() + bias + resid.float()
    gu.assert_close_bf16(out, ref, f"fp8 MX gemm {M}x{N}x{K}")


@pytest.mark.parametrize("M,C", [(512, 64), (4096, 320), (1040, 640)])
def test_gemm_fp8_geglu_writes_the_block_scaled_hidden_tensor_and_ff2_reads_it(M, C):
    """ff.net.0 -> GEGLU with the hidden tensor leaving as e4m3 + one E8M0 scale per token and 32 hidden units (OUT_FP8_MX), then
    ff.net.2 consuming exactly that pair.  The dequantised hidden tensor must sit within the e4m3 rounding of the fp32 GEGLU of the same
    (dequantised) operands, every scale must be the smallest power of two that keeps its block inside +-448, and the second GEMM must be
    exact on what the first one wrote."""
    x = bf(rnd(M, C, seed=88))
    w = rnd(8 * C, C, seed=89, scale=0.1)
    b = rnd(8 * C, seed=90, scale=0.5)
    wp = torch.empty((8 * C, C), dtype=torch.bfloat16, device=DEV)
    bp = torch.empty(8 * C, dtype=torch.float32, device=DEV)
    _lib.call("dfh_pack_matrix", _lib.ptr(w), _lib.ptr(wp), 8 * C, C, C, 0, 0, 1, gu.stream())       # value / gate rows interleaved
    _lib.call("dfh_pack_vector", _lib.ptr(b), _lib.ptr(bp), 8 * C, 0, 1, 0, gu.stream())
    xq, wq = torch.empty((M, C), dtype=torch.uint8, device=DEV), torch.empty((8 * C, C), dtype=torch.uint8, device=DEV)
    xs, ws = torch.empty(M, device=DEV), torch.empty(8 * C, device=DEV)
    _lib.call("dfh_quantize_rows_fp8", _lib.ptr(x), C, _lib.ptr(xq), _lib.ptr(xs), M, C, gu.stream())
    _lib.call("dfh_quantize_rows_fp8", _lib.ptr(wp), C, _lib.ptr(wq), _lib.ptr(ws), 8 * C, C, gu.stream())
    import ctypes
    hid = torch.full((M, 4 * C), 0x7f, dtype=torch.uint8, device=DEV)
    hsx = torch.zeros((4 * C // 32, M), dtype=torch.uint8, device=DEV)
    d = _fp8_desc(A=xq, sA=xs, W=wq, sW=ws, M=M, N=8 * C, K=C, bias=bp, act=4, out=hid, ld_out=4 * C, out_mode=4, out_sx=hsx)
    _lib.call("dfh_gemm_fp8", ctypes.byref(d), gu.stream())
    torch.cuda.synchronize()
    xd, wd = _fp8_dequant(xq, xs), _fp8_dequant(wq, ws)
    wdv = wd.view(-1, 2, 16, C)
    wv, wg = wdv[:, 0].reshape(-1, C), wdv[:, 1].reshape(-1, C)
    ref = (xd @ wv.T + b[:4 * C]) * F.gelu(xd @ wg.T + b[4 * C:])
    got = _mx_dequant(hid, hsx)
    assert not torch.isnan(got).any()
    assert gu.rel_err(got, ref) <= 4e-2                                   # 3 mantissa bits
    blk = ref.abs().view(M, -1, 32).amax(dim=2)                           # the scale each block should carry
    want = torch.clamp(torch.ceil(torch.log2(blk / 448.0)) + 127, 1, 253)
    have = hsx.float().t()
    assert float((have != want).float().mean()) <= 2e-3                  # an amax that sits within rounding of a power-of-two boundary may tip
    assert float(got.abs().view(M, -1, 32).amax(dim=2).div(torch.exp2(have - 127)).max()) <= 448.0
    # ff.net.2 on that pair: + bias + residual, bf16 out AND e4m3 + E8M0 out (the operand of proj_out)
    w2 = bf(rnd(C, 4 * C, seed=91, scale=0.05))
    w2q, w2s = torch.empty((C, 4 * C), dtype=torch.uint8, device=DEV), torch.empty(C, device=DEV)
    _lib.call("dfh_quantize_rows_fp8", _lib.ptr(w2), 4 * C, _lib.ptr(w2q), _lib.ptr(w2s), C, 4 * C, gu.stream())
    b2, res = rnd(C, seed=92), bf(rnd(M, C, seed=93))
    out = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    d2 = _fp8_desc(A=hid, sx=hsx, W=w2q, sW=w2s, M=M, N=C, K=4 * C, bias=b2, resid=res, ld_res=C, out=out, ld_out=C)
    _lib.call("dfh_gemm_fp8", ctypes.byref(d2), gu.stream())
    ref2 = got @ _fp8_dequant(w2q, w2s).T + b2 + res.float()
    gu.assert_close_bf16(out, ref2, "ff2 on the block-scaled hidden tensor")
    if C % 32 == 0:
        o8 = torch.full((M, C), 0x7f, dtype=torch.uint8, device=DEV)
        osx = torch.zeros((C // 32, M), dtype=torch.uint8, device=DEV)
        d3 = _fp8_desc(A=hid, sx=hsx, W=w2q, sW=w2s, M=M, N=C, K=4 * C, bias=b2, resid=res, ld_res=C, out=o8, ld_out=C, out_mode=4, out_sx=osx)
        _lib.call("dfh_gemm_fp8", ctypes.byref(d3), gu.stream())
        torch.cuda.synchronize()
        assert gu.rel_err(_mx_dequant(o8, osx), ref2) <= 4e-2


def test_gemm_fp8_transposed_output_tracks_the_maximum_per_batch_element():
    """The V projection's epilogue leaves max |V| per batch element (atomicMax on the float bits): the bound the attention output is
    quantised against.  Batches of 192 rows (whole 32-row wave blocks: one atomic per wave) and of 200 rows (blocks straddle images: one
    per lane)."""
    for rows in (192, 200):
        B, N, K = 3, 320, 320
        x, w = bf(rnd(B * rows, K, seed=91)), bf(rnd(N, K, seed=92, scale=0.1))
        x[rows:2 * rows] *= 3.0
        am = torch.zeros(B, device=DEV)
        out, xd, wd = _fp8_gemm(x, w, out_mode=1, rows_per_b=rows, amax=am)
        torch.cuda.synchronize()
        assert torch.equal(am, out.float().abs().amax(dim=(1, 2)))


@pytest.mark.parametrize("B,HW,Cc", [(2, 4096, 320), (3, 1024, 640), (4, 256, 1280), (16, 64, 1280), (2, 16, 64)])
def test_groupnorm_fp8_output_is_the_normalised_value_under_the_static_scale(B, HW, Cc):
    """proj_in's e4m3 operand: the GroupNorm kernels (two-kernel path, one-slab path) emit (x - mean) * rstd * q_mul as e4m3 -- no
    affine (the consumer's weights carry gamma), no statistics of the output needed (static scale).  Dequantised it must sit within the
    e4m3 rounding of F.group_norm without affine."""
    x = bf(rnd(B, HW, Cc, seed=140) * 2.0 + 0.7)
    q = torch.full((B, HW, Cc), 0x7f, dtype=torch.uint8, device=DEV)
    partial = torch.zeros(B * 64 * 64 * 2, device=DEV)
    _lib.call("dfh_groupnorm_fp8", _lib.ptr(x), B, HW, Cc, 32, 1e-6, 14.0, _lib.ptr(q), _lib.ptr(partial), gu.stream())
    torch.cuda.synchronize()
    ref = F.group_norm(x.float().permute(0, 2, 1), 32, eps=1e-6).permute(0, 2, 1)
    got = q.view(torch.float8_e4m3fn).float() / 14.0
    assert not torch.isnan(got).any() and gu.rel_err(got, ref) <= 4e-2


@pytest.mark.parametrize("B,H,D,Nq,Nk", [(2, 8, 40, 4096, 4096), (2, 8, 40, 1024, 77), (3, 8, 80, 1024, 1024), (2, 8, 160, 256, 256), (2, 8, 160, 64, 77),
                                         (2, 2, 32, 16, 16)])
def test_attention_fp8_output_is_scaled_by_the_maximum_of_v(B, H, D, Nq, Nk):
    """to_out's e4m3 operand, written by the attention epilogues (32x32x16 kernel, the short-key kernel, the 16x16x32 kernel): the
    normalised output times 448 / max |V| of the batch element.  Against the bf16 output of the same launch."""
    Cc = H * D
    q, k = bf(rnd(B, Nq, Cc, seed=150)), bf(rnd(B, Nk, Cc, seed=151))
    Np = (Nk + 7) // 8 * 8
    vt = torch.zeros(B, Cc, Np, dtype=torch.bfloat16, device=DEV)
    vt[:, :, :Nk] = bf(rnd(B, Cc, Nk, seed=152))
    vt[1] *= 5.0
    am = vt.float().abs().amax(dim=(1, 2)).contiguous()
    o16 = torch.empty(B, Nq, Cc, dtype=torch.bfloat16, device=DEV)
    o8 = torch.full((B, Nq, Cc), 0x7f, dtype=torch.uint8, device=DEV)
    args = (_lib.ptr(q), Cc, _lib.ptr(k), Cc, _lib.ptr(vt), Np)
    _lib.call("dfh_attention", *args, _lib.ptr(o16), Cc, B, H, D, Nq, Nk, D ** -0.5, gu.stream())
    _lib.call("dfh_attention_fp8out", *args, _lib.ptr(o8), Cc, _lib.ptr(am), B, H, D, Nq, Nk, D ** -0.5, gu.stream())
    torch.cuda.synchronize()
    got = o8.view(torch.float8_e4m3fn).float() * (am / 448.0)[:, None, None]
    assert not torch.isnan(got).any() and gu.rel_err(got, o16.float()) <= 4e-2


@pytest.mark.parametrize("B,H,D,N", [(2, 8, 40, 1024), (1, 8, 40, 4096), (2, 8, 80, 1024), (2, 8, 160, 256), (3, 8, 160, 64), (1, 4, 80, 200)])
def test_attention_fp8_products_match_the_bf16_kernel(B, H, D, N):
    """attention_fp8_kernel (both products on the e4m3 MFMA, operands quantised inside the kernel with static factors derived from the
    projection weights) against fp32 softmax attention of the same bf16 q / k / v, and against the bf16 kernel.  q, k, v are REAL
    projections of a LayerNorm-ed input (that is what the static bounds are derived for): x -> LayerNorm -> W' with channel-dependent
    row norms (a 7 x spread: the per-channel balancing of q and k has work to do) and a bias.  N = 200: the 64-query tail / ragged rows.
    Tolerance 8e-2 (measured 0.4e-2 .. 3.3e-2 on these moderately peaked softmaxes; with logits spread over +-25 -- weights 2.5 x larger --
    the e4m3 scores cost 0.10 - 0.15 where the bf16 kernel stays at 3e-3: the reason the kernel is opt-in beside being slower)."""
    Cc = H * D
    Nk = N if N % 64 == 0 else 256
    g = torch.Generator().manual_seed(180)
    x = torch.randn(B * max(N, Nk), Cc, generator=g).to(DEV)
    gamma, beta = 1.0 + 0.2 * rnd(Cc, seed=181), 0.2 * rnd(Cc, seed=182)
    spread = torch.exp(torch.linspace(-1.0, 1.0, 3 * Cc))[torch.randperm(3 * Cc, generator=g)].to(DEV)
    w = bf(rnd(3 * Cc, Cc, seed=183, scale=0.02) * spread[:, None])
    wf = torch.empty_like(w)
    sv, bv = torch.empty(3 * Cc, device=DEV), torch.empty(3 * Cc, device=DEV)
    _lib.call("dfh_ln_fold", _lib.ptr(w), Cc, _lib.ptr(gamma), _lib.ptr(beta), None, _lib.ptr(wf), _lib.ptr(sv), _lib.ptr(bv), 3 * Cc, Cc, gu.stream())
    rq, rk, rv, hs = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV), torch.empty(H, device=DEV)
    _lib.call("dfh_attn_scales", _lib.ptr(wf), _lib.ptr(bv), Cc, H, _lib.ptr(rq), _lib.ptr(rk), _lib.ptr(rv), _lib.ptr(hs), gu.stream())
    torch.cuda.synchronize()
    qkv = F.layer_norm(x, (Cc,), gamma, beta, 1e-5) @ w.float().T
    q = bf(qkv[:B * N, :Cc]).view(B, N, Cc).contiguous()
    k = bf(qkv[:B * Nk, Cc:2 * Cc]).view(B, Nk, Cc).contiguous()
    v = bf(qkv[:B * Nk, 2 * Cc:]).view(B, Nk, Cc)
    vt = v.transpose(1, 2).contiguous()
    # the factors really are bounds: no quantised operand can saturate
    assert float((q.float().abs() * rq).max()) <= 448.0 and float((k.float().abs() * rk).max()) <= 448.0 and float((v.float().abs() * rv).max()) <= 448.0
    torch.testing.assert_close((rq * rk).view(H, D), (1.0 / hs)[:, None].expand(H, D), rtol=1e-5, atol=0)
    o16 = torch.empty(B, N, Cc, dtype=torch.bfloat16, device=DEV)
    o8 = torch.full((B, N, Cc), float("nan"), dtype=torch.bfloat16, device=DEV)
    args = (_lib.ptr(q), Cc, _lib.ptr(k), Cc, _lib.ptr(vt), Nk)
    _lib.call("dfh_attention", *args, _lib.ptr(o16), Cc, B, H, D, N, Nk, D ** -0.5, gu.stream())
    _lib.census_reset()
    _lib.call("dfh_attention_fp8", *args, _lib.ptr(o8), Cc, _lib.ptr(rq), _lib.ptr(rk), _lib.ptr(rv), _lib.ptr(hs), B, H, D, N, Nk, D ** -0.5,
              gu.stream())
    torch.cuda.synchronize()
    assert _lib.census()["attention_fp8"] == 1
    ref = F.scaled_dot_product_attention(q.float().view(B, N, H, D).transpose(1, 2), k.float().view(B, Nk, H, D).transpose(1, 2),
                                         v.float().view(B, Nk, H, D).transpose(1, 2)).transpose(1, 2).reshape(B, N, Cc)
    e8, e16 = gu.rel_err(o8.float(), ref), gu.rel_err(o16.float(), ref)
    print(f"fp8 attention D={D} N={N}: rel err {e8:.2e} (bf16 kernel {e16:.2e})")
    assert not torch.isnan(o8).any() and e8 <= 8e-2


def test_amax_slabs():
    B, rows, ld = 3, 640, 80
    x = bf(rnd(B, rows, ld, seed=160))
    x[:, :, 77:] = float("nan")                      # pad columns (77 text tokens in rows of 80): never read
    row0 = torch.tensor([0, 64, 320], dtype=torch.int32, device=DEV)
    nrows = torch.tensor([64, 256, 320], dtype=torch.int32, device=DEV)
    out = torch.zeros(3, B, device=DEV)
    _lib.call("dfh_amax_slabs", _lib.ptr(x), rows * ld, ld, 77, _lib.ptr(row0), _lib.ptr(nrows), _lib.ptr(out), 3, B, gu.stream())
    torch.cuda.synchronize()
    want = torch.stack([x[:, r:r + n, :77].float().abs().amax(dim=(1, 2)) for r, n in ((0, 64), (64, 256), (320, 320))])
    assert torch.equal(out, want)


@pytest.mark.parametrize("M,N,K", [(256, 160, 64), (300, 320, 320), (1000, 640, 128), (4096, 2560, 320), (77, 24, 192), (12000, 960, 320)])
def test_gemm_fp8_exact_on_its_quantised_operands(M, N, K):
    """Against the product of the DEQUANTISED operands the kernel is an fp32-accumulating GEMM: only accumulation order and
    the final bf16 rounding remain (asymmetric random operands: a swapped operand / row / column map cannot pass)."""
    x, w = bf(rnd(M, K, seed=84)), bf(rnd(N, K, seed=85, scale=0.1))
    bias, resid = rnd(N, seed=86), bf(rnd(M, N, seed=87))
    out, xd, wd = _fp8_gemm(x, w, bias=bias, resid=resid)
    gu.assert_close_bf16(out, xd @ wd.T + bias + resid.float(), f"fp8 gemm {M}x{N}x{K}")
    # and the quantisation error itself against the bf16 operands: the stated fp8 tolerance (per-token x per-channel scales)
    assert gu.rel_err(out.float(), x.float() @ w.float().T + bias + resid.float()) <= 5e-2


@pytest.mark.parametrize("M,C", [(300, 64), (4096, 320), (520, 640)])
def test_gemm_fp8_geglu(M, C):
    x = bf(rnd(M, C, seed=88))
    w = rnd(8 * C, C, seed=89, scale=0.1)
    b = rnd(8 * C, seed=90, scale=0.5)
    wp = torch.empty((8 * C, C), dtype=torch.bfloat16, device=DEV)
    bp = torch.empty(8 * C, dtype=torch.float32, device=DEV)
    _lib.call("dfh_pack_matrix", _lib.ptr(w), _lib.ptr(wp), 8 * C, C, C, 0, 0, 1, gu.stream())       # value / gate rows interleaved
    _lib.call("dfh_pack_vector", _lib.ptr(b), _lib.ptr(bp), 8 * C, 0, 1, 0, gu.stream())
    out, xd, wd = _fp8_gemm(x, wp, bias=bp, act=4)
    # undo the 16-row interleave on the dequantised packed weights: packed row 32 j + i = value 16 j + i, + 16 = its gate
    wdv = wd.view(-1, 2, 16, C)
    wv, wg = wdv[:, 0].reshape(-1, C), wdv[:, 1].reshape(-1, C)
    a, gate = xd @ wv.T + b[:4 * C], xd @ wg.T + b[4 * C:]
    gu.assert_close_bf16(out, a * F.gelu(gate), "fp8 geglu")


def test_gemm_fp8_transposed_output():
    B, rows, N, K = 3, 200, 320, 320
    x, w = bf(rnd(B * rows, K, seed=91)), bf(rnd(N, K, seed=92, scale=0.1))
    out, xd, wd = _fp8_gemm(x, w, out_mode=1, rows_per_b=rows)
    ref = (xd @ wd.T).view(B, rows, N).transpose(1, 2)
    gu.assert_close_bf16(out, ref, "fp8 transposed")


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("M,parts,offset", [(128, 2, 0.0), (512, 2, 3.0), (1024, 5, 0.0), (384, 1, 0.0)])
def test_mlp_fused_matches_torch(M, parts, offset, form):
    """dfh_mlp_fused (csrc/mlp_fused2.hip; form 1 = the probe kernel scripts/probes/kernels/mlp_fused_v1.hip): the GEGLU feed-forward + proj_out of a C = 320 transformer block in one kernel,
    out = proj_out(ff.net.2(GEGLU(ff.net.0(LN3(x)))) + x) + resid, against fp32 torch on the same bf16 operands -- and against the
    two-launch walk it replaces (folded-LayerNorm GEGLU projection, then the [hidden | x] linear), in both forms of the kernel (32-token
    waves on the 32x32x16 MFMA, one per SIMD; 16-token waves on the 16x16x32 MFMA, two per SIMD: the walk's default).  Row statistics come in the producer's
    per-column-tile record layout (1, 2 or 5 tiles per row); rows with a common offset (mean >> std) included.  Both intermediate roundings
    of the unfused walk are kept (hidden units to bf16; the output once), so the two paths agree to bf16 accumulation-order noise."""
    import ctypes
    if form == 1 and "probes" not in os.environ.get("DFH_LIB", ""):
        pytest.skip("form 1 is a probe kernel (scripts/probes): needs DFH_LIB=<probe library>")
    C = 320
    x = bf(rnd(M, C, seed=71) + offset)
    resid = bf(rnd(M, C, seed=72))
    gamma, beta = 1.0 + 0.2 * rnd(C, seed=73), 0.3 * rnd(C, seed=74)
    wg, bg = rnd(8 * C, C, seed=75, scale=0.05), rnd(8 * C, seed=76, scale=0.3)          # ff.net.0.proj: rows [values | gates]
    w2, b2 = rnd(C, 4 * C, seed=77, scale=0.03), rnd(C, seed=78, scale=0.3)                # ff.net.2
    wo, bo = rnd(C, C, seed=79, scale=0.05), rnd(C, seed=80, scale=0.3)                    # proj_out
    # packed (16 values | 16 gates) GEGLU rows, LayerNorm folded in
    wp = torch.empty((8 * C, C), dtype=torch.bfloat16, device=DEV)
    bp = torch.empty(8 * C, dtype=torch.float32, device=DEV)
    _lib.call("dfh_pack_matrix", _lib.ptr(wg), _lib.ptr(wp), 8 * C, C, C, 0, 0, 1, gu.stream())
    _lib.call("dfh_pack_vector", _lib.ptr(bg), _lib.ptr(bp), 8 * C, 0, 1, 0, gu.stream())
    wf = torch.empty_like(wp)
    s1, b1 = torch.empty(8 * C, device=DEV), torch.empty(8 * C, device=DEV)
    _lib.call("dfh_ln_fold", _lib.ptr(wp), C, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(bp), _lib.ptr(wf), _lib.ptr(s1), _lib.ptr(b1), 8 * C, C, gu.stream())
    # [pout . ff2 | pout] and its bias, as unet_model.h derives them (fp32 product, one rounding)
    w2p = bf(torch.cat([wo.float() @ bf(w2).float(), bf(wo).float()], dim=1)).contiguous()
    w2p[:, 4 * C:] = bf(wo)
    bias = (bf(wo).float() @ b2 + bo).contiguous()
    # row statistics of x in the producer's layout: [parts][M][2] = (mean, centred sum of squares) per column tile
    cnt = C // parts
    xp = x.float().view(M, parts, cnt).transpose(0, 1)
    mean_t = xp.mean(-1)
    st = torch.stack([mean_t, ((xp - mean_t[..., None]) ** 2).sum(-1)], dim=-1).contiguous()
    img = torch.empty(_lib.raw().dfh_mlp_fused_image_bytes(), dtype=torch.uint8, device=DEV)
    _lib.call("dfh_mlp_fused_pack", _lib.ptr(wf), _lib.ptr(s1), _lib.ptr(b1), _lib.ptr(w2p), _lib.ptr(img), form, gu.stream())
    out = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    # output statistics for a GroupNorm(32) consumer (form 2): images of 128 tokens -> one chunk each
    G, hw = 32, 128
    gst = torch.full((M // hw, G, hw // 128, 2), float("nan"), device=DEV) if form == 2 else None
    _lib.call("dfh_mlp_fused", _lib.ptr(x), _lib.ptr(resid), _lib.ptr(img), _lib.ptr(st), parts, cnt, 1e-5, _lib.ptr(bias), _lib.ptr(out), M, form,
              _lib.ptr(gst), C // G, hw, gu.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    if gst is not None:                       # sums of the ROUNDED outputs, fixed order: tight tolerance
        og = out.float().view(M // hw, hw, G, C // G)
        torch.testing.assert_close(gst[:, :, 0, 0], og.sum((1, 3)), rtol=1e-5, atol=1e-3)
        torch.testing.assert_close(gst[:, :, 0, 1], (og ** 2).sum((1, 3)), rtol=1e-5, atol=1e-3)
    # fp32 torch on the same operands
    ln = F.layer_norm(x.float(), (C,), gamma, beta, 1e-5)
    hh = ln @ bf(wg).float().T + bg
    av, gate = hh.chunk(2, -1)
    hid = bf(av * F.gelu(gate)).float()
    ref = torch.cat([hid, x.float()], dim=1) @ w2p.float().T + bias + resid.float()
    gu.assert_close_bf16(out, ref, "fused mlp vs torch")
    # the two-launch walk on the same operands
    dd = gu.gemm_desc(M=M, N=8 * C, W=wf, ldw=C, a0=x, a0_c=C, bias=b1, act=4)
    _lib.call("dfh_gemm_ln", ctypes.byref(dd), None, None, _lib.ptr(st), parts, cnt, 1e-5, _lib.ptr(s1), gu.stream())
    two = gu.gemm(M=M, N=C, W=w2p, ldw=5 * C, a0=dd.keep_out, a0_c=4 * C, a1=x, a1_c=C, bias=bias, resid=resid)
    torch.cuda.synchronize()
    assert gu.rel_err(out, two) < 6e-3, gu.rel_err(out, two)


@pytest.mark.parametrize("B,HW,C,pre", [(3, 4096, 320, False), (2, 1024, 640, False), (4, 256, 320, True), (2, 128, 64, False)])
def test_groupnorm_fold_into_projection_matches_torch(B, HW, C, pre):
    """dfh_groupnorm_fold + dfh_gemm(w_img_stride, rowvec): the transformer entry norm -> proj_in (difashion.py:249-253) without the
    normalised tensor -- per-image weights W . gamma . rstd, the mean / beta terms as a per-image row vector.  Against fp32 torch
    (group_norm -> linear on the same bf16 operands) and against the un-folded product path (dfh_groupnorm + dfh_gemm); channel means
    far from zero (the cancellation the rounded-weight mean term is there for).  pre: statistics handed over as producer partials."""
    import ctypes
    G = 32
    x = bf(rnd(B, HW, C, seed=91) * (1.0 + 2.0 * rnd(1, 1, C, seed=92).abs()) + 3.0 * rnd(1, 1, C, seed=93))
    gamma, beta = 1.0 + 0.3 * rnd(C, seed=94), 0.5 * rnd(C, seed=95)
    w, bias = bf(rnd(C, C, seed=96, scale=0.06)), rnd(C, seed=97, scale=0.3)
    ref = F.linear(F.group_norm(x.float().permute(0, 2, 1), G, gamma, beta, 1e-6).permute(0, 2, 1), w.float(), bias).reshape(B * HW, C)
    wimg = torch.empty(B, C, C, dtype=torch.bfloat16, device=DEV)
    rv = torch.empty(B, C, device=DEV)
    part = torch.zeros(B * 64 * G * 2, device=DEV)
    pre_t, chunks = None, 0
    if pre:                                    # [B][G][chunks][2] sums / sums of squares over 2 pixel chunks, as a producer epilogue leaves them
        chunks = 2
        xs = x.float().reshape(B, chunks, HW // chunks, G, C // G)
        pre_t = torch.stack([xs.sum((2, 4)), (xs * xs).sum((2, 4))], -1).permute(0, 2, 1, 3).contiguous()
    _lib.call("dfh_groupnorm_fold", _lib.ptr(x), B, HW, C, G, _lib.ptr(gamma), _lib.ptr(beta), 1e-6, _lib.ptr(pre_t) if pre else None, chunks,
              _lib.ptr(part), _lib.ptr(w), C, C, _lib.ptr(bias), _lib.ptr(wimg), _lib.ptr(rv), gu.stream())
    out = gu.gemm(M=B * HW, N=C, W=wimg, ldw=C, a0=x.reshape(B * HW, C), a0_c=C, rowvec=rv, rv_ld=C, rv_off=0, rows_per_b=HW, w_img_stride=C * C)
    torch.cuda.synchronize()
    gu.assert_close_bf16(out, ref, "GroupNorm folded into proj_in")
    # the un-folded product path on the same operands: the fold must not be the less accurate of the two by more than a rounding
    gn = torch.empty_like(x)
    _lib.call("dfh_groupnorm", _lib.ptr(x), C, None, 0, B, HW, G, _lib.ptr(gamma), _lib.ptr(beta), 1e-6, 0, _lib.ptr(gn), _lib.ptr(part), gu.stream())
    plain = gu.gemm(M=B * HW, N=C, W=w, ldw=C, a0=gn.reshape(B * HW, C), a0_c=C, bias=bias)
    torch.cuda.synchronize()
    assert gu.rel_err(out, ref) <= 1.5 * gu.rel_err(plain, ref) + 1e-3, (gu.rel_err(out, ref), gu.rel_err(plain, ref))


# ----------------------------------------------------------------------------- the plan is the launch
_PLAN_CASES = {   # kernel kind -> (shape, kernel, tile / wide variant, bm x bn, K slices): the smallest shapes at which the rules pick each kind
    "eight_wave_gstat128": (dict(M=256, K=64, N=320, gstat_hw=128), 0, 5, (128, 160), 1),
    "tile_128x64": (dict(M=128, K=64, N=8), 0, 2, (128, 64), 1),
    "ring_256x160_splitk": (dict(conv=(1, 16, 512), N=320), 0, 0, (256, 160), 4),
    "wide_256x160_gstat256": (dict(M=57344, K=64, N=320, resid=True, gstat_hw=4096), 3, 1, (256, 160), 1),
    "big_256x320": (dict(conv=(14, 64, 128), N=320, gstat_hw=4096), 1, 5, (256, 320), 1),
    "big_geglu_256x256": (dict(M=57344, K=64, N=256, act=4), 2, 4, (256, 256), 1),
    "wide_256x128": (dict(M=57344, K=64, N=256), 3, 4, (256, 128), 1),
    "batched_winograd": (dict(M=256, K=64, N=320, nbatch=16), 0, 5, (128, 160), 1),
    "deep_ring": (dict(M=4096, K=320, N=320), 0, 5, (128, 160), 1),
}


@pytest.mark.parametrize("kind", list(_PLAN_CASES))
def test_gemm_plan_is_the_launch_that_runs(kind):
    """dfh_gemm_plan (host code) against the launch itself, one shape per kernel kind of the product build: the statistics chunk rows /
    row-statistics column tile the entry point reports are the plan's, the census counter that rises is the plan's (plus splitk_reduce
    for a split plan), and the output matches the fp32 reference within this file's GEMM tolerance (assert_close_bf16)."""
    shape, kernel, sub, (bm, bn), split = _PLAN_CASES[kind]
    N, act, nb = shape["N"], shape.get("act", 0), shape.get("nbatch", 0)
    bias = rnd(N, seed=3)
    if "conv" in shape:
        B, H, Cin = shape["conv"]
        M = B * H * H
        x, w = bf(rnd(B, Cin, H, H, seed=1)), bf(rnd(N, Cin, 3, 3, seed=2, scale=0.05))
        kw = dict(M=M, N=N, W=gu.pack_conv(w.float()), ldw=9 * Cin, conv_src=gu.nhwc(x), conv_c=Cin, batch=B, Hin=H, Win=H, bias=bias)
        ref = gu.nhwc(F.conv2d(x.float(), w.float(), bias, padding=1)).view(M, N)
    else:
        M, K = shape["M"], shape["K"]
        a, w = bf(rnd(max(nb, 1), M, K, seed=1)), bf(rnd(max(nb, 1), N, K, seed=2, scale=0.05))
        res = bf(rnd(M, N, seed=4)) if shape.get("resid") else None
        kw = dict(M=M, N=N, W=w, ldw=K, a0=a, a0_c=K, bias=bias, resid=res, act=act)
        ref = a.float() @ w.float().transpose(1, 2) + bias + (res.float() if res is not None else 0)
    out = torch.empty(max(nb, 1), M, N // 2 if act == 4 else N, dtype=torch.bfloat16, device=DEV)
    d = gu.gemm_desc(out=out, ld_out=out.shape[-1], **kw)
    hw = shape.get("gstat_hw", 0)
    gst = torch.zeros(2 * (M // max(hw, 1)) * 32 * max(hw // 128, 1), dtype=torch.float32, device=DEV) if hw else None
    if hw:
        d.gstat, d.gstat_cpg, d.gstat_hw = gst.data_ptr(), N // 32, hw
    x_ = _lib.GemmPlanExtra(nbatch=nb, want_rowstat=0 if (hw or nb) else 1)
    info = _lib.GemmPlanInfo()
    _lib.call("dfh_gemm_plan", C.byref(d), C.byref(x_), C.byref(info))
    print(kind, info.line.decode())
    assert (info.kernel, info.wide if kernel == 3 else info.tile, info.bm, info.bn, info.split) == (kernel, sub, bm, bn, split)
    if kind in ("deep_ring", "batched_winograd", "eight_wave_gstat128"):
        assert info.stages == 4 and info.lean == 1          # at most 320 workgroups: the deep-ring eight-wave instantiation
    _lib.census_reset()
    if nb:
        _lib.call("dfh_gemm_batched", C.byref(d), nb, M * kw["a0_c"], N * kw["a0_c"], M * N, gu.stream())
        assert info.gstat_rows == 0 and info.rowstat_bn == 0
    elif hw:
        written = C.c_int(-1)
        _lib.call("dfh_gemm_gstat", C.byref(d), gu.stream(), C.byref(written))
        assert written.value == info.gstat_rows
    else:
        st = torch.zeros(2 * M * max(N // 64, 1) + 16, dtype=torch.float32, device=DEV)
        bn_ = C.c_int(-1)
        _lib.call("dfh_gemm_ln", C.byref(d), _lib.ptr(st), C.byref(bn_), None, 0, 0, 0.0, None, gu.stream())
        assert bn_.value == info.rowstat_bn
    torch.cuda.synchronize()
    census = {k: v for k, v in _lib.census().items() if v}
    want = {_lib.raw().dfh_census_name(info.census).decode(): 1}
    if info.split > 1:
        want["splitk_reduce"] = 1
    if info.gstat_rows:
        want["gstat_written"] = 1
    assert census == want
    if act == 4:      # packed GEGLU rows: 16-column blocks of values and gates alternate (dfh_pack_matrix's interleave)
        v, g = ref[0].view(M, N // 32, 2, 16).unbind(2)
        ref = (v * F.gelu(g)).reshape(1, M, N // 2)
    gu.assert_close_bf16(out, ref.view(out.shape), kind)
