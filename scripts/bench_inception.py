#!/usr/bin/env python3
"""Throughput of DESIGN.md row f9 (Inception v3 for FID / IS), reported and not gated: one JSON line to profiles/inception_bench.json.

  * the feature extractor (``FIDInceptionV3((3,))``) on a batch of 50 images of 512 x 512: device-event ms per batch, images/s, and the
    batch's convolution flops (from the library's own launch plan, the first layer counted with its three real channels) over that time
    against the 157.3 TFLOP/s fp32 matrix peak -- an end-to-end rate, not a kernel's share;
  * the convolution launches of that batch alone: the library's per-launch events (dfh_prof_begin / dfh_prof_end) around the whole walk
    give their summed time, and so the conv kernel's own share of the peak over the network;
  * every distinct convolution geometry of the plan on its own at batch 50 (dfh_incep_conv_bn_relu between the events; the weight pack of
    that entry point is outside them): ms, TFLOP/s, share of the peak, grouped as square / 1 x 7 and 7 x 1 / strided / 1 x 1.

Every case is warmed up twice; the figure is the median of five windows and the spread (min .. max) is kept.  The kernels' time does
not depend on the values.

    python scripts/bench_inception.py [--out profiles/inception_bench.json] [--batch 50] [--size 512]
"""
import argparse
import ctypes as C
import os

import torch
from _rowbench import ROOT, emit, header, spread, timed

import difashion_amd as da  # noqa: E402
from difashion_amd import _lib  # noqa: E402
from difashion_amd import inception as I  # noqa: E402

PEAK_TFLOPS = 157.3
K_CONV = 1


def conv_flops(e, n):
    cin = 3 if e.Cin == 4 else e.Cin
    return 2.0 * n * e.Hout * e.Wout * e.KH * e.KW * cin * e.Cout


def group_of(e):
    if e.stride == 2:
        return "strided"
    if e.KH != e.KW:
        return "1x7_7x1_1x3_3x1"
    return "1x1" if e.KH == 1 else "square"


def conv_case(e, n, g, windows=5, min_window_ms=50.0):
    """One convolution launch of the plan on its own: ms from the library's per-launch events."""
    x = torch.randn((n, e.Hin, e.Win, e.Cin), generator=g, device="cuda")
    wt = torch.randn((e.Cout, e.Cin, e.KH, e.KW), generator=g, device="cuda") * (2.0 / (e.KH * e.KW * e.Cin)) ** 0.5
    bn = [torch.ones(e.Cout, device="cuda"), torch.zeros(e.Cout, device="cuda"), torch.zeros(e.Cout, device="cuda"), torch.ones(e.Cout, device="cuda")]
    arr = (C.c_void_p * 4)(*[t.data_ptr() for t in bn])
    packed = torch.empty(e.Cout * (e.KH * e.KW * e.Cin + 2), device="cuda")
    out = torch.empty((n, e.Hout, e.Wout, e.Cout), device="cuda")
    run = lambda: _lib.call("dfh_incep_conv_bn_relu", _lib.ptr(x), _lib.ptr(wt), e.Cin, arr, _lib.ptr(packed), _lib.ptr(out), n, e.Hin, e.Win, e.Cin,
                            e.Cout, e.KH, e.KW, e.stride, e.padH, e.padW, e.Cout, 0, _lib.stream_ptr())

    def window(reps):
        _lib.prof_begin()
        for _ in range(reps):
            run()
        rec = _lib.prof_end()["gemm_conv3x3"]
        assert rec["launches"] == reps
        return rec["ms"] / reps

    run(); run()
    torch.cuda.synchronize()
    reps = max(1, min(200, int(min_window_ms / max(window(1), 1e-3)) + 1))
    t = spread([window(reps) for _ in range(windows)])
    flops = conv_flops(e, n)
    tf = flops / (t["ms"] * 1e-3) / 1e12
    return dict(layer=e.name.decode(), group=group_of(e), C_in=e.Cin, C_out=e.Cout, k=[e.KH, e.KW], stride=e.stride, H=e.Hin, W=e.Win, gflop=round(flops / 1e9, 3),
                tflops=round(tf, 2), fraction_of_fp32_matrix_peak=round(tf / PEAK_TFLOPS, 4), launches_per_window=reps, **t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inception_bench.json"))
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    g = torch.Generator(device="cuda").manual_seed(0)
    res = dict(**header(card=True), peak_fp32_matrix_tflops=PEAK_TFLOPS, batch=a.batch, source_size=a.size)
    model = da.FIDInceptionV3((3,)).to("cuda")
    x = torch.rand((a.batch, 3, a.size, a.size), generator=g, device="cuda")
    assert model.images_per_call(a.size, a.size) >= a.batch
    plan = I.plan(model._context(), a.batch, a.size, a.size)
    convs = [e for e in plan if e.kind == K_CONV]
    flops = sum(conv_flops(e, a.batch) for e in convs)
    t = timed(lambda: model(x))
    res["extractor"] = dict(ms_per_batch=t["ms"], images_per_s=round(a.batch / t["ms"] * 1e3, 1), conv_gflop_per_batch=round(flops / 1e9, 2),
                            launches=len(plan), end_to_end_fraction_of_fp32_matrix_peak=round(flops / (t["ms"] * 1e-3) / 1e12 / PEAK_TFLOPS, 4), **t)
    per = []
    for _ in range(5):
        _lib.prof_begin()
        model(x)
        rec = _lib.prof_end()["gemm_conv3x3"]
        assert rec["launches"] == len(convs)
        per.append(rec["ms"])
    s = spread(per)
    res["conv_launches_of_the_walk"] = dict(launches=len(convs), fraction_of_fp32_matrix_peak=round(flops / (s["ms"] * 1e-3) / 1e12 / PEAK_TFLOPS, 4), **s)
    seen, layers = set(), []
    for e in convs:
        key = (e.Hin, e.Win, e.Cin, e.Cout, e.KH, e.KW, e.stride, e.padH, e.padW)
        if key in seen:
            continue
        seen.add(key)
        layers.append(conv_case(e, a.batch, g))
    res["layers"] = layers
    groups = {}
    for L in layers:
        groups.setdefault(L["group"], []).append(L)
    res["groups"] = {k: dict(layers=len(v), gflop=round(sum(L["gflop"] for L in v), 2), ms=round(sum(L["ms"] for L in v), 4),
                             fraction_of_fp32_matrix_peak=round(sum(L["gflop"] for L in v) / sum(L["ms"] for L in v) / PEAK_TFLOPS, 4),      # GFLOP / ms = TFLOP/s
                             best=max(L["fraction_of_fp32_matrix_peak"] for L in v), worst=min(L["fraction_of_fp32_matrix_peak"] for L in v))
                     for k, v in groups.items()}
    emit(res, a.out)


if __name__ == "__main__":
    main()
