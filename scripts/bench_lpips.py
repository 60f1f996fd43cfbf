#!/usr/bin/env python3
"""Throughput of DESIGN.md row f8 (LPIPS on VGG16), reported and not gated: one JSON line to profiles/lpips_bench.json.

  * each of the thirteen convolutions on the two images of one pair at 512^2 and 1024^2: the time of the conv launch alone (the
    library's per-launch events, dfh_prof_begin / dfh_prof_end, around dfh_lpips_conv3x3_relu; the weight pack of that entry point is
    outside the events) and its TFLOP/s against the 157.3 TFLOP/s fp32 matrix peak;
  * a whole pair through LPIPS.forward at 1024^2 (one pair a call, and three, what a 4 GiB workspace takes) and at 512^2 (one, and
    fifteen), device-event ms per pair against the flop floor: 305 856 MAC a pixel x 2 images at the peak = 8.2 ms / 2.0 ms.

Every case is warmed up twice; the figure is the median of five windows and the spread (min .. max) is kept.  The kernels' time does
not depend on the values.

    python scripts/bench_lpips.py [--out profiles/lpips_bench.json] [--sizes 512 1024]
"""
import argparse
import os

import torch
from _rowbench import ROOT, emit, header, spread

import difashion_amd as da  # noqa: E402
from difashion_amd import _lib  # noqa: E402

PEAK_TFLOPS = 157.3
MAC_PER_PIXEL = 305_856
# (C_in as the kernel sees it, C_out, level) of the thirteen convs
CONVS = [(4, 64, 0), (64, 64, 0), (64, 128, 1), (128, 128, 1), (128, 256, 2), (256, 256, 2), (256, 256, 2), (256, 512, 3), (512, 512, 3),
         (512, 512, 3), (512, 512, 4), (512, 512, 4), (512, 512, 4)]
NAMES = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2", "conv5_3"]


def conv_case(cin, cout, h, w, g, windows=5, min_window_ms=50.0):
    """The conv launch alone on 2 images of h x w: ms from the library's own per-launch events."""
    x = torch.randn((2, h, w, cin), generator=g, device="cuda")
    wt = torch.randn((cout, cin, 3, 3), generator=g, device="cuda") * (2.0 / (9 * cin)) ** 0.5
    bias = torch.zeros((cout,), device="cuda")
    packed = torch.empty(9 * cin * cout, device="cuda")
    out = torch.empty((2, h, w, cout), device="cuda")
    run = lambda: _lib.call("dfh_lpips_conv3x3_relu", _lib.ptr(x), _lib.ptr(wt), cin, _lib.ptr(bias), _lib.ptr(packed), _lib.ptr(out), 2, h, w,
                            cin, cout, _lib.stream_ptr())

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
    flops = 2.0 * 2 * h * w * 9 * (3 if cin == 4 else cin) * cout          # the algorithm's: the first layer has 3 input channels
    tf = flops / (t["ms"] * 1e-3) / 1e12
    return dict(C_in=cin, C_out=cout, H=h, W=w, gflop=round(flops / 1e9, 3), tflops=round(tf, 2), fraction_of_fp32_matrix_peak=round(tf / PEAK_TFLOPS, 4),
                launches_per_window=reps, **t)


def pair_case(model, pairs, size, g, windows=5):
    a = torch.rand((pairs, 3, size, size), generator=g, device="cuda") * 2 - 1
    b = torch.rand((pairs, 3, size, size), generator=g, device="cuda") * 2 - 1
    model(a, b); model(a, b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(windows):
        e0.record(); model(a, b); e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / pairs)
    floor_ms = 2.0 * MAC_PER_PIXEL * 2 * size * size / (PEAK_TFLOPS * 1e12) * 1e3
    t = spread(per)
    return dict(pairs_per_call=pairs, size=size, ms_per_pair=t["ms"], flop_floor_ms=round(floor_ms, 3), fraction_of_flop_floor=round(floor_ms / t["ms"], 4),
                pairs_per_s=round(1e3 / t["ms"], 2), **t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    g = torch.Generator(device="cuda").manual_seed(0)
    res = dict(**header(card=True), peak_fp32_matrix_tflops=PEAK_TFLOPS)
    model = da.LPIPS().to("cuda")
    for size in a.sizes:
        convs = {}
        for name, (cin, cout, level) in zip(NAMES, CONVS):
            convs[name] = conv_case(cin, cout, size >> level, size >> level, g)
        res[f"convs_{size}"] = convs
        res[f"convs_{size}_sum_ms"] = round(sum(c["ms"] for c in convs.values()), 4)
        many = model.pairs_per_call(size, size)
        res[f"pair_{size}"] = [pair_case(model, 1, size, g), pair_case(model, many, size, g)]
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
