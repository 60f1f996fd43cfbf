#!/usr/bin/env python3
"""The optimizer launch with fp32 and with 8-bit states, side by side on one MI355X: recorded, not gated.  One JSON line to
profiles/adamw8_bench.json.

Both launches update the same n elements with the EMA shadow folded in, n = the aligned parameter count of the SD-1.5 U-Net (every
parameter rounded up to the 64-element granule of the flat buffers):
  * dfh_adamw_ema: fp32 exp_avg / exp_avg_sq, 36 B per element (p r+w, g r, m r+w, v r+w, shadow r+w);
  * dfh_adamw8 with a shadow: one code byte per moment and one fp32 absmax per 64 elements and moment, 24.25 B per element.
The two alternate in one process, window by window (same card, same clocks, same neighbours): after a warm-up each window is at least
ten launches between two device events; the figure is the median of the windows, the spread is kept.  The byte floor of the 8-bit launch
is 24.25 / 36 = 0.674 of the fp32 one.

    python scripts/bench_adamw8.py [--out profiles/adamw8_bench.json] [--windows 7] [--launches 10] [--n ELEMENTS]
"""
import argparse
import ctypes as C
import os

import torch
from _rowbench import ROOT, emit, header, spread

from difashion_amd import _lib  # noqa: E402
from difashion_amd.training import _align  # noqa: E402

BYTES_FP32, BYTES_Q8 = 36.0, 24.25


def sd15_aligned_elements() -> int:
    """Sum over the SD-1.5 U-Net's parameters (the library's own table; host only) of the count rounded up to 64."""
    c = _lib.UNetConfigC()
    c.sample_size, c.in_channels, c.out_channels, c.num_blocks = 64, 8, 4, 4
    for i, (ch, heads, attn) in enumerate(zip((320, 640, 1280, 1280), (8, 8, 8, 8), (1, 1, 1, 0))):
        c.block_out_channels[i], c.num_heads[i], c.down_attn[i] = ch, heads, attn
    c.layers_per_block, c.cross_attention_dim = 2, 768
    c.use_linear_projection, c.norm_num_groups, c.norm_eps, c.text_len = 0, 32, 1e-5, 77
    h = C.c_void_p()
    _lib.call("dfh_unet_create", C.byref(c), C.byref(h))
    lib = _lib.raw()
    try:
        total = 0
        for i in range(lib.dfh_unet_num_params(h)):
            numel = 1
            for d in range(lib.dfh_unet_param_ndim(h, i)):
                numel *= lib.dfh_unet_param_dim(h, i, d)
            total += _align(numel)
        return total
    finally:
        lib.dfh_unet_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw8_bench.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--n", type=int, default=0, help="elements (a multiple of 64); default: the SD-1.5 U-Net's aligned parameter count")
    a = ap.parse_args()
    assert a.windows >= 5 and a.launches >= 10, "at least five windows of at least ten launches"
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    n = a.n or sd15_aligned_elements()
    assert n % 64 == 0
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda scale: torch.randn(n, generator=g, device="cuda") * scale
    # per-block gradient scales over a few decades, as the layers of a network have: the codes then spread over the tables
    grad = rn(1.0) * torch.exp(2.0 * torch.randn(n // 64, generator=g, device="cuda")).repeat_interleave(64) * 1e-3
    sumsq = torch.zeros(1, device="cuda")
    _lib.call("dfh_sumsq", _lib.ptr(grad), n, _lib.ptr(sumsq), _lib.stream_ptr())
    # each launch owns its parameters, shadow and states; the gradient and the clip norm are shared (read only)
    p32, sh32, m, v = rn(0.05), rn(0.05), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    p8, sh8 = p32.clone(), sh32.clone()
    c1, c2 = torch.full((n,), 127, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    a1, a2 = torch.zeros(n // 64, device="cuda"), torch.zeros(n // 64, device="cuda")
    hyper = (1e-4, 0.9, 0.999, 1e-8, 1e-2)
    step = [0]

    def fp32_launch():
        _lib.call("dfh_adamw_ema", _lib.ptr(p32), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), _lib.ptr(sh32), n, *hyper, step[0], _lib.ptr(sumsq),
                  1.0, 0.9999, _lib.stream_ptr())

    def q8_launch():
        _lib.call("dfh_adamw8", _lib.ptr(p8), _lib.ptr(grad), _lib.ptr(c1), _lib.ptr(a1), _lib.ptr(c2), _lib.ptr(a2), _lib.ptr(sh8), n, *hyper,
                  step[0], _lib.ptr(sumsq), 1.0, 0.9999, _lib.stream_ptr())

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn):
        e0.record()
        for _ in range(a.launches):
            step[0] += 1
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.launches

    for fn in (fp32_launch, q8_launch, fp32_launch, q8_launch):          # warm-up: two windows each
        window(fn)
    per32, per8 = [], []
    for _ in range(a.windows):                                            # alternating
        per32.append(window(fp32_launch))
        per8.append(window(q8_launch))
    t32, t8 = spread(per32), spread(per8)
    assert bool(torch.isfinite(p32).all()) and bool(torch.isfinite(p8).all())
    res = dict(**header(card=True), elements=n, windows=a.windows, launches_per_window=a.launches,
               adamw_ema_fp32=dict(bytes_per_element=BYTES_FP32, tb_per_s=round(BYTES_FP32 * n / (t32["ms"] * 1e-3) / 1e12, 3), **t32),
               adamw8_ema=dict(bytes_per_element=BYTES_Q8, tb_per_s=round(BYTES_Q8 * n / (t8["ms"] * 1e-3) / 1e12, 3), **t8),
               ratio_q8_over_fp32=round(t8["ms"] / t32["ms"], 4), byte_floor_ratio=round(BYTES_Q8 / BYTES_FP32, 4),
               state_gb=dict(fp32=round(8.0 * n / 1e9, 3), q8=round((2.0 + 8.0 / 64) * n / 1e9, 3)))
    emit(res, a.out)


if __name__ == "__main__":
    main()
