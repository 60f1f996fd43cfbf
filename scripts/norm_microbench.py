#!/usr/bin/env python3
"""The normalisation kernels on the U-Net's shapes at batch 16: time and effective HBM GB/s (algorithmic bytes: every tensor read and
written once).  Legs: dfh_groupnorm (+SiLU), dfh_groupnorm_bwd, dfh_groupnorm_fp8, dfh_groupnorm_fold, dfh_layernorm, dfh_layernorm_fp8,
dfh_layernorm_bwd.  One process, one library: DFH_LIB=<other build> times that build (an A/B alternates the two in separate runs).

  python scripts/norm_microbench.py [--only <text in the leg's name>] [--iters N]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from difashion_amd import _lib

DEV = "cuda"
B, G = 16, 32
P = _lib.ptr
ITERS = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""


def timeit(fn, iters=ITERS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def report(name, fn, nbytes):
    if ONLY in name:
        us = timeit(fn)
        print(f"{name}: {us:7.1f} us  {nbytes / us / 1e3:7.1f} GB/s", flush=True)


def h16(*shape):
    return torch.randn(*shape, device=DEV).to(_lib.storage_dtype())


# (H, C0, C1): every GroupNorm of the U-Net (resnet norm1 / norm2 incl. the up path's concatenated inputs); (H, C): its transformer levels
RESNET = ((64, 320, 0), (64, 320, 320), (64, 640, 320), (32, 320, 0), (32, 640, 0), (32, 640, 320), (32, 640, 640), (32, 1280, 640), (16, 640, 0),
          (16, 1280, 0), (16, 1280, 640), (16, 1280, 1280), (8, 1280, 0), (8, 1280, 1280))
TOKENS = ((64, 320), (32, 640), (16, 1280), (8, 1280))
FP16 = _lib.storage() == "fp16"             # the fp16-storage library is inference only: no backward, no e4m3 legs

print(f"# {_lib.LIB_PATH} storage={_lib.storage()} batch {B}, {ITERS} launches a figure", flush=True)
s = _lib.stream_ptr()
part = torch.empty(B * 64 * G * 2, device=DEV)
for H, C0, C1 in RESNET:
    HW, C = H * H, C0 + C1
    x0, x1 = h16(B, HW, C0), (h16(B, HW, C1) if C1 else None)
    g, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    out = torch.empty(B, HW, C, device=DEV, dtype=_lib.storage_dtype())
    report(f"groupnorm+silu {H}x{H} C={C0}+{C1}", lambda: _lib.call("dfh_groupnorm", P(x0), C0, P(x1), C1, B, HW, G, P(g), P(b), 1e-5, 1, P(out), P(part), s),
           4.0 * B * HW * C)
    if FP16:
        continue
    stats = torch.empty(B * G * 2, device=DEV)
    _lib.call("dfh_groupnorm_stats", P(x0), C0, P(x1), C1, B, HW, G, P(g), P(b), 1e-5, 1, P(out), P(part), P(stats), s)
    dy, dx0, dx1 = h16(B, HW, C), torch.empty_like(x0), (torch.empty_like(x1) if C1 else None)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    report(f"groupnorm_bwd+silu {H}x{H} C={C0}+{C1}", lambda: _lib.call("dfh_groupnorm_bwd", P(x0), C0, P(x1), C1, P(dy), B, HW, G, P(g), P(b), P(stats), 1,
                                                                       P(dx0), 0, P(dx1), 0, P(dg), P(db), P(part), s), 10.0 * B * HW * C)
    del dy, dx0, dx1
for H, C in TOKENS:
    HW, M = H * H, B * H * H
    x = h16(B, HW, C)
    g, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    y = torch.empty_like(x)
    report(f"layernorm {H}x{H} C={C}", lambda: _lib.call("dfh_layernorm", P(x), P(g), P(b), P(y), M, C, 1e-5, s), 4.0 * M * C)
    w, bias = h16(C, C), torch.zeros(C, device=DEV)
    wimg, rv = torch.empty(B, C, C, device=DEV, dtype=_lib.storage_dtype()), torch.empty(B, C, device=DEV)
    report(f"groupnorm_fold {H}x{H} C={C}", lambda: _lib.call("dfh_groupnorm_fold", P(x), B, HW, C, G, P(g), P(b), 1e-6, None, 0, P(part), P(w), C, C, P(bias),
                                                             P(wimg), P(rv), s), 2.0 * M * C + 2.0 * C * C * (1 + B))
    if FP16:
        continue
    q, scale = torch.empty(M, C, dtype=torch.uint8, device=DEV), torch.empty(M, device=DEV)
    report(f"layernorm_fp8 {H}x{H} C={C}", lambda: _lib.call("dfh_layernorm_fp8", P(x), P(g), P(b), P(q), P(scale), M, C, 1e-5, s), 3.0 * M * C)
    report(f"groupnorm_fp8 {H}x{H} C={C}", lambda: _lib.call("dfh_groupnorm_fp8", P(x), B, HW, C, G, 1e-6, 14.0, P(q), P(part), s), 3.0 * M * C)
    dy, dx = h16(B, HW, C), torch.empty_like(x)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    report(f"layernorm_bwd {H}x{H} C={C}", lambda: _lib.call("dfh_layernorm_bwd", P(x), P(dy), P(g), P(dx), 0, P(dg), P(db), M, C, 1e-5, s), 6.0 * M * C)
