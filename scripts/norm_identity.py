#!/usr/bin/env python3
"""Output identity of the normalisation kernels (csrc/norm.hip, norm_bwd.hip, the LayerNorm quantiser of gemm_fp8.hip, the GroupNorm
prologue of winograd.hip: everything that shares csrc/norm_steps.h) between two builds of the library (GPU only).

One process, one library (DFH_LIB chooses it, DFH_STORAGE its storage format): a fixed list of seeded cases goes through the public
entry points, and one line per case carries the SHA-256 of every output and the launch census of the case.  Run it with each build
and compare the two outputs:

  DFH_LIB=<other build> python scripts/norm_identity.py | grep -v '^#~' > a.txt;  python scripts/norm_identity.py | grep -v '^#~' > b.txt;  cmp a.txt b.txt
  python scripts/norm_identity.py --only layernorm          # the cases whose name contains the text

dgamma / dbeta of the backward kernels are sums of float atomics: not bit-stable between two runs of ONE library.  They are not
hashed; a line that starts with '#~' gives their largest difference from a float64 sum computed here, relative to the largest
|value| (informative: leave those lines out of the comparison).  An entry point the fp16-storage library refuses prints its refusal.

The shapes: every GroupNorm shape of tests/test_gpu_ops.py and tests/test_gpu_backward.py (the four forward paths, each gn_mid_kernel
instantiation, both orders of the chunk reduction, one chunk and 64), e4m3 output from the one-slab and the two-kernel path, the
fold with and without producer statistics, the fused Winograd prologue direct and chained, LayerNorm at C = 32 / 320 / 640 / 1280
with a ragged last row group, its e4m3 form and its backward with and without accumulation."""
import hashlib
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from difashion_amd import _lib

DEV = "cuda"
G = 32
P, S = _lib.ptr, _lib.stream_ptr


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed)) * scale).to(DEV)


def h16(t):
    return t.to(_lib.storage_dtype())


def empty16(*shape):
    return torch.empty(shape, dtype=_lib.storage_dtype(), device=DEV)


def gn_inputs(B, C0, C1, HW):
    x0 = h16(rnd(B, HW, C0, seed=31) * 2 + 0.7)
    x1 = h16(rnd(B, HW, C1, seed=32) - 0.4) if C1 else None
    C = C0 + C1
    return x0, x1, rnd(C, seed=33) * 0.3 + 1, rnd(C, seed=34) * 0.2, torch.empty(B * 64 * G * 2, device=DEV)


def groupnorm(B, C0, C1, HW, silu, eps):
    x0, x1, gamma, beta, part = gn_inputs(B, C0, C1, HW)
    out = empty16(B, HW, C0 + C1)
    _lib.call("dfh_groupnorm", P(x0), C0, P(x1), C1, B, HW, G, P(gamma), P(beta), eps, silu, P(out), P(part), S())
    return dict(out=out)


def producer_partials(x, B, HW, C, chunks):
    """[B][G][chunks][2] sums / sums of squares over pixel chunks, as a producing GEMM's epilogue leaves them"""
    xs = x.float().reshape(B, chunks, HW // chunks, G, C // G)
    return torch.stack([xs.sum((2, 4)), (xs * xs).sum((2, 4))], -1).permute(0, 2, 1, 3).contiguous()


def groupnorm_pre(B, C, HW, chunks, silu):
    x0, _, gamma, beta, _ = gn_inputs(B, C, 0, HW)
    out, stats = empty16(B, HW, C), torch.empty(B * G * 2, device=DEV)
    _lib.call("dfh_groupnorm_pre", P(x0), C, B, HW, G, P(gamma), P(beta), 1e-5, silu, P(out), P(producer_partials(x0, B, HW, C, chunks)), chunks,
              P(stats), S())
    return dict(out=out, stats=stats)


def groupnorm_fp8(B, HW, C):
    x0, _, _, _, part = gn_inputs(B, C, 0, HW)
    q = torch.empty(B, HW, C, dtype=torch.uint8, device=DEV)
    _lib.call("dfh_groupnorm_fp8", P(x0), B, HW, C, G, 1e-6, 448.0 / 32.0, P(q), P(part), S())
    return dict(q=q)


def groupnorm_fold(B, HW, C, pre):
    x = h16(rnd(B, HW, C, seed=91) * (1.0 + 2.0 * rnd(1, 1, C, seed=92).abs()) + 3.0 * rnd(1, 1, C, seed=93))
    gamma, beta = 1.0 + 0.3 * rnd(C, seed=94), 0.5 * rnd(C, seed=95)
    w, bias = h16(rnd(C, C, seed=96, scale=0.06)), rnd(C, seed=97, scale=0.3)
    wimg, rv, part = empty16(B, C, C), torch.empty(B, C, device=DEV), torch.zeros(B * 64 * G * 2, device=DEV)
    pre_t = producer_partials(x, B, HW, C, 2) if pre else None
    _lib.call("dfh_groupnorm_fold", P(x), B, HW, C, G, P(gamma), P(beta), 1e-6, P(pre_t), 2 if pre else 0, P(part), P(w), C, C, P(bias), P(wimg),
              P(rv), S())
    return dict(wimg=wimg, rv=rv)


def rel_to_f64(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def groupnorm_bwd(B, C0, C1, HW, silu, eps):
    x0, x1, gamma, beta, part = gn_inputs(B, C0, C1, HW)
    C = C0 + C1
    dy = h16(rnd(B, HW, C, seed=35))
    out, stats = empty16(B, HW, C), torch.empty(B * G * 2, device=DEV)
    _lib.call("dfh_groupnorm_stats", P(x0), C0, P(x1), C1, B, HW, G, P(gamma), P(beta), eps, silu, P(out), P(part), P(stats), S())
    dx0, dx1 = h16(rnd(B, HW, C0, seed=36)), (empty16(B, HW, C1) if C1 else None)       # dx0 accumulates into existing contents
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    _lib.call("dfh_groupnorm_bwd", P(x0), C0, P(x1), C1, P(dy), B, HW, G, P(gamma), P(beta), P(stats), silu, P(dx0), 1, P(dx1), 0, P(dg), P(db),
              P(part), S())
    torch.cuda.synchronize()
    x = (torch.cat([x0, x1], -1) if C1 else x0).double()
    st = stats.double().view(B, G, 2).repeat_interleave(C // G, 1)                       # [B][C][2] (mean, rstd) as the kernels read them
    xh = (x - st[:, None, :, 0]) * st[:, None, :, 1]
    dz = dy.double()
    if silu:
        z = gamma.double() * xh + beta.double()
        sg = torch.sigmoid(z)
        dz = dz * sg * (1 + z * (1 - sg))
    note = f"dgamma {rel_to_f64(dg, (dz * xh).sum((0, 1))):.1e} dbeta {rel_to_f64(db, dz.sum((0, 1))):.1e}"
    return dict(stats=stats, dx0=dx0, **({"dx1": dx1} if C1 else {})), note


def gn_wino(B, C0, C1, H, W):
    x0 = h16(rnd(B, H, W, C0, seed=40))
    x1 = h16(rnd(B, H, W, C1, seed=41, scale=2.0)) if C1 else None
    C = C0 + C1
    gamma, beta = 1.0 + 0.1 * rnd(C, seed=42), 0.1 * rnd(C, seed=43)
    V = empty16(16, B * (H // 2) * (W // 2), C)
    _lib.call("dfh_gn_wino_input", P(x0), C0, P(x1), C1, P(gamma), P(beta), 1e-5, G, P(V), B, H, W, S())
    return dict(V=V)


def gn_wino_chain(B, C, H, W, temb):
    mt = B * (H // 2) * (W // 2)
    Mp, bias = h16(rnd(16, mt, C, seed=70)), rnd(C, seed=71)
    rv = rnd(B, 2 * C, seed=72) if temb else None
    gamma, beta = 1.0 + 0.1 * rnd(C, seed=73), 0.1 * rnd(C, seed=74)
    V = empty16(16, mt, C)
    _lib.call("dfh_gn_wino_input_chain", P(Mp), P(bias), P(rv), 2 * C if temb else 0, C if temb else 0, C, P(gamma), P(beta), 1e-5, G, P(V),
              B, H, W, S())
    return dict(V=V)


def ln_inputs(M, C):
    return h16(rnd(M, C, seed=35) * 3 + 1.5), rnd(C, seed=36) * 0.3 + 1, rnd(C, seed=37) * 0.2


def layernorm(M, C):
    x, gamma, beta = ln_inputs(M, C)
    y = torch.empty_like(x)
    _lib.call("dfh_layernorm", P(x), P(gamma), P(beta), P(y), M, C, 1e-5, S())
    return dict(y=y)


def layernorm_fp8(M, C):
    x, gamma, beta = ln_inputs(M, C)
    q, scale = torch.empty(M, C, dtype=torch.uint8, device=DEV), torch.empty(M, device=DEV)
    _lib.call("dfh_layernorm_fp8", P(x), P(gamma), P(beta), P(q), P(scale), M, C, 1e-5, S())
    return dict(q=q, scale=scale)


def layernorm_bwd(M, C, acc):
    x, gamma, _ = ln_inputs(M, C)
    dy = h16(rnd(M, C, seed=38))
    dx = h16(rnd(M, C, seed=39)) if acc else torch.empty_like(x)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    _lib.call("dfh_layernorm_bwd", P(x), P(dy), P(gamma), P(dx), acc, P(dg), P(db), M, C, 1e-5, S())
    torch.cuda.synchronize()
    xd = x.double()
    xh = (xd - xd.mean(1, keepdim=True)) * torch.rsqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-5)
    return dict(dx=dx), f"dgamma {rel_to_f64(dg, (dy.double() * xh).sum(0)):.1e} dbeta {rel_to_f64(db, dy.double().sum(0)):.1e}"


GN_FWD = [(3, 320, 0, 256, 1, 1e-5), (3, 640, 320, 64, 1, 1e-5), (3, 1280, 1280, 16, 1, 1e-5), (3, 64, 0, 4, 0, 1e-6), (3, 32, 32, 256, 1, 1e-5),
          (3, 1280, 640, 64, 0, 1e-6), (8, 264, 248, 16, 1, 1e-5), (8, 264, 248, 256, 1, 1e-5), (8, 1280, 640, 256, 1, 1e-5),
          (8, 1280, 1280, 256, 1, 1e-5), (16, 1280, 640, 64, 1, 1e-5), (2, 320, 0, 4096, 1, 1e-5), (16, 640, 0, 64, 1, 1e-5)]
GN_BWD = [(3, 320, 0, 256, 1, 1e-5), (3, 640, 320, 64, 1, 1e-5), (3, 64, 0, 4, 0, 1e-6), (3, 32, 32, 256, 1, 1e-5), (3, 1280, 640, 64, 0, 1e-6),
          (3, 1280, 768, 1, 1, 1e-5), (2, 320, 0, 4096, 1, 1e-5)]
CASES = (
    [(f"groupnorm dfh_groupnorm {s}", lambda s=s: groupnorm(*s)) for s in GN_FWD]
    + [(f"groupnorm dfh_groupnorm_pre {s}", lambda s=s: groupnorm_pre(*s)) for s in ((4, 320, 256, 2, 1), (2, 640, 1024, 8, 0), (2, 320, 4096, 32, 1))]
    + [(f"groupnorm dfh_groupnorm_fp8 {s}", lambda s=s: groupnorm_fp8(*s)) for s in ((2, 4096, 320), (3, 1024, 640), (4, 256, 1280), (16, 64, 1280), (2, 16, 64))]
    + [(f"groupnorm dfh_groupnorm_fold {s}", lambda s=s: groupnorm_fold(*s))
       for s in ((3, 4096, 320, False), (2, 1024, 640, False), (4, 256, 320, True), (2, 128, 64, False))]
    + [(f"groupnorm dfh_groupnorm_stats + dfh_groupnorm_bwd {s}", lambda s=s: groupnorm_bwd(*s)) for s in GN_BWD]
    + [(f"winograd dfh_gn_wino_input {s}", lambda s=s: gn_wino(*s))
       for s in ((2, 1280, 0, 16, 16), (3, 1280, 640, 8, 8), (2, 640, 0, 16, 16), (16, 1280, 1280, 8, 8), (2, 128, 128, 4, 6))]
    + [(f"winograd dfh_gn_wino_input_chain {s}", lambda s=s: gn_wino_chain(*s))
       for s in ((2, 1280, 16, 16, True), (16, 1280, 8, 8, True), (3, 640, 8, 8, False), (2, 128, 4, 6, True))]
    # M = 1030: a million elements, so that one fp32 rounding that differs per element shows in the 16-bit output (about one flip in 2^15)
    + [(f"layernorm dfh_layernorm {s}", lambda s=s: layernorm(*s))
       for s in ((37, 32), (37, 320), (301, 320), (37, 640), (131, 640), (37, 1280), (1030, 320), (1030, 640), (1030, 1280))]
    + [(f"layernorm dfh_layernorm_fp8 {s}", lambda s=s: layernorm_fp8(*s))
       for s in ((37, 32), (37, 320), (301, 320), (37, 640), (37, 1280), (1030, 320), (1030, 640), (1030, 1280))]
    + [(f"layernorm dfh_layernorm_bwd {s}", lambda s=s: layernorm_bwd(*s))
       for s in ((37, 32, 0), (130, 320, 0), (130, 320, 1), (130, 640, 0), (130, 640, 1), (70, 1280, 0), (70, 1280, 1), (1030, 320, 0), (1030, 640, 0),
                 (1030, 1280, 0), (1030, 1280, 1))]
)


if __name__ == "__main__":
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    torch.set_grad_enabled(False)
    print(f"# storage={_lib.storage()}", flush=True)
    for name, run in CASES:
        if only not in name:
            continue
        _lib.census_reset()
        try:
            outs = run()
        except _lib.DfhError as e:
            if "refused" not in str(e):
                raise
            print(f"{name:72s} refused by the {_lib.storage()}-storage library", flush=True)
            continue
        outs, note = outs if isinstance(outs, tuple) else (outs, None)
        torch.cuda.synchronize()
        finite = all(bool(torch.isfinite(v.float()).all()) for v in outs.values() if v.dtype != torch.uint8)
        census = " ".join(f"{k}={v}" for k, v in _lib.census().items() if v)
        print(f"{name:72s} " + " ".join(f"{k} {sha(v)}" for k, v in outs.items()) + f" | {census}" + ("" if finite else " NOT-FINITE"), flush=True)
        if note:
            print(f"#~ {name}: {note}", flush=True)
