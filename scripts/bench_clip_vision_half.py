#!/usr/bin/env python3
"""fp32 beside 16-bit: ``encode_image`` of the HIP CLIP image encoder over 200 images at ViT-H/14 and
at ViT-L/14, reported and not gated: one JSON line to profiles/clip_vision_half_bench.json.

  * this process (bf16 storage) times the fp32 tower and the bf16 tower of ONE model object, alternating inside every window, so
    that both see the same box in the same minutes; a child process under ``DFH_STORAGE=fp16`` does the same for fp32 beside fp16.
    The fp32 tower's kernels are the parent commit's, so its time in the same run is the baseline;
  * device events around the 200 images (batches of --batch), after a warm-up pass of every mode; the figure is the median of
    five windows and the spread (min .. max) is kept;
  * per launch class (linears, attention, LayerNorm, split-K reduce, everything else) from a separately profiled batch
    (dfh_prof_begin / dfh_prof_end bracket every launch with events: not the timed run);
  * achieved TFLOP/s = the algorithm's multiply-adds x 2 over the time: an end-to-end rate, not a kernel's share of a peak.

    python scripts/bench_clip_vision_half.py [--images 200] [--batch 50] [--models vit_h_14,vit_l_14] [--out profiles/clip_vision_half_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import torch
from _rowbench import ROOT, emit, header, randomise, spread
from bench_clip_vision import MODELS, flops_per_image

import difashion_amd as da  # noqa: E402
from difashion_amd import _lib  # noqa: E402

CLASSES = {"gemm_linear": "linears", "attention": "attention", "layernorm": "layernorm", "splitk_reduce": "splitk_reduce", "other": "other"}


def bench_model(name, images, batch, windows=5):
    cfg = MODELS[name]
    own = _lib.storage_dtype()
    modes = {"fp32": torch.float32, _lib.storage(): own}
    m = da.CLIPVisionModelWithProjection(**cfg, init_seed=None).to("cuda").eval().requires_grad_(False)
    g = torch.Generator(device="cuda").manual_seed(0)
    randomise(m, g)                                          # the speed does not depend on the values; parity is tests/test_gpu_clip_vision_half.py
    n_batches = max(1, images // batch)
    px = torch.randn(n_batches, batch, 3, cfg["image_size"], cfg["image_size"], generator=g, device="cuda")

    def run(dtype):
        m.set_compute_dtype(dtype)
        for i in range(n_batches):
            emb = m.encode_image(px[i])
        return emb

    for dtype in modes.values():                             # warm-up: workspaces, the packed copy, code-object load
        assert torch.isfinite(run(dtype)).all()
    torch.cuda.synchronize()
    per = {k: [] for k in modes}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(windows):
        for k, dtype in modes.items():                       # alternating: fp32, 16-bit, fp32, ...
            torch.cuda.synchronize()                         # (the mode switch inside run() costs nothing: the packed copy is kept across it)
            a.record()
            run(dtype)
            b.record()
            torch.cuda.synchronize()
            per[k].append(a.elapsed_time(b))
    lin, att, emb_f = flops_per_image(cfg)
    flops = (lin + att + emb_f) * batch * n_batches
    res = dict(model=name, images=batch * n_batches, batch=batch, gflop_per_image=round((lin + att + emb_f) / 1e9, 1))
    for k, dtype in modes.items():
        t = spread(per[k])
        m.set_compute_dtype(dtype)
        m.encode_image(px[0])
        _lib.prof_begin()
        m.encode_image(px[0])
        prof = _lib.prof_end()
        total = sum(prof[c]["ms"] for c in CLASSES)
        res[k] = dict(ms_per_200_images=t["ms"] * 200.0 / (batch * n_batches), ms_per_image=round(t["ms"] / (batch * n_batches), 4), windows=per[k],
                      end_to_end_tflops=round(flops / (t["ms"] * 1e-3) / 1e12, 1), **t,
                      profiled_batch={v: dict(ms=round(prof[c]["ms"], 3), launches=prof[c]["launches"], share_of_time=round(prof[c]["ms"] / total, 4),
                                              tflops=round(prof[c]["flops"] / (prof[c]["ms"] * 1e-3) / 1e12, 1) if prof[c]["ms"] > 0 else 0.0)
                                      for c, v in CLASSES.items()})
    res[f"speedup_{_lib.storage()}_over_fp32"] = round(res["fp32"]["ms"] / res[_lib.storage()]["ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--models", default="vit_h_14,vit_l_14")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_vision_half_bench.json"))
    ap.add_argument("--child", action="store_true", help="print the result of this process's storage format and stop (the fp16 leg)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    res = dict(**header(card=True), storage=_lib.storage(), models={n: bench_model(n, a.images, a.batch) for n in a.models.split(",")})
    if a.child:
        print("CLIPVH_BENCH " + json.dumps(res))
        return
    del res["storage"]
    res = {"bf16_process": res}
    torch.cuda.empty_cache()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--images", str(a.images), "--batch", str(a.batch), "--models", a.models],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=1500)
    lines = [l for l in r.stdout.splitlines() if l.startswith("CLIPVH_BENCH ")]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"the fp16 child ended with status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    res["fp16_process"] = json.loads(lines[-1][len("CLIPVH_BENCH "):])
    emit(res, a.out)


if __name__ == "__main__":
    main()
