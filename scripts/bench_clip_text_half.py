#!/usr/bin/env python3
"""fp32 beside 16-bit: ``CLIPTextModel(input_ids)`` of the HIP CLIP text encoder at the CLIP-L/14 and
OpenCLIP-H/14 text towers, over 33 x 77 tokens (a training batch of 8 outfits plus the null prompt) and 51 x 77 (the prompt table),
reported and not gated: one JSON line to profiles/clip_text_half_bench.json.

  * this process (bf16 storage) times the fp32 tower and the bf16 tower of ONE model object, alternating inside every window, so
    that both see the same box in the same minutes; a child process under ``DFH_STORAGE=fp16`` does the same for fp32 beside fp16.
    The fp32 tower's kernels are the parent commit's, so its time in the same run is the baseline;
  * a call is what ``DiFashion.forward`` makes: ids already on the device, the wrapper's id range check (one host sync) included;
    device events around --calls calls, after a warm-up of every mode; the figure is the median of five windows and the spread
    (min .. max) is kept;
  * kernel time per launch class from a separately profiled call (dfh_prof_begin / dfh_prof_end bracket every launch with events:
    not the timed run): what is left of the call time is launch gaps and the host side;
  * achieved TFLOP/s = the algorithm's multiply-adds x 2 over the time: an end-to-end rate, not a kernel's share of a peak.

    python scripts/bench_clip_text_half.py [--calls 20] [--models sd15_clip_l,sd2_openclip_h] [--batches 33,51] [--out profiles/clip_text_half_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import torch
from _rowbench import ROOT, emit, header, randomise, spread

import difashion_amd as da  # noqa: E402
from difashion_amd import _lib  # noqa: E402

MODELS = {
    "sd15_clip_l": dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, hidden_act="quick_gelu"),
    "sd2_openclip_h": dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16, hidden_act="gelu"),
}
T = 77


def flops_per_call(cfg, batch):
    """multiply-adds x 2 of the linears and of causal attention (the lower triangle only)"""
    D, I, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
    M = batch * T
    return L * (2.0 * M * (4 * D * D + 2 * D * I) + 2.0 * 2.0 * batch * D * T * (T + 1) / 2)


def bench_model(name, batches, calls, windows=5):
    cfg = MODELS[name]
    own = _lib.storage_dtype()
    modes = {"fp32": torch.float32, _lib.storage(): own}
    m = da.CLIPTextModel(**cfg, init_seed=None).to("cuda").eval().requires_grad_(False)
    g = torch.Generator(device="cuda").manual_seed(0)
    randomise(m, g)                                          # the speed does not depend on the values; parity is tests/test_gpu_clip_text_half.py
    res = dict(model=name, tokens=T, shapes={})
    for batch in batches:
        ids = torch.randint(1, 49000, (batch, T), generator=g, device="cuda")

        def run(dtype):
            m.set_compute_dtype(dtype)
            for _ in range(calls):
                out = m(ids)[0]
            return out

        for dtype in modes.values():                         # warm-up: workspaces, the packed copy, code-object load
            assert torch.isfinite(run(dtype)).all()
        torch.cuda.synchronize()
        per = {k: [] for k in modes}
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(windows):
            for k, dtype in modes.items():                   # alternating: fp32, 16-bit, fp32, ...
                torch.cuda.synchronize()                     # (the mode switch inside run() costs nothing: the packed copy is kept across it)
                a.record()
                run(dtype)
                b.record()
                torch.cuda.synchronize()
                per[k].append(a.elapsed_time(b) / calls)
        flops = flops_per_call(cfg, batch)
        rec = dict(batch=batch, rows=batch * T, gflop_per_call=round(flops / 1e9, 1), calls_per_window=calls)
        for k, dtype in modes.items():
            t = spread(per[k])
            m.set_compute_dtype(dtype)
            m(ids)
            _lib.prof_begin()
            m(ids)
            prof = _lib.prof_end()
            rec[k] = dict(ms_per_call=t["ms"], windows=[round(v, 4) for v in per[k]], end_to_end_tflops=round(flops / (t["ms"] * 1e-3) / 1e12, 1), **t,
                          profiled_call={c: dict(ms=round(v["ms"], 3), launches=v["launches"]) for c, v in prof.items() if v["launches"]},
                          profiled_kernel_ms=round(sum(v["ms"] for v in prof.values()), 3))
        rec[f"speedup_{_lib.storage()}_over_fp32"] = round(rec["fp32"]["ms"] / rec[_lib.storage()]["ms"], 3)
        rec["faster_in_every_window"] = all(h < f for h, f in zip(per[_lib.storage()], per["fp32"]))
        res["shapes"][f"{batch}x{T}"] = rec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--models", default="sd15_clip_l,sd2_openclip_h")
    ap.add_argument("--batches", default="33,51")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_text_half_bench.json"))
    ap.add_argument("--child", action="store_true", help="print the result of this process's storage format and stop (the fp16 leg)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    batches = [int(b) for b in a.batches.split(",")]
    res = dict(**header(card=True), storage=_lib.storage(), models={n: bench_model(n, batches, a.calls) for n in a.models.split(",")})
    if a.child:
        print("CLIPTH_BENCH " + json.dumps(res))
        return
    del res["storage"]
    res = {"bf16_process": res}
    torch.cuda.empty_cache()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--models", a.models, "--batches", a.batches],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("CLIPTH_BENCH ")]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"the fp16 child ended with status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    res["fp16_process"] = json.loads(lines[-1][len("CLIPTH_BENCH "):])
    emit(res, a.out)


if __name__ == "__main__":
    main()
