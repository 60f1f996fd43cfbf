"""What gradient checkpointing costs in time: the SD-1.5 training step at batch 32 (the forward that keeps what the backward needs, then the
backward; synthetic weights as in bench.py) in the three modes of dfh_unet_set_checkpointing, on one device.

    python scripts/bench_checkpointing.py [--parent-lib <libdifashion_hip.so of the parent commit>] > profiles/checkpointing_bench.json

Method: one worker process per library.  Inside a worker the modes alternate (0, 1, 2, 0, 1, 2, ...): every visit binds the mode's
workspace, runs warm-up steps, then one WINDOW of timed steps with three device events a step (before the forward, between forward and
backward, after the backward); a window's figure is the median of its steps.  Per mode: the median over the windows, and their
minimum / maximum as the spread.  With --parent-lib the workers alternate too (this tree, parent, this tree, parent): the parent's library
runs mode 0 only, loaded through DFH_LIB, and mode 0 of this tree must sit inside the spread of the two.  No figure is asserted anywhere."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(args):
    import torch
    import difashion_amd as da
    from difashion_amd import _lib
    dev = torch.device("cuda", 0)
    B = args.batch
    m = da.UNet2DConditionModel(sample_size=64, in_channels=8, max_batch=B, init_seed=None).to(dev).train()
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():                          # bench.py's synthetic weights
        for n, p in m.named_parameters():
            is_norm = ".norm" in n or n.startswith("conv_norm_out")
            if n.endswith(".weight") and not is_norm:
                p.normal_(0.0, 0.02, generator=g)
            elif n.endswith(".weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    x = torch.randn(B, 8, 64, 64, device=dev, generator=g).requires_grad_(True)
    e = torch.randn(B, 77, 768, device=dev, generator=g)
    t = torch.randint(0, 1000, (B,), device=dev, generator=g)
    dout = torch.randn(B, 4, 64, 64, device=dev, generator=g) / 64
    modes = [int(v) for v in args.modes.split(",")]
    windows = {mode: [] for mode in modes}
    workspace = {}

    def one_step(events):
        if events:
            events[0].record()
        out = m(x, t, e).sample
        if events:
            events[1].record()
        out.backward(dout)
        if events:
            events[2].record()

    for _ in range(args.rounds):
        for mode in modes:
            if mode:
                m.enable_gradient_checkpointing(keep_attention=mode == 2)
            else:
                m.disable_gradient_checkpointing()
            for _ in range(args.warmup):
                one_step(None)
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
            for ev in evs:
                one_step(ev)
            torch.cuda.synchronize()
            fwd = [ev[0].elapsed_time(ev[1]) for ev in evs]
            tot = [ev[0].elapsed_time(ev[2]) for ev in evs]
            windows[mode].append(dict(forward_ms=statistics.median(fwd), step_ms=statistics.median(tot)))
            workspace[mode] = m._train_buffers[3].numel()
    print("RESULT " + json.dumps(dict(lib=_lib.LIB_PATH, build=_lib.raw().dfh_build_info().decode(), device=torch.cuda.get_device_name(0),
                                      windows={str(k): v for k, v in windows.items()}, workspace_bytes={str(k): v for k, v in workspace.items()})))


def summary(windows):
    out = {}
    for key in ("forward_ms", "step_ms"):
        v = [w[key] for w in windows]
        out[key] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), windows=len(v))
    out["backward_ms"] = round(out["step_ms"]["median"] - out["forward_ms"]["median"], 3)
    return out


def run_worker(args, modes, lib=None):
    env = {k: v for k, v in os.environ.items() if k not in ("DFH_LIB", "DFH_LIB_ALLOW_ABI_MISMATCH")}
    if lib:
        env.update(DFH_LIB=lib, DFH_LIB_ALLOW_ABI_MISMATCH="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--modes", modes, "--batch", str(args.batch), "--rounds", str(args.rounds),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100)
    if r.returncode != 0:
        sys.exit(f"worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    print(f"[bench_checkpointing] worker done: modes {modes}, library {lib or 'this tree'}", file=sys.stderr, flush=True)
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--modes", default="0,1,2")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--passes", type=int, default=2, help="how often the (this tree, parent) pair of workers runs")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    mine, parent, info = {}, [], {}
    for _ in range(args.passes if args.parent_lib else 1):
        r = run_worker(args, "0,1,2")
        info = dict(device=r["device"], build=r["build"], workspace_bytes=r["workspace_bytes"])
        for mode, w in r["windows"].items():
            mine.setdefault(mode, []).extend(w)
        if args.parent_lib:
            parent.extend(run_worker(args, "0", lib=os.path.abspath(args.parent_lib))["windows"]["0"])
    res = dict(workload=f"SD-1.5 U-Net training step, batch {args.batch}: forward_train + backward, d_sample on, gradients accumulated",
               method=f"{args.rounds} rounds x modes alternating per worker, {args.warmup} warm-up + {args.steps} timed steps a window, "
                      "device events, window = median of its steps; median / min / max over the windows", **info,
               modes={mode: summary(w) for mode, w in mine.items()})
    if parent:
        res["parent_mode0"] = summary(parent)
    base = res["modes"]["0"]
    for mode in ("1", "2"):
        s = res["modes"][mode]
        s["step_over_mode0"] = round(s["step_ms"]["median"] / base["step_ms"]["median"], 4)
        s["extra_ms"] = round(s["step_ms"]["median"] - base["step_ms"]["median"], 3)
        s["extra_over_forward"] = round(s["extra_ms"] / base["forward_ms"]["median"], 4)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
