#!/usr/bin/env python3
"""Do two builds of the library launch and compute the same thing, switch by switch?  For a host-only change of the walks.

    python scripts/walk_identity.py run OUT_DIR                  one process: the legs below under the environment it was started with
    python scripts/walk_identity.py compare OTHER_LIB [REPORT]   this tree against DFH_LIB=OTHER_LIB, once with nothing set and once per
                                                                 SETTINGS entry, one child process at a time

A run is the smallest config of tests/test_gpu_unet.py with attention at more than one level (GLUE_CFG): one bf16 forward at B = 2, one
forward with the dup-tail hint at B = 4 / dup = 1, one forward after enable_fp8(), one training step (forward + backward) -- and, because
GLUE_CFG's first block is 32 wide and has no e4m3 copy, the dup-tail forward of TINY after enable_fp8().  Two more legs cover the run
cache (a GLUE_CFG forward at B = 2 through prepare_run over three timesteps) and the VAE (the smallest of tests/test_gpu_vae.py: encode
at B = 3 / 32x32, decode of its latents).  It writes the GEMM plan dump
(DFH_GEMM_PLAN_DUMP), the census of every leg and the sha256 of every output tensor; gradients of vectors (biases, norm scales) are
summed with float atomics and are kept as values instead (compared as tests/test_gpu_train.py does: rtol 1e-5, atol 1e-6 of the largest)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = ["", "DFH_LN_FOLD=0", "DFH_QKV_MERGE=0", "DFH_FFP_FOLD=0", "DFH_GN_FOLD=0", "DFH_GN_PRE=0", "DFH_WINO=0", "DFH_WINO_CHAIN=0",
            "DFH_UPS_PHASE=0", "DFH_MLP_FUSED=0", "DFH_FP8_EXT=0", "DFH_TRAIN_SIDE=0", "DFH_TRAIN_UPS_PHASE=0"]
TAPS = ("conv_in", "down0", "down1", "down2", "down3", "mid", "up0", "up1", "up2", "up3")


def run(out_dir):
    import torch

    from difashion_amd import _lib
    from oracle import unet_ref
    from tests.helpers import GLUE_CFG
    from tests.test_gpu_unet import DEV, hip_unet, inputs

    sha = lambda t: hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()
    rec, vectors = {}, {}

    def forward(leg, m, cfg, B, dup=0):
        x, e = inputs(cfg, B, 23)
        x, e = x.to(DEV), e.to(DEV)
        if dup:
            x[B - dup:] = x[B - 2 * dup:B - dup]
        with torch.no_grad():
            m(x, 501, e)                                   # first call: packs and derives the weights
            _lib.census_reset()
            m._dup_tail_once = dup
            out = m(x, 501, e).sample
        torch.cuda.synchronize()
        rec[leg] = {"census": {k: v for k, v in _lib.census().items() if v}, "sha256": {"out": sha(out), **{k: sha(m.debug_tap(k)) for k in TAPS}}}

    params = unet_ref.init_params(GLUE_CFG, seed=5, w_std=0.05, affine_jitter=0.1)
    m = hip_unet(GLUE_CFG, params, max_batch=4)
    forward("bf16_B2", m, GLUE_CFG, 2)
    forward("dup_tail_B4_dup1", m, GLUE_CFG, 4, dup=1)
    m.enable_fp8()
    forward("fp8_B2", m, GLUE_CFG, 2)
    mt = hip_unet(unet_ref.TINY, unet_ref.init_params(unet_ref.TINY, seed=5, w_std=0.05, affine_jitter=0.1), max_batch=4)
    mt.enable_fp8()
    forward("tiny_fp8_dup_tail_B4_dup1", mt, unet_ref.TINY, 4, dup=1)

    m = hip_unet(GLUE_CFG, params, max_batch=4)
    x, e = (t.to(DEV) for t in inputs(GLUE_CFG, 2, 23))
    steps = [981, 501, 21]
    with torch.no_grad():
        m(x, steps[0], e)                                  # packs and derives the weights
        m.prepare_run(e, steps)
        _lib.census_reset()
        outs = {f"out_t{t}": sha(m(x, t, e).sample) for t in steps}
        torch.cuda.synchronize()
        rec["run_cache_B2"] = {"census": {k: v for k, v in _lib.census().items() if v}, "sha256": {"out": outs[f"out_t{steps[-1]}"], **outs}}
        m.end_run()

    from oracle import vae_ref
    from tests.test_gpu_vae import hip_vae
    v = hip_vae(vae_ref.TINY_VAE, vae_ref.init_params(vae_ref.TINY_VAE, seed=2, w_std=0.05, affine_jitter=0.1))
    img = (torch.rand(3, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    with torch.no_grad():
        _lib.census_reset()
        dist = v.encode(img).latent_dist
        dec = v.decode(dist.mean, return_dict=False)[0]
    torch.cuda.synchronize()
    rec["vae_tiny_B3"] = {"census": {k: v_ for k, v_ in _lib.census().items() if v_}, "sha256": {"out": sha(dec), "moments": sha(dist.parameters)}}

    m = hip_unet(GLUE_CFG, params, max_batch=4).train()
    x, e = inputs(GLUE_CFG, 3, 11)
    dout = torch.randn(3, GLUE_CFG.out_channels, 16, 16, generator=torch.Generator().manual_seed(5))
    xd = x.to(DEV).requires_grad_(True)
    _lib.census_reset()
    out = m(xd, torch.tensor([7, 500, 981]).to(DEV), e.to(DEV)).sample
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    hashes = {"out": sha(out), "d_sample": sha(xd.grad)}
    for k, p in m.named_parameters():
        if p.grad.ndim >= 2:
            hashes["grad " + k] = sha(p.grad)
        else:
            vectors[k] = p.grad.detach().float().cpu()
    rec["train_step_B3"] = {"census": {k: v for k, v in _lib.census().items() if v}, "sha256": hashes}
    torch.save(vectors, os.path.join(out_dir, "vector_grads.pt"))
    with open(os.path.join(out_dir, "legs.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


def child(out_dir, setting, lib):
    os.makedirs(out_dir, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DFH_")}
    env["DFH_GEMM_PLAN_DUMP"] = os.path.join(out_dir, "plan_dump.txt")
    if setting:
        env.update([setting.split("=")])
    if lib:
        env.update(DFH_LIB=lib, DFH_LIB_ALLOW_ABI_MISMATCH="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "run", out_dir], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:           # a fault ends the whole comparison: nothing more is started on the GPU
        sys.exit(f"run failed ({r.returncode}) under '{setting}' lib={lib or 'this tree'}:\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
    return json.load(open(os.path.join(out_dir, "legs.json"))), open(env["DFH_GEMM_PLAN_DUMP"]).read()


def compare(other_lib, report, work):
    import torch
    lines, same_all, default = [], True, None
    for setting in SETTINGS:
        tag = setting.replace("=", "_") or "default"
        mine, dump_m = child(os.path.join(work, "tree", tag), setting, None)
        theirs, dump_t = child(os.path.join(work, "other", tag), setting, os.path.abspath(other_lib))
        census = all(mine[l]["census"] == theirs[l]["census"] for l in mine)
        hashes = all(mine[l]["sha256"] == theirs[l]["sha256"] for l in mine)
        va, vb = (torch.load(os.path.join(work, side, tag, "vector_grads.pt")) for side in ("tree", "other"))
        worst = 0.0
        for k in va:
            torch.testing.assert_close(va[k], vb[k], rtol=1e-5, atol=1e-6 * float(vb[k].abs().max() + 1e-30), msg=k)
            worst = max(worst, float((va[k] - vb[k]).abs().max() / (vb[k].abs().max() + 1e-30)))
        if default is None:
            default = mine
        reached = "" if not setting else ("" if any(mine[l]["census"] != default[l]["census"] for l in mine) else
                                          "   [census equals the default's: the switch's path is not reached at this size, or it changes no counted launch]")
        ok = census and hashes and dump_m == dump_t and set(mine) == set(theirs)
        same_all = same_all and ok
        print(f"[{tag}] {'identical' if ok else 'DIFFERS'}", file=sys.stderr, flush=True)
        lines.append(f"{setting or '(nothing set)':<24} plan dump {'identical' if dump_m == dump_t else 'DIFFERS'} ({len(dump_m.splitlines())} launches, sha256 "
                     f"{hashlib.sha256(dump_m.encode()).hexdigest()[:16]})  census {'identical' if census else 'DIFFERS'}  "
                     f"{sum(len(mine[l]['sha256']) for l in mine)} tensor hashes {'identical' if hashes else 'DIFFER'}  "
                     f"{len(va)} vector gradients within tolerance (largest difference {worst:.1e} of the largest value){reached}")
        for l in sorted(mine):
            lines.append(f"    {l:<28} out {mine[l]['sha256']['out'][:16]}  census {json.dumps(mine[l]['census'], sort_keys=True)}")
    lines.append(f"all {len(SETTINGS)} settings identical between the two builds: {same_all}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if report:
        open(report, "w").write(text)
    return 0 if same_all else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None, tempfile.mkdtemp(prefix="walk_identity_")))
