"""Child-process body of tests/test_gpu_fp16.py: the fp16-storage library is a property of the process, so every GPU leg of that file
runs here, in a process started with DFH_STORAGE=fp16 (``python -m tests.fp16_child <group>``).  Each leg records its measured figures
under a key of one JSON object, printed at the end as a line ``FP16_RESULT {...}``; the parent test asserts on them (the bounds live
there).  A leg that raises is recorded as {"error": ...} and the remaining legs still run -- unless the GPU itself failed, which ends
the process.  Tables go to DFH_FP16_REPORT_DIR (default: profiles/)."""
import json
import os
import sys
import time
import traceback

import torch

import difashion_amd as da
from difashion_amd import _lib
from oracle import unet_ref
from tests.gpu_util import DEV, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("DFH_FP16_REPORT_DIR") or os.path.join(ROOT, "profiles")
# the bf16 library's figures on the same legs (profiles/r06/parity_full_size.txt), printed beside the fp16 ones
BF16_SD15_B1 = {"conv_in": 2.87e-3, "down0": 7.21e-3, "down2": 1.48e-2, "mid": 1.60e-2, "up1": 1.74e-2, "up3": 1.39e-2, "out": 1.76e-2}
BF16_SD15_B16 = {"conv_in": 2.86e-3, "down0": 7.26e-3, "down1": 1.07e-2, "down2": 1.48e-2, "mid": 1.59e-2, "up1": 1.73e-2, "up2": 1.76e-2,
                 "up3": 1.37e-2, "out": 1.76e-2}
BF16_SD2BASE = 1.50e-2


def finite(t):
    return bool(torch.isfinite(t).all())


def leg_small():
    from tests.helpers import GLUE_CFG
    from tests.test_gpu_unet import hip_unet, inputs
    res = {}
    for name, cfg in [("tiny", unet_ref.TINY), ("glue", GLUE_CFG),
                      ("tiny_linear_proj", unet_ref.UNetConfig(sample_size=16, block_out_channels=(64, 128, 256, 256), cross_attention_dim=64,
                                                               num_heads=(2, 2, 4, 4), use_linear_projection=True))]:
        params = unet_ref.init_params(cfg, seed=3, w_std=0.05, affine_jitter=0.1)
        m = hip_unet(cfg, params)
        x, e = inputs(cfg, 3, 11)
        t = torch.tensor([7, 500, 981])
        taps = {}
        with torch.no_grad():
            ref = unet_ref.unet_forward(params, cfg, x, t, e, taps=taps)
            out = m(x.to(DEV), t.to(DEV), e.to(DEV)).sample
        rep, fin = {}, finite(out)
        for k in ("conv_in", "down0", "down1", "down2", "down3", "mid", "up0", "up1", "up2", "up3"):
            got = m.debug_tap(k).cpu()
            fin &= finite(got)
            rep[k] = rel_err(got, taps[k])
        rep["out"] = rel_err(out.cpu(), ref)
        print(name, {k: f"{v:.2e}" for k, v in rep.items()}, flush=True)
        res[name] = dict(report=rep, finite=fin)
    return res


def leg_inputs_and_refusals():
    """fp16 and fp32 inputs agree up to the input cast; a bf16 input, enable_fp8() and a training forward are refused with the reason."""
    from tests.test_gpu_unet import hip_unet, inputs
    cfg = unet_ref.TINY
    params = unet_ref.init_params(cfg, seed=3, w_std=0.05, affine_jitter=0.1)
    m = hip_unet(cfg, params)
    x, e = inputs(cfg, 2, 5)
    xd, ed = x.to(DEV), e.to(DEV)
    res = {}
    with torch.no_grad():
        o32 = m(xd, 500, ed).sample
        # inputs that ARE fp16 values: the fp32 call casts them to the same bits
        xh, eh = xd.half(), ed.half()
        o16 = m(xh, 500, eh).sample
        o32h = m(xh.float(), 500, eh.float()).sample
        res["fp16_out_dtype"] = str(o16.dtype)
        res["fp16_vs_fp32_same_values_max_abs"] = float((o16.float() - o32h.half().float()).abs().max())
        res["fp16_vs_fp32_rel"] = rel_err(o16.float().cpu(), o32.cpu())
        try:
            m(xd.bfloat16(), 500, ed.bfloat16())
            res["bf16_input"] = "NOT REFUSED"
        except TypeError as err:
            res["bf16_input"] = f"TypeError: {err}"
    try:
        m.enable_fp8()
        res["enable_fp8"] = "NOT REFUSED"
    except da.DfhError as err:
        res["enable_fp8"] = f"DfhError: {err}"
    mt = hip_unet(cfg, params)
    mt.train()
    try:
        mt(xd, 500, ed)                      # grad enabled, parameters require grad: the training forward
        res["train_forward"] = "NOT REFUSED"
    except da.DfhError as err:
        res["train_forward"] = f"DfhError: {err}"
    try:
        _lib.call("dfh_geglu_bwd", None, None, None, 0, 0, None)          # refused before any argument is looked at
        res["c_abi_train"] = "NOT REFUSED"
    except da.DfhError as err:
        res["c_abi_train"] = f"DfhError: {err}"
    return res


def leg_saturation():
    """An input scaled so that it is itself inside the fp16 range while an intermediate of the fp32 oracle exceeds 65504: the epilogue that
    stores that intermediate saturates (the tap reads exactly 65504 somewhere) and everything downstream stays finite."""
    from tests.test_gpu_unet import hip_unet, inputs
    cfg = unet_ref.TINY
    params = unet_ref.init_params(cfg, seed=3, w_std=0.05, affine_jitter=0.1)
    m = hip_unet(cfg, params)
    x, e = inputs(cfg, 2, 5)
    x = x * 1.5e4
    taps = {}
    with torch.no_grad():
        ref = unet_ref.unet_forward(params, cfg, x, torch.tensor([500, 500]), e, taps=taps)
        out = m(x.to(DEV), 500, e.to(DEV)).sample
    names = ("conv_in", "down0", "down1", "down2", "down3", "mid", "up0", "up1", "up2", "up3")
    got = {k: m.debug_tap(k) for k in names}
    over = [k for k in names if float(taps[k].abs().max()) > 65504.0]
    return dict(input_peak=float(x.abs().max()), oracle_peak=max(float(taps[k].abs().max()) for k in names), oracle_finite=finite(ref),
                finite=finite(out) and all(finite(v) for v in got.values()), taps_over_range=over,
                saturated_taps=[k for k in over if float(got[k].abs().max()) == 65504.0],
                hip_peak=max(float(v.abs().max()) for v in got.values()))


def _table(title, rep, bf):
    lines = [title, f"  {'tap':8s} {'bf16':>10s} {'fp16':>10s} {'bf16/fp16':>10s}"]
    for k, v in rep.items():
        b = bf.get(k)
        lines.append(f"  {k:8s} {b:10.2e} {v:10.2e} {b / v:10.1f}" if b else f"  {k:8s} {'':>10s} {v:10.2e}")
    return lines


def leg_full_size():
    """SD-1.5 at batch 1 and batch 16 (with the launch census) and SD-2-base, the inputs / weights / taps of tests/test_gpu_unet.py."""
    from tests.test_gpu_unet import full_size_reference, hip_unet, inputs
    res, lines = {}, ["fp16-storage library against the fp32 oracle, relative L2 per tap; bf16 column: profiles/r06/parity_full_size.txt",
                      _lib.raw().dfh_build_info().decode()]
    cfg = unet_ref.SD15
    params = unet_ref.init_params(cfg, seed=0)
    x, e = inputs(cfg, 1, 123)
    t = torch.tensor([481])
    ref, tap_err = full_size_reference("sd15_b1", params, cfg, x, t, e, want_taps=True)
    m = hip_unet(cfg, params, max_batch=1)
    with torch.no_grad():
        out = m(x.to(DEV), t.to(DEV), e.to(DEV)).sample
    fin = finite(out)
    rep = {}
    for k in ("conv_in", "down0", "down2", "mid", "up1", "up3"):
        got = m.debug_tap(k).cpu()
        fin &= finite(got)
        rep[k] = tap_err(k, got)
    rep["out"] = rel_err(out.cpu(), ref)
    res["sd15_b1"] = dict(report=rep, finite=fin)
    lines += _table("SD-1.5, batch 1", rep, BF16_SD15_B1)
    print("sd15", rep, flush=True)
    del m
    torch.cuda.empty_cache()

    x, e = inputs(cfg, 16, 123)
    t = torch.tensor([981, 981, 981, 981, 741, 741, 741, 741, 501, 501, 501, 501, 21, 21, 21, 21])
    ref, tap_err = full_size_reference("sd15_b16", params, cfg, x, t, e, want_taps=True)
    m = hip_unet(cfg, params, max_batch=16)
    del params
    xd, td, ed = x.to(DEV), t.to(DEV), e.to(DEV)
    with torch.no_grad():
        m(xd, td, ed)
        torch.cuda.synchronize()
        _lib.census_reset()
        t0 = time.time()
        out = m(xd, td, ed).sample
        torch.cuda.synchronize()
    cen = {k: v for k, v in _lib.census().items() if v}
    fin = finite(out)
    rep = {}
    for k in ("conv_in", "down0", "down1", "down2", "mid", "up1", "up2", "up3"):
        got = m.debug_tap(k).cpu()
        fin &= finite(got)
        rep[k] = tap_err(k, got)
    rep["out"] = rel_err(out.cpu(), ref)
    res["sd15_b16"] = dict(report=rep, finite=fin, census=cen)
    lines += _table("SD-1.5, batch 16", rep, BF16_SD15_B16) + [f"census {cen}"]
    print("sd15 B=16", rep, cen, flush=True)
    del m
    torch.cuda.empty_cache()

    cfg = unet_ref.SD2BASE
    params = unet_ref.init_params(cfg, seed=0)
    x, _ = inputs(cfg, 1, 321)
    e = torch.randn(1, 77, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(322))
    t = torch.tensor([731])
    ref, _ = full_size_reference("sd2base_b1", params, cfg, x, t, e)
    m = hip_unet(cfg, params, max_batch=1)
    del params
    with torch.no_grad():
        out = m(x.to(DEV), t.to(DEV), e.to(DEV)).sample
    rep = {"out": rel_err(out.cpu(), ref)}
    res["sd2base_b1"] = dict(report=rep, finite=finite(out))
    lines += _table("SD-2-base, batch 1", rep, {"out": BF16_SD2BASE})
    print("sd2base", rep, flush=True)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "fp16_parity_full_size.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return res


def leg_sampler():
    """Teacher-forced and free-running legs of tests/test_gpu_pipeline.py on the 50-step GOR case and the auto-init DDIM case."""
    from oracle import glue_ref, sched_ref
    from tests.helpers import GLUE_CFG, enc_params, glue_unet_params, load
    from tests.test_gpu_pipeline import encoder
    from tests.test_gpu_unet import hip_unet
    p = glue_unet_params()
    unet = hip_unet(GLUE_CFG, p, max_batch=32)
    res = {}
    for case in ("gor_full_ddim50", "autoinit_gor_ddim6"):
        rec = load(f"sample_{case}.npz")
        steps = int(rec["steps"])
        sc, sh, sm = (float(v) for v in rec["scales"])
        otaps = {}
        ref = glue_ref.sample_outfits(lambda x, t, e: unet_ref.unet_forward(p, GLUE_CFG, x, t, e), enc_params(rec), sched_ref.DDIMRef(),
                                      olists=rec["olists"], all_latents=rec["all_latents"], init_latents=rec["init_latents"],
                                      hist_latents=rec["hist_sel"], null_latent=rec["null_latent"],
                                      category_prompts=rec["category_prompts"], null_prompt=rec["null_prompt"],
                                      num_inference_steps=steps, cate_scale=sc, hist_scale=sh, mutual_scale=sm, taps=otaps)
        n = len([k for k in otaps if k.startswith("x_in_")])
        ehs = otaps["ehs"].to(DEV)
        errs = []
        with torch.no_grad():
            for i in range(n):
                got = unet(otaps[f"x_in_{i}"].to(DEV), otaps[f"t_{i}"], ehs, return_dict=False)[0]
                errs.append(rel_err(got.cpu(), otaps[f"unet_out_{i}"]))
        d = lambda k: rec[k].to(DEV)
        got = da.sample_outfits(unet, encoder(rec), da.DDIMScheduler(), olists=rec["olists"], all_latents=d("all_latents"),
                                init_latents=d("init_latents"), hist_latents=d("hist_sel"), null_latent=d("null_latent"),
                                category_prompts=d("category_prompts"), null_prompt=d("null_prompt"),
                                num_inference_steps=steps, cate_scale=sc, hist_scale=sh, mutual_scale=sm, taps=(ptaps := {}))
        # the fp32 glue inside the product sampler: history channels of the first assembled input are an exact selection (dfh_assemble_input),
        # and the guided epsilon of step 0 is the oracle's combination of the very per-branch predictions it was made from (dfh_cfg_step)
        mode, _ = glue_ref.cfg_plan(sc, sh, sm, True, True)
        res[case] = dict(teacher_forced_max=max(errs), free_running=rel_err(got.cpu(), ref), finite=finite(got), steps=n,
                         x_in_0_hist_exact=bool(torch.equal(ptaps["x_in_0"].cpu()[:, 4:], rec["x_in_0"][:, 4:])),
                         eps_0_exact=bool(torch.equal(ptaps["eps_0"].cpu(), glue_ref.cfg_combine(mode, ptaps["unet_out_0"].cpu(), sc, sh, sm))))
        print(case, res[case], flush=True)
    return res


def leg_glue():
    """The fp32 glue kernels under the fp16 library, on the inputs of tests/test_gpu_ops.py: dfh_mutual_reduce (its fp32 output bit-exact; its
    storage-type output = that sum rounded once to fp16), dfh_assemble_input and the guidance combine of dfh_cfg_step bit-exact."""
    import ctypes as C
    from difashion_amd.pipeline import sampling_tables, training_tables
    from difashion_amd.schedulers import DDIMScheduler
    from oracle import glue_ref
    from tests import gpu_util as gu
    rnd = gu.rnd
    res = {}
    olists = torch.tensor([[0, 0, 5, 6], [7, 0, 0, 0], [1, 2, 3, 0]])
    L = 4 * 16 * 16
    given, gen = rnd(12, 4, 16, 16, seed=52), rnd(6, 4, 16, 16, seed=53)
    tab, wt = (t.to(DEV) for t in sampling_tables(olists))
    out = torch.empty((6, L), dtype=torch.float16, device=DEV)
    out32 = torch.empty((6, L), device=DEV)
    _lib.call("dfh_mutual_reduce", _lib.ptr(gen), _lib.ptr(given), _lib.ptr(tab), _lib.ptr(wt), _lib.ptr(out), _lib.ptr(out32), 6, 4, L, gu.stream())
    torch.cuda.synchronize()
    ref = glue_ref.mutual_sum(olists, given.cpu(), gen.cpu())
    res["mutual_reduce_f32_exact"] = bool(torch.equal(out32.cpu().view_as(ref), ref))
    res["mutual_reduce_storage_is_rounded_f32"] = bool(torch.equal(out.cpu().view_as(ref), ref.half()))
    tab, wt = (t.to(DEV) for t in training_tables(8, 4))
    noisy = rnd(8, 4, 16, 16, seed=54)
    o32, o16 = torch.empty((8, L), device=DEV), torch.empty((8, L), dtype=torch.float16, device=DEV)
    _lib.call("dfh_mutual_reduce", _lib.ptr(noisy), None, _lib.ptr(tab), _lib.ptr(wt), _lib.ptr(o16), _lib.ptr(o32), 8, 4, L, gu.stream())
    torch.cuda.synchronize()
    ref = glue_ref.mutual_mean(noisy.cpu(), 4)
    res["mutual_mean_f32_exact"] = bool(torch.equal(o32.cpu().view_as(ref), ref))
    Fn, CL = 3, 4 * 8 * 8
    lat, mut, hist = rnd(Fn, 4, 8, 8, seed=55), rnd(Fn, 4, 8, 8, seed=56), rnd(Fn, 4, 8, 8, seed=57)
    null = rnd(4, 8, 8, seed=58)
    mreal = torch.tensor([1, 1, 0, 0], dtype=torch.uint8, device=DEV)
    hreal = torch.tensor([1, 0, 0, 0], dtype=torch.uint8, device=DEV)
    x = torch.empty((4 * Fn, 8, 8, 8), device=DEV)
    _lib.call("dfh_assemble_input", _lib.ptr(lat), _lib.ptr(mut), _lib.ptr(hist), _lib.ptr(null), _lib.ptr(mreal), _lib.ptr(hreal), _lib.ptr(x),
              4, Fn, CL, float(1 - 0.1), 0.1, 0, gu.stream())
    torch.cuda.synchronize()
    nulls = null[None].expand(Fn, -1, -1, -1)
    ref = torch.cat([(1 - 0.1) * torch.cat([lat] * 4) + 0.1 * torch.cat([mut, mut, nulls, nulls]), torch.cat([hist, nulls, nulls, nulls])], dim=1)
    res["assemble_input_exact"] = bool(torch.equal(x, ref))
    s = DDIMScheduler()
    s.set_timesteps(50)
    exact = True
    for mode, name, R in [(1, "full", 4), (2, "cate_hist", 3), (3, "cate_mutual", 3), (4, "cate", 2), (5, "hist", 2), (6, "mutual", 2), (0, "none", 1)]:
        eps_all, lat = rnd(R * Fn, 4, 8, 8, seed=59), rnd(Fn, 4, 8, 8, seed=60)
        for t in (981, 21):
            xx, eps_out = lat.clone(), torch.empty_like(lat)
            k = s.step_coef(t, 0.0)
            _lib.call("dfh_cfg_step", _lib.ptr(eps_all), _lib.ptr(xx), _lib.ptr(eps_out), None, xx.numel(), mode, 12.0, 4.0, 5.0, C.byref(k), gu.stream())
            torch.cuda.synchronize()
            exact &= bool(torch.equal(eps_out.cpu(), glue_ref.cfg_combine(name, eps_all.cpu(), 12.0, 4.0, 5.0)))
    res["cfg_step_combine_exact"] = exact
    return res


def leg_fashion_generation():
    """DiFashion.fashion_generation WITHOUT init_latents (it draws them itself) under the fp16 library: the call of
    tests/test_gpu_difashion.py::test_fashion_generation_draws_its_own_initial_latents against the golden run of the real reference class."""
    import types
    from tests.helpers import load
    from tests.helpers import GLUE_CFG, glue_unet_params
    from tests.test_gpu_difashion import DiFashion, H, IdentityVAE, TableText, TensorKeyDict, ZeroTok, encoder, sample_inputs
    from tests.test_gpu_unet import hip_unet
    name = "autoinit_gor_ddim6"
    rec = load(f"sample_{name}.npz")
    olists = torch.tensor([[0, 0, 0, 0], [4, 0, 0, 9]])
    images, null_img, cats, ids, uids, oids, _init, hist = sample_inputs(2, olists, seed=sum(map(ord, name)))
    if not torch.equal(images.reshape(8, 4, H, H), rec["all_latents"]):
        return dict(rng_stream_matches=False)
    unet = hip_unet(GLUE_CFG, glue_unet_params(), max_batch=32)
    args = types.SimpleNamespace(use_history=True, use_mutual_guidance=True, eta=0.1)
    m = DiFashion(args, vae=IdentityVAE(), unet=unet, fashion_encoder=encoder(rec), noise_scheduler=da.DDIMScheduler(),
                  text_encoder=TableText(), tokenizer=ZeroTok())
    d = lambda t: t.to(DEV)
    hist_dev = {u: TensorKeyDict({c: d(v) for c, v in h.items()}) for u, h in hist.items()}
    sc, sh, sm = (float(v) for v in rec["scales"])
    out = m.fashion_generation(uids=uids, oids=oids, input_ids=ids, olists=olists, outfit_images=d(images.reshape(8, 4, H, H)),
                               category=cats, history=hist_dev, num_inference_steps=int(rec["steps"]), category_guidance_scale=sc,
                               hist_guidance_scale=sh, mutual_guidance_scale=sm, null_img=d(null_img), eta=0.0, init_latents=None,
                               generator=torch.Generator().manual_seed(int(rec["generator_seed"])), output_type="latent", return_dict=True)
    final, init_out = out[0].images, out[-1]
    return dict(rng_stream_matches=True, init_exact=bool(torch.equal(init_out.cpu(), rec["init_latents"])),
                final=rel_err(final.cpu(), rec["final"]), finite=finite(final))


def leg_vae():
    from oracle import vae_ref
    from tests.test_gpu_vae import hip_vae
    cfg = vae_ref.SD_VAE
    params = vae_ref.init_params(cfg, seed=0)
    m = hip_vae(cfg, params)
    g = torch.Generator().manual_seed(4)
    x = torch.rand(1, 3, 512, 512, generator=g) * 2 - 1
    z = torch.randn(1, 4, 64, 64, generator=g)
    with torch.no_grad():
        ref_m = vae_ref.encode_moments(params, cfg, x)
        ref_img = vae_ref.decode(params, cfg, z)
    got_m = m.encode(x.to(DEV)).latent_dist.parameters.cpu()
    img = m.decode(z.to(DEV), return_dict=False)[0].cpu()
    return dict(moments=rel_err(got_m, ref_m), decode=rel_err(img, ref_img), finite=finite(got_m) and finite(img))


def write_sampler_vae_table(res):
    """profiles/fp16_parity_sampler_vae.txt: the measured figures of the glue / sampler / fashion_generation / VAE legs of this run."""
    lines = ["fp16-storage library, sampler / DiFashion.fashion_generation / VAE legs against the fp32 oracle (relative L2); bound = the bf16 test's",
             "bound / 8 (tests/test_gpu_pipeline.py 3e-2 and 8e-2, tests/test_gpu_difashion.py 8e-2, tests/test_gpu_vae.py 3e-2)",
             res["build_info"], "", f"  {'leg':70s} {'measured':>10s} {'bound':>10s}"]
    row = lambda name, v, b: lines.append(f"  {name:70s} {v:10.2e} {b:10.2e}")
    for case, r in (res.get("sampler") or {}).items():
        if isinstance(r, dict) and "teacher_forced_max" in r:
            row(f"{case}: teacher-forced U-Net output, worst of {r['steps']} steps", r["teacher_forced_max"], 3e-2 / 8)
            row(f"{case}: free-running final latents", r["free_running"], 8e-2 / 8)
            lines.append(f"  {case}: x_in_0 history channels exact = {r['x_in_0_hist_exact']}, guided eps_0 exact = {r['eps_0_exact']}")
    fg = res.get("fashion_generation") or {}
    if "final" in fg:
        row("fashion_generation, auto-init (autoinit_gor_ddim6): final latents", fg["final"], 8e-2 / 8)
        lines.append(f"  fashion_generation: initial latents equal the reference's draw = {fg['init_exact']}")
    v = res.get("vae") or {}
    if "moments" in v:
        row("SD VAE full size: encode moments", v["moments"], 3e-2 / 8)
        row("SD VAE full size: decode", v["decode"], 3e-2 / 8)
    g = res.get("glue") or {}
    if g and "error" not in g:
        lines.append("  fp32 glue kernels bit-exact (torch.equal against the oracle): " + ", ".join(f"{k}={x}" for k, x in g.items()))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "fp16_parity_sampler_vae.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


GROUPS = {"unet": [("small", leg_small), ("io", leg_inputs_and_refusals), ("saturation", leg_saturation), ("full", leg_full_size)],
          "sampler_vae": [("glue", leg_glue), ("sampler", leg_sampler), ("fashion_generation", leg_fashion_generation), ("vae", leg_vae)]}


def main(group):
    assert da.storage() == "fp16", "start this process with DFH_STORAGE=fp16"
    res = {"storage": da.storage(), "build_info": _lib.raw().dfh_build_info().decode()}
    for name, fn in GROUPS[group]:
        t0 = time.time()
        try:
            res[name] = fn()
        except Exception as err:                      # recorded; the parent fails the leg with this text
            traceback.print_exc()
            res[name] = {"error": f"{type(err).__name__}: {err}"}
            try:
                torch.cuda.synchronize()
            except Exception:                         # the GPU itself failed: nothing more is started on it
                res["aborted_after"] = name
                break
        res.setdefault("seconds", {})[name] = round(time.time() - t0, 1)
        torch.cuda.empty_cache()
    if group == "sampler_vae":
        write_sampler_vae_table(res)
    print("FP16_RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
