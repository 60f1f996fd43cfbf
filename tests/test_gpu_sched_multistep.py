"""-m gpu: the fused multistep sampler step ("Fused multistep sampler step").

6. dfh_cfg_multistep against the fp32 restatement (tests/helpers_sched_multistep.py), bit for bit, over every guidance mode,
conversion and kind, on both access widths, with guarded buffers; 7. the fused PLMS sequence against PNDMScheduler.step at every
entry; 8. DPMSolverMultistepScheduler's own step loop against the fp32 restatement (bit for bit) and the fp64 one (3x the fp32
restatement's own distance, the rule of rows f6 / f8); 9. OutfitSampler with PLMS and DPM-Solver++ against a teacher-forced twin
built from dfh_cfg_step(STEP_NONE) + the class's stand-alone step, and its allocation count against a DDIM step's; 10. the
fp16-storage library gives the same bits."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib, schedulers as S
from tests import helpers_sched_multistep as H
from tests.gpu_util import DEV, rel_err, release_cached_gpu_memory
from tests.helpers import GLUE_CFG, glue_unet_params, load
from tests.sched_multistep_fp16_child import FP16_CASES, case_bits
from tests.test_gpu_pipeline import encoder
from tests.test_gpu_unet import hip_unet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = list(itertools.product((True, False), repeat=3))


# ------------------------------------------------------------------ 6. the kernel
@pytest.mark.parametrize("shape,misalign", [((3, 4, 8, 8), 0), ((1, 4, 5, 5), 0), ((1, 1, 1, 1027), 0), ((3, 4, 8, 8), 1)],
                         ids=["n768_vec4", "n100_vec4_partial_block", "n1027_scalar_tail", "n768_unaligned_scalar"])
def test_kernel_equals_the_fp32_restatement_bit_for_bit(shape, misalign):
    """n = 768: three blocks of 16-byte accesses; n = 100: neither a multiple of the block nor of 256; n = 1027: odd, the scalar form
    over more than four blocks; n = 768 at buffers one float off a 16-byte boundary: the scalar form at a size the 16-byte form takes."""
    c = 0
    for mode in H.MODES:
        for conv, kind, terms in H.COMBOS:
            H.check_kernel_case(mode, shape, conv, kind, terms, seed=c, taps=TAPS[c % 8], in_place=c % 3 != 0, misalign=misalign)
            c += 1
    assert c == 7 * 18


# ------------------------------------------------------------------ 7. PLMS identity
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_fused_plms_sequence_equals_pndm_step_at_every_entry(prediction_type):
    shape = (3, 4, 8, 8)
    g = torch.Generator().manual_seed(11)
    x_T = torch.randn(shape, generator=g).to(DEV)
    ref, fused = da.PNDMScheduler(prediction_type=prediction_type), da.PNDMScheduler(prediction_type=prediction_type)
    ref.set_timesteps(10, device=DEV)
    fused.set_timesteps(10, device=DEV)
    assert len(ref._timesteps_host) == 11
    x_ref, lat = x_T.clone(), x_T.clone()
    slots, saved = [torch.empty_like(lat) for _ in range(4)], torch.empty_like(lat)
    for i, t in enumerate(ref._timesteps_host):
        out = torch.randn(shape, generator=g).to(DEV)
        x_ref = ref.step(out.clone(), t, x_ref, return_dict=False)[0]
        k, roles = fused.step_plan(i)
        S.cfg_multistep(out, saved if roles["x_src"] == "saved" else lat, lat, k, reads=[slots[j] for j in roles["reads"]],
                        q_out=None if roles["push"] is None else slots[roles["push"]], x_save=saved if roles["x_save"] else None)
        assert torch.equal(lat, x_ref), (prediction_type, i)
    assert bool(torch.isfinite(lat).all())


# ------------------------------------------------------------------ 8. DPM-Solver++ trajectory
@pytest.mark.parametrize("n", [10, 20])
@pytest.mark.parametrize("solver_type", ["midpoint", "heun"])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_dpm_step_loop_equals_the_restatement(n, solver_type, prediction_type):
    """Measured (MI355X), relative L2 of the final x against the fp64 restatement -- product == fp32 restatement in every case:
    see profiles/sched_multistep_gpu_tests.txt."""
    shape = (3, 4, 8, 8)
    g = torch.Generator().manual_seed(100 + n)
    x_T = torch.randn(shape, generator=g)
    outs = [torch.randn(shape, generator=g) for _ in range(n)]
    cfg = dict(solver_type=solver_type, prediction_type=prediction_type)
    ref32 = H.dpm_trajectory(outs, x_T, n, torch.float32, **cfg)
    ref64 = H.dpm_trajectory(outs, x_T, n, torch.float64, **cfg)
    sched = da.DPMSolverMultistepScheduler(**cfg)
    sched.set_timesteps(n, device=DEV)
    x = x_T.to(DEV)
    for i, t in enumerate(sched.timesteps):
        x_in, kept = x, x.clone()
        x = sched.step(outs[i].to(DEV), t, x_in, return_dict=False)[0]
        assert torch.equal(x_in, kept) and x.data_ptr() != x_in.data_ptr()      # the sample is not modified: the result is a new tensor
        assert torch.equal(x.cpu(), ref32[i]), (n, solver_type, prediction_type, i)
    yard = rel_err(ref32[-1], ref64[-1])
    got = rel_err(x.cpu(), ref64[-1])
    print(f"dpm++ {n} steps {solver_type} {prediction_type}: product vs fp64 {got:.3e}, fp32 restatement vs fp64 {yard:.3e}")
    assert got <= 3 * yard


# ------------------------------------------------------------------ 9. the sampler
@pytest.fixture(scope="module")
def unet():
    return hip_unet(GLUE_CFG, glue_unet_params(), max_batch=32)


def _prepare(unet, rec, sched):
    d = lambda k: rec[k].to(DEV)
    sc, sh, sm = (float(v) for v in rec["scales"])
    return da.OutfitSampler(unet, encoder(rec), sched).prepare(
        olists=rec["olists"], all_latents=d("all_latents"), init_latents=d("init_latents"), hist_latents=d("hist_sel"),
        null_latent=d("null_latent"), category_prompts=d("category_prompts"), null_prompt=d("null_prompt"), num_inference_steps=10,
        cate_scale=sc, hist_scale=sh, mutual_scale=sm, eta=0.1, use_history=bool(rec["use_history"]),
        use_mutual_guidance=bool(rec["use_mutual"]), keep_eps=True)


def _allocations():
    return torch.cuda.memory_stats()["allocation.all.allocated"]


def _step_counted(s, i):
    torch.cuda.synchronize()
    before = _allocations()
    s.step(i)
    torch.cuda.synchronize()
    return _allocations() - before


@pytest.mark.parametrize("kind", ["plms", "dpm"])
def test_sampler_is_one_launch_equal_to_its_twin_and_allocates_like_ddim(kind, unet):
    rec = load("sample_gor_full_ddim10.npz")
    make = da.PNDMScheduler if kind == "plms" else da.DPMSolverMultistepScheduler
    s = _prepare(unet, rec, make())
    assert s.mode_name == "full" and len(s.hist_slots) == (4 if kind == "plms" else 2) and (s.x_saved is not None) == (kind == "plms")
    twin = make()
    twin.set_timesteps(10, device=DEV)
    assert twin._timesteps_host == s.ts and len(s.ts) == (11 if kind == "plms" else 10)
    x = rec["init_latents"].to(DEV).float().clone()
    sc, sh, sm = s.scales
    none = _lib.StepCoef()
    none.kind = S.STEP_NONE
    counts = []
    for i, t in enumerate(s.ts):
        counts.append(_step_counted(s, i))
        eps = torch.empty_like(x)
        _lib.call("dfh_cfg_step", _lib.ptr(s.eps_all), None, _lib.ptr(eps), None, x.numel(), s.mode, sc, sh, sm, C.byref(none), _lib.stream_ptr())
        assert torch.equal(eps, s.eps_comb), (kind, i)
        x = twin.step(eps, t, x, return_dict=False)[0]
        assert torch.equal(x, s.latents), (kind, i)
    assert bool(torch.isfinite(x).all())
    ddim = _prepare(unet, rec, da.DDIMScheduler())
    ddim_counts = [_step_counted(ddim, i) for i in range(3)]
    print(f"{kind}: allocations per step {counts}, of a DDIM step {ddim_counts}")
    assert all(c == ddim_counts[2] for c in counts[2:])


# ------------------------------------------------------------------ 10. fp16-storage build
def test_fp16_storage_library_gives_the_same_bits():
    """The kernel is fp32 glue: libdifashion_hip_f16.so, in a process of its own, gives the bits of the default build."""
    here = {n: case_bits(n) for n in FP16_CASES}
    release_cached_gpu_memory()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    r = subprocess.run([sys.executable, "-m", "tests.sched_multistep_fp16_child"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("SCHED_MULTISTEP_FP16_RESULT ")]
    assert line, r.stdout[-2000:]
    res = json.loads(line[-1][len("SCHED_MULTISTEP_FP16_RESULT "):])
    assert res["storage"] == "fp16" and "storage=fp16" in res["build_info"]
    assert res["cases"] == here
