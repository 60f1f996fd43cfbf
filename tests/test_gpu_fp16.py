"""-m gpu: the fp16-storage build of the kernel library (DFH_STORAGE=fp16, libdifashion_hip_f16.so) against the fp32 oracle.

The storage format is a property of the process, so the legs run in child processes (tests/fp16_child.py), one for the U-Net legs and
one for the sampler / VAE legs, one child at a time.  Each child is started once; if it dies, its stored failure fails every test that reads
its result and no further child is started.

Bounds: every rounding on the path is a storage rounding with fp32 accumulation, and fp16 carries 3 more significand bits than bf16, so
each bound is the bf16 test's own bound divided by 8: U-Net output and every tap <= 3e-2 / 8 = 3.75e-3 (tests/test_gpu_unet.py TOL),
teacher-forced sampler steps <= 3e-2 / 8, free-running final latents <= 8e-2 / 8 (tests/test_gpu_pipeline.py), VAE moments / decode
<= 3e-2 / 8 (tests/test_gpu_vae.py).  Measured values are printed before they are asserted.  A leg that misses its bound is a finding
about the fp16 walk (a step that does not scale with the storage format), not a reason to widen the bound."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 3e-2 / 8
FREE_RUN_TOL = 8e-2 / 8
# the bf16 walk's launch census of the batch-16 SD-1.5 forward (profiles/r06/parity_full_size.txt, line 5)
BF16_CENSUS_B16 = {'gemm_wide': 1, 'gemm_8wave': 13, 'gemm_lean': 116, 'gemm_other': 4, 'gemm_row': 32, 'splitk_reduce': 12,
                   'gstat_written': 37, 'gn_pre': 20, 'gn_stats': 6, 'gn_small': 6, 'layernorm': 3, 'ln_folded': 45, 'attention_x32': 20,
                   'attention_16': 12, 'conv_phase': 3, 'conv_wino': 24, 'mlp_fused': 5, 'gn_folded': 5}


_OUTCOME = {}          # group -> ("ok", result) | ("died", text): a child is started ONCE, whatever became of it


def child(group):
    """Result of the group's child process.  The outcome is kept, failure included: a child that died, aborted or ran out of time is never
    started again, and after it no other child is started either -- every test that needs one fails from the stored text."""
    if group in _OUTCOME:
        return _OUTCOME[group]
    died = [g for g, (kind, _) in _OUTCOME.items() if kind == "died"]
    if died:
        _OUTCOME[group] = ("died", f"not started: the fp16 child of group {died[0]!r} died before it ({_OUTCOME[died[0]][1][:300]})")
        return _OUTCOME[group]
    from tests.gpu_util import release_cached_gpu_memory
    release_cached_gpu_memory()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    try:
        r = subprocess.run([sys.executable, "-m", "tests.fp16_child", group], capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    except subprocess.TimeoutExpired as err:
        _OUTCOME[group] = ("died", f"the fp16 child ({group}) did not finish in {err.timeout} s")
        return _OUTCOME[group]
    print(r.stdout[-6000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("FP16_RESULT ")]
    if r.returncode != 0 or not lines:
        _OUTCOME[group] = ("died", f"the fp16 child ({group}) ended with status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
        return _OUTCOME[group]
    res = json.loads(lines[-1][len("FP16_RESULT "):])
    _OUTCOME[group] = ("died", f"aborted after leg {res['aborted_after']}: {res}") if "aborted_after" in res else ("ok", res)
    return _OUTCOME[group]


def leg(group, name):
    kind, res = child(group)
    assert kind == "ok", res
    assert res["storage"] == "fp16" and "storage=fp16" in res["build_info"], res
    assert name in res, f"leg {name} did not run: {res}"
    assert "error" not in res[name], res[name]["error"]
    return res[name]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("name", ["tiny", "glue", "tiny_linear_proj"])
def test_fp16_unet_matches_oracle_small(name):
    r = leg("unet", "small")[name]
    print(name, {k: f"{v:.2e}" for k, v in r["report"].items()})
    assert r["finite"]
    assert all(v <= TOL for v in r["report"].values()), r["report"]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("name", ["sd15_b1", "sd15_b16", "sd2base_b1"])
def test_fp16_unet_full_size_matches_oracle(name):
    """The child writes the per-tap table, bf16 beside fp16, to profiles/fp16_parity_full_size.txt (DFH_FP16_REPORT_DIR moves it)."""
    r = leg("unet", "full")[name]
    print(name, {k: f"{v:.2e}" for k, v in r["report"].items()})
    assert r["finite"]
    assert all(v <= TOL for v in r["report"].values()), r["report"]


@pytest.mark.timeout(1200)
def test_fp16_batch16_walk_takes_the_same_kernels_as_bf16():
    cen = leg("unet", "full")["sd15_b16"]["census"]
    print(cen)
    assert cen == BF16_CENSUS_B16, {k: (cen.get(k, 0), BF16_CENSUS_B16.get(k, 0)) for k in set(cen) | set(BF16_CENSUS_B16)
                                    if cen.get(k, 0) != BF16_CENSUS_B16.get(k, 0)}


@pytest.mark.timeout(1200)
def test_fp16_saturates_instead_of_overflowing():
    r = leg("unet", "saturation")
    print(r)
    assert r["input_peak"] < 65504.0 < r["oracle_peak"], "the input must be in range and an intermediate of the oracle beyond it"
    assert r["finite"] and r["hip_peak"] <= 65504.0
    assert r["taps_over_range"] and r["saturated_taps"], "no tap beyond the range reads exactly 65504: nothing saturated"


@pytest.mark.timeout(1200)
def test_fp16_inputs_and_refusals():
    r = leg("unet", "io")
    print(r)
    assert r["fp16_out_dtype"] == "torch.float16"
    assert r["fp16_vs_fp32_same_values_max_abs"] == 0.0          # same bits after the input cast -> the same walk
    assert r["fp16_vs_fp32_rel"] <= 2.0 ** -10                    # inputs rounded to fp16 once (11-bit significand), output rounded to fp16
    assert r["bf16_input"].startswith("TypeError") and "fp16-storage" in r["bf16_input"]
    assert r["enable_fp8"].startswith("DfhError") and "fp16" in r["enable_fp8"]
    assert r["train_forward"].startswith("DfhError") and "inference only" in r["train_forward"]
    assert r["c_abi_train"].startswith("DfhError") and "refused by the fp16-storage library" in r["c_abi_train"]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("case", ["gor_full_ddim50", "autoinit_gor_ddim6"])
def test_fp16_sampler_teacher_forced_and_free_running(case):
    r = leg("sampler_vae", "sampler")[case]
    print(case, r)
    assert r["finite"]
    assert r["teacher_forced_max"] <= TOL
    assert r["free_running"] <= FREE_RUN_TOL
    assert r["x_in_0_hist_exact"] and r["eps_0_exact"]           # the fp32 glue inside the product sampler stays bit-exact


@pytest.mark.timeout(1200)
def test_fp16_glue_kernels_stay_bit_exact():
    """dfh_cfg_step (guidance combine), dfh_assemble_input and the fp32 output of dfh_mutual_reduce are fp32 kernels and equal the oracle bit
    for bit under the fp16 library; dfh_mutual_reduce's storage-type output is that fp32 sum rounded once to fp16."""
    r = leg("sampler_vae", "glue")
    print(r)
    assert all(r.values()), r


@pytest.mark.timeout(1200)
def test_fp16_fashion_generation_draws_its_own_initial_latents():
    """DiFashion.fashion_generation unchanged on top of the fp16 library, auto-init path; bound = that test's 8e-2 / 8."""
    r = leg("sampler_vae", "fashion_generation")
    print(r)
    assert r["rng_stream_matches"], "torch CPU RNG stream differs from the capture container"
    assert r["init_exact"] and r["finite"]
    assert r["final"] <= FREE_RUN_TOL


@pytest.mark.timeout(1200)
def test_fp16_sd_vae_full_size_matches_oracle():
    r = leg("sampler_vae", "vae")
    print(r)
    assert r["finite"]
    assert r["moments"] <= TOL and r["decode"] <= TOL
