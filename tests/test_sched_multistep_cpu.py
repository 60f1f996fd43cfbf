"""CPU tier (-m "not gpu"): the host side of the fused multistep sampler step ("Fused multistep sampler step").

1. the restatement (tests/helpers_sched_multistep.py) is pinned by a closed form in fp64; 2. the product's timestep lists, per-step
coefficients and order bookkeeping equal the restatement's; 3. the call surface of DPMSolverMultistepScheduler; 4. the C ABI of
dfh_cfg_multistep and its refusals (no launch is made); 5. the pointer roles of the PLMS list.  The arithmetic of the kernel is
checked on the GPU (tests/test_gpu_sched_multistep.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib, schedulers as S
from tests import helpers_sched_multistep as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEF_FIELDS = ["conv", "kind", "terms", "c0", "c1", "w", "cx", "ce", "cd0", "cr", "cd1"]
f32 = lambda v: np.float32(float(v))


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------ 1. the restatement against the closed form (fp64)
@pytest.mark.parametrize("n", [10, 20])
def test_order_1_is_the_ddim_update_on_the_same_grid(n):
    tab, ts = H.tables(torch.float64), H.timesteps(n)
    mu, s, x_T = H.gaussian_problem()
    xa = xb = x_T
    worst = 0.0
    for i, t in enumerate(ts):
        k = H.dpm_coef(tab, ts, i, have_history=i > 0, solver_order=1)
        assert k["kind"] == H.DPM1
        xa = H.update(k, xa, H.convert(k, H.exact_eps(tab, t, xa, mu, s), xa), [None])
        xb = H.ddim_step(tab, t, ts[i + 1] if i + 1 < len(ts) else 0, xb, H.exact_eps(tab, t, xb, mu, s))
        worst = max(worst, float((xa - xb).abs().max()))
    print(f"order 1 vs DDIM, {n} steps: max |diff| {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("n", [10, 20, 40])
def test_order_2_beats_order_1_on_the_gaussian_problem(n):
    """At the entry of the last step (t = timesteps[-1], before the large final lambda jump) the relative L2 error of order 2
    (midpoint) against the exact ODE solution is at least 5x smaller than that of order 1.  A wrong D1 factor (1, 0.25, -0.5 instead
    of 0.5) gives at most 2.1; the correct formulas give about 34, 11.7 and 11.0 at 10, 20 and 40 steps."""
    tab = H.tables(torch.float64)
    mu, s, x_T = H.gaussian_problem()
    errs = {}
    for order in (1, 2):
        x, t, t0 = H.solve_gaussian(n, order)
        errs[order] = rel_l2(x, H.exact_x(tab, t, t0, x_T, mu, s))
    print(f"{n} steps: order 1 {errs[1]:.3e} order 2 {errs[2]:.3e} ratio {errs[1] / errs[2]:.1f}")
    assert errs[1] >= 5 * errs[2]


# ------------------------------------------------------------------ 2. product host logic against the restatement
@pytest.mark.parametrize("n", [10, 15, 20, 25, 50, 1000])
def test_timestep_lists_equal_the_restatement(n):
    sched = da.DPMSolverMultistepScheduler()
    sched.set_timesteps(n)
    assert sched.timesteps.tolist() == sched._timesteps_host == H.timesteps(n)
    assert sched.timesteps.dtype == torch.int64 and sched.num_inference_steps == len(H.timesteps(n))
    if n == 1000:
        raw = np.linspace(0, 999, 1001).round()[::-1][:-1]
        assert len(set(raw.tolist())) < 1000 and len(sched.timesteps) == len(set(raw.tolist()))      # the duplicate is gone
    else:
        assert len(sched.timesteps) == n


def test_tables_equal_the_restatement():
    sched, tab = da.DPMSolverMultistepScheduler(), H.tables(torch.float32)
    for got, want in ((sched.alphas_cumprod, tab["ac"]), (sched.alpha_t, tab["alpha"]), (sched.sigma_t, tab["sigma"]), (sched.lambda_t, tab["lam"])):
        assert got.dtype == torch.float32 and torch.equal(got, want)


@pytest.mark.parametrize("n", [10, 20])
@pytest.mark.parametrize("solver_type", ["midpoint", "heun"])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_every_coefficient_equals_the_restatement_bit_for_bit(n, solver_type, prediction_type):
    sched = da.DPMSolverMultistepScheduler(solver_type=solver_type, prediction_type=prediction_type)
    sched.set_timesteps(n)
    tab, ts = H.tables(torch.float32), H.timesteps(n)
    for i in range(len(ts)):
        k, roles = sched.step_plan(i)
        want = H.dpm_coef(tab, ts, i, have_history=i > 0, solver_type=solver_type, prediction_type=prediction_type)
        assert (k.conv, k.kind) == (want["conv"], want["kind"]), i
        for name in ("c0", "c1", "cx", "cd0", "cr", "cd1"):
            got = np.float32(getattr(k, name))
            assert got.tobytes() == f32(want[name]).tobytes(), (i, name, got, float(want[name]))
        assert roles["push"] == i % 2 and roles["reads"] == ([] if k.kind == S.MS_DPM1 else [(i - 1) % 2])
        assert roles["x_src"] == "latents" and roles["x_save"] is False


def test_r0_of_the_third_step_written_out_from_the_table():
    sched = da.DPMSolverMultistepScheduler()
    sched.set_timesteps(10)
    assert sched._timesteps_host[:4] == [999, 899, 799, 699]
    lam = sched.lambda_t
    r0 = (lam[799] - lam[899]) / (lam[699] - lam[799])          # (lambda_s0 - lambda_s1) / (lambda_t - lambda_s0): NOT its inverse
    k, _ = sched.step_plan(2)
    assert np.float32(k.cr).tobytes() == f32(1.0 / r0).tobytes()
    assert 0.5 < float(r0) < 2.0 and abs(float(r0) - 1.0) > 1e-3      # the two lambda gaps differ: an inverted r0 is another number


def test_order_bookkeeping():
    sched = da.DPMSolverMultistepScheduler()
    for n, last_kind in ((10, S.MS_DPM1), (20, S.MS_DPM2)):       # lower_order_final acts below 15 entries
        sched.set_timesteps(n)
        kinds = [sched.step_plan(i)[0].kind for i in range(n)]
        assert kinds[0] == S.MS_DPM1 and kinds[1:-1] == [S.MS_DPM2] * (n - 2) and kinds[-1] == last_kind
    sched = da.DPMSolverMultistepScheduler(lower_order_final=False)
    sched.set_timesteps(10)
    assert sched.step_plan(9)[0].kind == S.MS_DPM2
    # the state a run leaves behind is reset by set_timesteps
    sched.lower_order_nums, sched._pushes, sched.model_outputs = 2, 7, [torch.zeros(1), torch.zeros(1)]
    sched.set_timesteps(10)
    assert sched.lower_order_nums == 0 and sched._pushes == 0 and sched.model_outputs == [None, None]
    # with no earlier output a step is first-order wherever it is in the list
    assert sched.step_plan(5, lower_order_nums=0)[0].kind == S.MS_DPM1
    first = da.DPMSolverMultistepScheduler(solver_order=1)
    first.set_timesteps(20)
    for i in range(20):
        k, roles = first.step_plan(i)
        assert k.kind == S.MS_DPM1 and roles["reads"] == []


# ------------------------------------------------------------------ 3. call surface
def test_from_config_swaps_between_the_three_classes(tmp_path):
    pndm = da.PNDMScheduler(prediction_type="v_prediction")
    dpm = da.DPMSolverMultistepScheduler.from_config(pndm.config)
    assert dpm.config.prediction_type == "v_prediction" and dpm.config.solver_order == 2 and "skip_prk_steps" not in dpm.config
    ddim = da.DDIMScheduler()
    dpm2 = da.DPMSolverMultistepScheduler.from_config(ddim.config, solver_type="heun")
    assert dpm2.config.solver_type == "heun" and dpm2.config.num_train_timesteps == 1000
    assert (dpm2.order, dpm2.init_noise_sigma) == (1, 1.0)
    back = da.PNDMScheduler.from_config(dpm2.config)
    assert back.config.skip_prk_steps is True and "solver_order" not in back.config
    assert "solver_type" not in da.DDIMScheduler.from_config(dpm.config).config
    dpm2.save_pretrained(str(tmp_path))
    again = da.DPMSolverMultistepScheduler.from_pretrained(str(tmp_path))
    assert dict(again.config) == dict(dpm2.config)
    assert dict(again.config)["algorithm_type"] == "dpmsolver++" and again.config.lower_order_final is True


@pytest.mark.parametrize("key,value", [("solver_order", 3), ("algorithm_type", "dpmsolver"), ("algorithm_type", "sde-dpmsolver"),
                                       ("algorithm_type", "sde-dpmsolver++"), ("solver_type", "bh1"), ("thresholding", True),
                                       ("use_karras_sigmas", True), ("lambda_min_clipped", -5.1), ("prediction_type", "sample")])
def test_unsupported_keys_raise_with_their_name(key, value):
    with pytest.raises(ValueError, match=key):
        da.DPMSolverMultistepScheduler(**{key: value})


def test_step_signature_and_cpu_refusal():
    params = inspect.signature(da.DPMSolverMultistepScheduler.step).parameters
    assert list(params) == ["self", "model_output", "timestep", "sample", "generator", "return_dict"]
    assert "eta" not in params and params["generator"].default is None and params["return_dict"].default is True
    sched = da.DPMSolverMultistepScheduler()
    with pytest.raises(ValueError, match="set_timesteps"):
        sched.step(torch.zeros(1, 4, 2, 2), 999, torch.zeros(1, 4, 2, 2))
    sched.set_timesteps(10)
    with pytest.raises(_lib.DfhError, match="HIP path only"):
        sched.step(torch.zeros(1, 4, 2, 2), 999, torch.zeros(1, 4, 2, 2))
    assert sched.step_index(899) == 1 and sched.step_index(123) == 9          # an absent timestep means the last entry


# ------------------------------------------------------------------ 4. C ABI, without a GPU
def test_symbol_struct_and_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "difashion_hip.h")).read(), flags=re.S)
    assert re.search(r"\bdfh_cfg_multistep\s*\(", src) and "#define DFH_ABI_VERSION 8" in src
    for lib_name in _lib._LIB_NAMES.values():
        assert hasattr(C.CDLL(os.path.join(_lib.CSRC, lib_name)), "dfh_cfg_multistep"), lib_name
    assert "dfh_cfg_multistep" in _lib.SIGNATURES and len(_lib.SIGNATURES["dfh_cfg_multistep"][1]) == 16
    body = re.search(r"typedef struct dfh_multistep_coef \{(.*?)\} dfh_multistep_coef;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", f.strip()) for f in re.sub(r"^[a-z_0-9]+\s+", "", decl).split(",")]
    assert fields == COEF_FIELDS == [f[0] for f in _lib.MultistepCoef._fields_]
    assert C.sizeof(_lib.MultistepCoef) == 3 * 4 + 11 * 4 == 56        # 3 ints, 2 + 4 + 2 + 3 floats, no padding
    assert _lib.MultistepCoef.w.offset == 20 and _lib.MultistepCoef.cd1.offset == 52


def _call(n=64, mode=0, conv=0, kind=S.MS_PLMS, terms=1, lat=0x10000, x_src=0x10000, q_out=0, h=(0, 0, 0)):
    k = _lib.MultistepCoef()
    k.conv, k.kind, k.terms = conv, kind, terms
    p = C.c_void_p
    _lib.call("dfh_cfg_multistep", p(0x90000), p(x_src), p(lat), p(0), p(q_out), p(0), p(h[0]), p(h[1]), p(h[2]), n, mode, 1.0, 1.0, 1.0,
              C.byref(k), p(0))


@pytest.mark.parametrize("what,kw", [
    ("n == 0", dict(n=0)),
    ("guidance mode", dict(mode=7)), ("guidance mode", dict(mode=-1)),
    ("unknown conv", dict(conv=3)), ("unknown conv", dict(conv=-1)),
    ("unknown kind", dict(kind=3)), ("unknown kind", dict(kind=-1)),
    ("terms outside 1..4", dict(terms=0)), ("terms outside 1..4", dict(terms=5)),
    ("h1 missing", dict(terms=2)), ("h2 missing", dict(terms=3, h=(0x20000, 0, 0))), ("h3 missing", dict(terms=4, h=(0x20000, 0x30000, 0))),
    ("h1 missing", dict(kind=S.MS_DPM2)),
    ("aliases", dict(terms=2, h=(0x10000, 0, 0))), ("aliases", dict(terms=3, h=(0x20000, 0x10000, 0))),
    ("aliases", dict(terms=4, h=(0x20000, 0x30000, 0x10000))), ("aliases", dict(q_out=0x10000)),
    ("aliases", dict(q_out=0x10000 + 4 * 63)), ("aliases", dict(kind=S.MS_DPM2, h=(0x10000 - 4 * 63, 0, 0))),
])
def test_entry_point_refusals_happen_before_any_launch(what, kw):
    """Made-up non-null addresses: a call that got past the checks would fault, so each case must be refused by the host code."""
    with pytest.raises(_lib.DfhError, match=re.escape(what)):
        _call(**kw)


def test_null_arguments_are_refused():
    for kw in (dict(lat=0), dict(x_src=0)):
        with pytest.raises(_lib.DfhError, match="null argument"):
            _call(**kw)


# ------------------------------------------------------------------ 5. PLMS pointer roles
def _transfer(sched, t, prev_t, vpred):
    ac = sched.alphas_cumprod
    a_t, a_prev = ac[t], (ac[prev_t] if prev_t >= 0 else ac[0])
    coeff = float((a_prev / a_t) ** 0.5)
    c_e = float((a_prev - a_t) / (a_t * (1 - a_prev) ** 0.5 + (a_t * (1 - a_t) * a_prev) ** 0.5))
    if vpred:
        return coeff - c_e * float((1 - a_t) ** 0.5), c_e * float(a_t ** 0.5)
    return coeff, c_e


@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_plms_roles_of_all_eleven_entries(prediction_type):
    sched = da.PNDMScheduler(prediction_type=prediction_type)
    sched.set_timesteps(10)
    ts = sched._timesteps_host
    assert ts == [901, 801, 801, 701, 601, 501, 401, 301, 201, 101, 1]
    W = H.PLMS_W
    #        push  reads      weights     x_src      x_save  (t, prev_t) of the transfer
    want = [(0, [], W[1], "latents", True, (901, 801)),
            (None, [0], [0.5, 0.5], "saved", False, (901, 801)),
            (1, [0], W[2], "latents", False, (801, 701)),
            (2, [1, 0], W[3], "latents", False, (701, 601)),
            (3, [2, 1, 0], W[4], "latents", False, (601, 501)),
            (0, [3, 2, 1], W[4], "latents", False, (501, 401)),
            (1, [0, 3, 2], W[4], "latents", False, (401, 301)),
            (2, [1, 0, 3], W[4], "latents", False, (301, 201)),
            (3, [2, 1, 0], W[4], "latents", False, (201, 101)),
            (0, [3, 2, 1], W[4], "latents", False, (101, 1)),
            (1, [0, 3, 2], W[4], "latents", False, (1, -99))]
    for i, (push, reads, w, x_src, x_save, (t, prev_t)) in enumerate(want):
        k, roles = sched.step_plan(i)
        assert roles == dict(push=push, reads=reads, x_src=x_src, x_save=x_save), i
        assert (k.conv, k.kind, k.terms) == (S.MS_CONV_NONE, S.MS_PLMS, len(w)), i
        assert [np.float32(k.w[j]) for j in range(len(w))] == [np.float32(v) for v in w], i
        cx, ce = _transfer(sched, t, prev_t, prediction_type == "v_prediction")
        assert (np.float32(k.cx), np.float32(k.ce)) == (np.float32(cx), np.float32(ce)), i
        assert push is None or push not in reads        # the slot that is written is never one that is read
    assert sched.counter == 0 and sched.ets == []       # the plan is a pure function: the scheduler's own state is untouched
