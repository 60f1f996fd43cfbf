"""DDIMScheduler / PNDMScheduler / DPMSolverMultistepScheduler with the diffusers call surface the reference glue uses
(SURVEY.md 8b): ``config.num_train_timesteps`` / ``config.prediction_type``
(DiFashion/models/difashion.py:154,:241), ``add_noise`` (:158), ``get_velocity`` (:244),
``alphas_cumprod`` (:270,:639), ``set_timesteps`` + ``timesteps`` (:356-357), ``scale_model_input``
(:472), ``step(eps, t, x, **{eta, generator}, return_dict=False)[0]`` (:569, kwargs discovered by
``inspect.signature`` :665-673), ``order`` (:433,:574), ``init_noise_sigma`` (:632).

The elementwise updates run in libdifashion_hip.so (dfh_cfg_step / dfh_cfg_multistep / dfh_noise_mix); the host side only
derives the per-step scalar coefficients from the fp32 alpha-bar table, with the same fp32 operations
the published diffusers code uses.  Device tensors only: no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Optional

import numpy as np
import torch

from . import _lib
from .unet import FrozenDict

CFG_NONE = 0
STEP_NONE, STEP_DDIM, STEP_LINEAR = -1, 0, 1
# dfh_cfg_multistep: conversion of the model output and kind of the update (include/difashion_hip.h)
MS_CONV_NONE, MS_CONV_X0_EPS, MS_CONV_X0_V = 0, 1, 2
MS_PLMS, MS_DPM1, MS_DPM2 = 0, 1, 2
PLMS_WEIGHTS = ((1.0,), (1.5, -0.5), (23 / 12, -16 / 12, 5 / 12), (55 / 24, -59 / 24, 37 / 24, -9 / 24))    # newest first


class SchedulerOutput(dict):
    __getattr__ = dict.__getitem__


def cfg_multistep(out_all, x_src, lat, coef: "_lib.MultistepCoef", *, reads=(), q_out=None, x_save=None, m_out=None,
                  mode: int = CFG_NONE, scales=(1.0, 1.0, 1.0)):
    """One dfh_cfg_multistep launch: ``lat`` <- update of ``x_src`` by the combined ``out_all`` and the history ``reads`` (newest first)."""
    h = [_lib.ptr(t) for t in reads] + [None] * (3 - len(reads))
    sc, sh, sm = scales
    _lib.call("dfh_cfg_multistep", _lib.ptr(out_all), _lib.ptr(x_src), _lib.ptr(lat), _lib.ptr(m_out), _lib.ptr(q_out), _lib.ptr(x_save),
              *h, lat.numel(), mode, sc, sh, sm, C.byref(coef), _lib.stream_ptr())


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise _lib.DfhError("scheduler arithmetic runs on the HIP path only: tensors must live on 'cuda'")


class _SchedulerBase:
    order = 1
    init_noise_sigma = 1.0
    config_name = "scheduler_config.json"

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", steps_offset: int = 1, set_alpha_to_one: bool = False,
                 prediction_type: str = "epsilon", clip_sample: bool = False, **unused):
        if beta_schedule != "scaled_linear":
            raise ValueError("only the 'scaled_linear' schedule of the Stable Diffusion configs is supported")
        if clip_sample:
            raise ValueError("clip_sample is not used by the Stable Diffusion scheduler configs")
        self.config = FrozenDict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                 beta_schedule=beta_schedule, steps_offset=steps_offset,
                                 set_alpha_to_one=set_alpha_to_one, prediction_type=prediction_type,
                                 clip_sample=clip_sample)
        self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._timesteps_host = self.timesteps.tolist()
        self._dev_tables = {}

    # -- diffusers persistence surface (difashion.py:64)
    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = None, **kwargs):
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, cls.config_name)) as f:
            cfg = {k: v for k, v in json.load(f).items() if not k.startswith("_")}
        cfg.update(kwargs)
        return cls(**cfg)

    @classmethod
    def from_config(cls, config, **overrides):
        """diffusers' scheduler swap, ``Other.from_config(pipe.scheduler.config)``: keys this class does not know are ignored."""
        cfg = {k: v for k, v in dict(config).items() if not k.startswith("_")}
        cfg.update(overrides)
        return cls(**cfg)

    def save_pretrained(self, save_directory: str):
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, self.config_name), "w") as f:
            json.dump(dict(self.config, _class_name=type(self).__name__), f, indent=2)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _tables(self, device):
        key = str(device)
        if key not in self._dev_tables:
            a = self.alphas_cumprod
            self._dev_tables[key] = ((a ** 0.5).to(device).contiguous(), ((1 - a) ** 0.5).to(device).contiguous())
        return self._dev_tables[key]

    def _mix(self, x0, noise, timesteps, want_velocity):
        _require_cuda(x0, noise)
        if x0.dtype != torch.float32 or noise.dtype != torch.float32:
            raise TypeError("add_noise / get_velocity operate on float32 latents")
        rows = x0.shape[0]
        L = x0[0].numel()
        t = timesteps.to(device=x0.device, dtype=torch.int64).reshape(-1).contiguous()
        if t.numel() != rows:
            raise ValueError("one timestep per row expected")
        sa, sb = self._tables(x0.device)
        out = torch.empty_like(x0)
        x0c, nc = x0.contiguous(), noise.contiguous()
        _lib.call("dfh_noise_mix", _lib.ptr(x0c), _lib.ptr(nc), _lib.ptr(t), _lib.ptr(sa), _lib.ptr(sb),
                  None if want_velocity else _lib.ptr(out), _lib.ptr(out) if want_velocity else None,
                  rows, L, _lib.stream_ptr())
        return out

    def add_noise(self, original_samples, noise, timesteps):
        return self._mix(original_samples, noise, timesteps, False)

    def get_velocity(self, sample, noise, timesteps):
        return self._mix(sample, noise, timesteps, True)

    def _apply(self, coef: _lib.StepCoef, model_output, sample, noise=None):
        _require_cuda(model_output, sample, noise)
        if model_output.dtype != torch.float32 or sample.dtype != torch.float32:
            raise TypeError("scheduler.step operates on float32 latents")
        out = sample.clone().contiguous()
        eps = model_output.contiguous()
        _lib.call("dfh_cfg_step", _lib.ptr(eps), _lib.ptr(out), None, _lib.ptr(noise), eps.numel(), CFG_NONE,
                  1.0, 1.0, 1.0, C.byref(coef), _lib.stream_ptr())
        return out


class DDIMScheduler(_SchedulerBase):
    """diffusers DDIMScheduler (timestep_spacing 'leading'), SURVEY.md Appendix B."""

    def set_timesteps(self, num_inference_steps: int, device=None):
        if num_inference_steps > self.config.num_train_timesteps:
            raise ValueError("num_inference_steps exceeds num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
        ts += self.config.steps_offset
        self._timesteps_host = ts.tolist()
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def step_coef(self, timestep: int, eta: float = 0.0) -> _lib.StepCoef:
        """Scalar coefficients of one DDIM update, in the fp32 arithmetic of the published code."""
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t = 1 - a_t
        var = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
        std = eta * var ** 0.5
        k = _lib.StepCoef()
        k.kind = STEP_DDIM
        k.vpred = 1 if self.config.prediction_type == "v_prediction" else 0
        if self.config.prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"Unknown prediction type {self.config.prediction_type}")
        k.sqrt_a_t = float(a_t ** 0.5)
        k.sqrt_b_t = float(b_t ** 0.5)
        k.sqrt_a_prev = float(a_prev ** 0.5)
        k.dir_coef = float((1 - a_prev - std ** 2) ** 0.5)
        k.std_dev = float(std)
        return k

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False,
             generator=None, variance_noise=None, return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' first")
        k = self.step_coef(timestep, eta)
        noise = None
        if eta > 0:
            noise = variance_noise
            if noise is None:
                noise = torch.randn(model_output.shape, generator=generator, device=model_output.device,
                                    dtype=model_output.dtype)
        prev = self._apply(k, model_output, sample, noise)
        return SchedulerOutput(prev_sample=prev) if return_dict else (prev,)


class PNDMScheduler(_SchedulerBase):
    """diffusers PNDMScheduler, PLMS branch (skip_prk_steps=True as in the SD config the reference
    loads at difashion.py:64).  The multistep epsilon blend is a host-ordered sequence of device
    axpy's; the transfer x' = c_x*x - c_e*eps runs in dfh_cfg_step (STEP_LINEAR)."""

    def __init__(self, *a, skip_prk_steps: bool = True, **k):
        super().__init__(*a, **k)
        if not skip_prk_steps:
            raise ValueError("only skip_prk_steps=True (PLMS) is supported")
        self.config["skip_prk_steps"] = True
        self.ets = []
        self.counter = 0
        self.cur_sample = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        base = (np.arange(0, num_inference_steps) * ratio).round() + self.config.steps_offset
        plms = np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy().astype(np.int64)
        self._timesteps_host = plms.tolist()
        self.timesteps = torch.from_numpy(plms).to(device) if device is not None else torch.from_numpy(plms)
        self.ets, self.counter, self.cur_sample = [], 0, None

    def _blend(self, terms):
        """sum_i c_i * e_i on device through the HIP linear-step kernel: x' = 1*x - (-c)*e."""
        (c0, e0), rest = terms[0], terms[1:]
        acc = None
        k = _lib.StepCoef()
        k.kind = STEP_LINEAR
        for c, e in [(c0, e0)] + list(rest):
            if acc is None:
                acc = torch.zeros_like(e)
            k.sqrt_a_t, k.sqrt_b_t = 1.0, -float(c)
            acc = self._apply(k, e, acc)
        return acc

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' first")
        t = int(timestep)
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        prev_t = t - ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_t = t
            t = t + ratio
        e = self.ets
        if len(e) == 1 and self.counter == 0:
            self.cur_sample = sample
        elif len(e) == 1 and self.counter == 1:
            model_output = self._blend([(0.5, model_output), (0.5, e[-1])])
            sample = self.cur_sample
            self.cur_sample = None
        elif len(e) == 2:
            model_output = self._blend([(1.5, e[-1]), (-0.5, e[-2])])
        elif len(e) == 3:
            model_output = self._blend([(23 / 12, e[-1]), (-16 / 12, e[-2]), (5 / 12, e[-3])])
        else:
            model_output = self._blend([(55 / 24, e[-1]), (-59 / 24, e[-2]), (37 / 24, e[-3]), (-9 / 24, e[-4])])
        k = _lib.StepCoef()
        k.kind = STEP_LINEAR
        k.sqrt_a_t, k.sqrt_b_t = self._transfer_coef(t, prev_t)
        prev = self._apply(k, model_output, sample)
        self.counter += 1
        return SchedulerOutput(prev_sample=prev) if return_dict else (prev,)

    def _transfer_coef(self, t: int, prev_t: int):
        """(c_x, c_e) of the transfer x' = c_x*x - c_e*out (diffusers _get_prev_sample) as host floats; the caller's c_float rounds them once."""
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t, b_prev = 1 - a_t, 1 - a_prev
        coeff = float((a_prev / a_t) ** 0.5)
        denom = a_t * b_prev ** 0.5 + (a_t * b_t * a_prev) ** 0.5
        c_e = float((a_prev - a_t) / denom)
        if self.config.prediction_type == "v_prediction":
            # diffusers _get_prev_sample: eps = sqrt(a_t) v + sqrt(b_t) x first, then the same transfer -- still linear in (x, v):
            # x' = (coeff - c_e sqrt(b_t)) x - c_e sqrt(a_t) v   (difashion.py:241-247 trains the v target under this setting)
            return coeff - c_e * float(b_t ** 0.5), c_e * float(a_t ** 0.5)
        if self.config.prediction_type == "epsilon":
            return coeff, c_e
        raise ValueError(f"prediction_type given as {self.config.prediction_type} must be one of `epsilon` or `v_prediction`")

    def step_plan(self, index: int):
        """Entry ``index`` of the PLMS list as ONE dfh_cfg_multistep call (what OutfitSampler launches): the filled coefficient struct and
        the pointer roles, a pure function of the index for a run that starts at entry 0.  It restates the bookkeeping of ``step``:
        entry 0 saves x and pushes its output; entry 1 pushes nothing and starts from the saved x with weights 0.5 / 0.5 over the new
        output and entry 0's; later entries push and blend the newest 2, 3, 4 outputs.  The raw outputs are blended for both prediction
        types (conv NONE); ``_transfer_coef`` folds the v-prediction into the transfer.

        roles: ``push`` = history slot (of 4) that takes the new output, or None; ``reads`` = slots of the earlier outputs, newest first,
        paired with ``coef.w[1:]``; ``x_src`` = 'latents' | 'saved'; ``x_save`` = whether x is stored to the saved-sample buffer."""
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        t = int(self._timesteps_host[index])
        prev_t = t - ratio
        k = _lib.MultistepCoef()
        k.conv, k.kind = MS_CONV_NONE, MS_PLMS
        if index == 1:
            prev_t, t = t, t + ratio
            weights, roles = (0.5, 0.5), dict(push=None, reads=[0], x_src="saved", x_save=False)
        else:
            p = 0 if index == 0 else index - 1          # this entry's push number (entry 1 pushes nothing)
            weights = PLMS_WEIGHTS[min(p, 3)]
            roles = dict(push=p % 4, reads=[(p - j) % 4 for j in range(1, len(weights))], x_src="latents", x_save=index == 0)
        k.terms = len(weights)
        for j, w in enumerate(weights):
            k.w[j] = w
        k.cx, k.ce = self._transfer_coef(t, prev_t)
        return k, roles


class DPMSolverMultistepScheduler(_SchedulerBase):
    """DPM-Solver++ multistep (2M), data-prediction form, deterministic.

    The call surface is **recalled from diffusers 0.18.2** (DPMSolverMultistepScheduler), as in SURVEY.md Appendix B: that package is not
    installed where this one is built, so the surface is restated from the published code and not pinned against it.  Supported:
    ``solver_order`` 1 | 2, ``algorithm_type='dpmsolver++'``, ``solver_type`` 'midpoint' | 'heun', ``prediction_type`` 'epsilon' |
    'v_prediction', ``lower_order_final``.  Order 3, 'dpmsolver', the 'sde-*' variants, thresholding, Karras sigmas, lambda-min clipping
    and ``prediction_type='sample'`` raise ValueError.

    ``step_plan`` derives the scalars of one update from the fp32 tables with fp32 torch scalar operations; the update itself is one
    dfh_cfg_multistep launch (conversion to x0, history difference, linear update)."""

    def __init__(self, *a, solver_order: int = 2, algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint",
                 lower_order_final: bool = True, thresholding: bool = False, use_karras_sigmas: bool = False,
                 lambda_min_clipped: float = -float("inf"), **k):
        super().__init__(*a, **k)
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order={solver_order!r}: orders 1 and 2 are supported")
        if algorithm_type != "dpmsolver++":
            raise ValueError(f"algorithm_type={algorithm_type!r}: only 'dpmsolver++' is supported")
        if solver_type not in ("midpoint", "heun"):
            raise ValueError(f"solver_type={solver_type!r}: 'midpoint' and 'heun' are supported")
        if thresholding:
            raise ValueError("thresholding=True is not supported (latent-space sampling does not use it)")
        if use_karras_sigmas:
            raise ValueError("use_karras_sigmas=True is not supported")
        if lambda_min_clipped != -float("inf"):
            raise ValueError(f"lambda_min_clipped={lambda_min_clipped!r} is not supported (no clipping of lambda)")
        if self.config.prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type={self.config.prediction_type!r}: 'epsilon' and 'v_prediction' are supported")
        self.config.update(solver_order=solver_order, algorithm_type=algorithm_type, solver_type=solver_type,
                           lower_order_final=bool(lower_order_final), thresholding=False)
        self.alpha_t = self.alphas_cumprod ** 0.5
        self.sigma_t = (1 - self.alphas_cumprod) ** 0.5
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self._reset()

    def _reset(self):
        self.model_outputs = [None, None]     # the two history slots (converted outputs); push number p writes slot p % 2
        self.lower_order_nums = 0
        self._pushes = 0

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        ts = np.linspace(0, T - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        _, first = np.unique(ts, return_index=True)
        ts = ts[np.sort(first)]                     # duplicates removed, order kept
        self.num_inference_steps = len(ts)
        self._timesteps_host = ts.tolist()
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self._reset()

    def step_index(self, timestep) -> int:
        t = int(timestep)
        return self._timesteps_host.index(t) if t in self._timesteps_host else len(self._timesteps_host) - 1

    def step_plan(self, index: int, lower_order_nums: Optional[int] = None, pushes: Optional[int] = None):
        """Step ``index`` of the timestep list as one dfh_cfg_multistep call: the filled coefficient struct and the pointer roles.
        ``lower_order_nums`` (earlier outputs available, at most solver_order) and ``pushes`` (outputs pushed so far) default to
        those of a run that started at entry 0, which makes the plan a pure function of the index.

        roles: ``push`` = history slot (of 2) that takes the converted output; ``reads`` = [slot of the previous output] for a
        second-order update, [] for a first-order one; ``x_src`` = 'latents'; ``x_save`` = False."""
        ts = self._timesteps_host
        last = index == len(ts) - 1
        if lower_order_nums is None:
            lower_order_nums = min(index, self.config.solver_order)
        if pushes is None:
            pushes = index
        s0 = ts[index]
        t = 0 if last else ts[index + 1]
        first_order = (self.config.solver_order == 1 or lower_order_nums < 1
                       or (last and self.config.lower_order_final and len(ts) < 15))
        lam, alpha, sigma = self.lambda_t, self.alpha_t, self.sigma_t
        h = lam[t] - lam[s0]
        e = alpha[t] * (torch.exp(-h) - 1.0)
        k = _lib.MultistepCoef()
        k.conv = MS_CONV_X0_V if self.config.prediction_type == "v_prediction" else MS_CONV_X0_EPS
        k.c0, k.c1 = float(alpha[s0]), float(sigma[s0])
        k.terms = 1
        k.cx, k.cd0 = float(sigma[t] / sigma[s0]), float(e)
        roles = dict(push=pushes % 2, reads=[], x_src="latents", x_save=False)
        if first_order:
            k.kind = MS_DPM1
            return k, roles
        s1 = ts[index - 1]
        r0 = (lam[s0] - lam[s1]) / h
        k.kind = MS_DPM2
        k.cr = float(1.0 / r0)
        if self.config.solver_type == "midpoint":
            k.cd1 = float(0.5 * e)
        else:
            k.cd1 = float(-(alpha[t] * ((torch.exp(-h) - 1.0) / h + 1.0)))
        roles["reads"] = [(pushes - 1) % 2]
        return k, roles

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True):
        """One solver step.  ``generator`` is accepted and ignored: the solver is deterministic."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' first")
        _require_cuda(model_output, sample)
        if model_output.dtype != torch.float32 or sample.dtype != torch.float32:
            raise TypeError("scheduler.step operates on float32 latents")
        k, roles = self.step_plan(self.step_index(timestep), self.lower_order_nums, self._pushes)
        out, x = model_output.contiguous(), sample.contiguous()
        slots = self.model_outputs
        if slots[roles["push"]] is None or slots[roles["push"]].shape != x.shape or slots[roles["push"]].device != x.device:
            slots[roles["push"]] = torch.empty_like(x)
        prev = torch.empty_like(x)
        cfg_multistep(out, x, prev, k, reads=[slots[s] for s in roles["reads"]], q_out=slots[roles["push"]])
        self._pushes += 1
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        return SchedulerOutput(prev_sample=prev) if return_dict else (prev,)
