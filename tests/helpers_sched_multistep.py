"""Restatement of the multistep sampler step (dfh_cfg_multistep, PLMS, DPM-Solver++ 2M) in plain torch, with a ``dtype`` argument
for fp32 and fp64.  It is written from the formulas of the design ("Fused multistep sampler step"), not from the product
code: tables, timestep list, per-step scalars, conversion, update, and the closed-form Gaussian test problem.

Every scalar is a 0-d torch tensor of ``dtype`` and every product and sum is an op of its own, so in fp32 the results are what a
kernel without fused multiply-adds gives, bit for bit."""
import ctypes as C

import numpy as np
import torch

from oracle import glue_ref

T = 1000
MODES = ["none", "full", "cate_hist", "cate_mutual", "cate", "hist", "mutual"]     # CFG mode codes 0..6 of the C ABI, in order
BRANCHES = {"none": 1, "full": 4, "cate_hist": 3, "cate_mutual": 3, "cate": 2, "hist": 2, "mutual": 2}
CONV_NONE, CONV_X0_EPS, CONV_X0_V = 0, 1, 2
PLMS, DPM1, DPM2 = 0, 1, 2
PLMS_W = {1: [1.0], 2: [1.5, -0.5], 3: [23 / 12, -16 / 12, 5 / 12], 4: [55 / 24, -59 / 24, 37 / 24, -9 / 24]}


def tables(dtype):
    """The Stable Diffusion schedule (scaled_linear, 0.00085 .. 0.012, 1000 steps): alphas_cumprod, alpha_t, sigma_t, lambda_t."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, T, dtype=dtype) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0)
    alpha, sigma = ac ** 0.5, (1 - ac) ** 0.5
    return dict(ac=ac, alpha=alpha, sigma=sigma, lam=torch.log(alpha) - torch.log(sigma))


def timesteps(n):
    ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].astype(np.int64).tolist()
    out = []
    for t in ts:                    # duplicates removed, order kept
        if t not in out:
            out.append(t)
    return out


def dpm_coef(tab, ts, i, *, have_history, solver_order=2, solver_type="midpoint", prediction_type="epsilon", lower_order_final=True):
    """Scalars of step i of the list ``ts``: dict(conv, kind, c0, c1, cx, cd0, cr, cd1), 0-d tensors of the tables' dtype."""
    lam, alpha, sigma = tab["lam"], tab["alpha"], tab["sigma"]
    last = i == len(ts) - 1
    s0, t = ts[i], (0 if last else ts[i + 1])
    first = solver_order == 1 or not have_history or (last and lower_order_final and len(ts) < 15)
    h = lam[t] - lam[s0]
    e = alpha[t] * (torch.exp(-h) - 1.0)
    zero = torch.zeros((), dtype=lam.dtype)
    k = dict(conv=CONV_X0_V if prediction_type == "v_prediction" else CONV_X0_EPS, kind=DPM1 if first else DPM2,
             c0=alpha[s0], c1=sigma[s0], cx=sigma[t] / sigma[s0], cd0=e, cr=zero, cd1=zero)
    if not first:
        s1 = ts[i - 1]
        r0 = (lam[s0] - lam[s1]) / h
        k["cr"] = 1.0 / r0
        k["cd1"] = 0.5 * e if solver_type == "midpoint" else -(alpha[t] * ((torch.exp(-h) - 1.0) / h + 1.0))
    return k


def _s(v, dtype):
    return v.to(dtype) if torch.is_tensor(v) else torch.tensor(v, dtype=torch.float32).to(dtype)    # a host float enters as the C float


def convert(k, m, x):
    dt = x.dtype
    if k["conv"] == CONV_X0_EPS:
        return (x - _s(k["c1"], dt) * m) / _s(k["c0"], dt)
    if k["conv"] == CONV_X0_V:
        return _s(k["c0"], dt) * x - _s(k["c1"], dt) * m
    return m


def update(k, x, q, hist):
    """x' of the update; ``hist`` = earlier converted outputs, newest first."""
    dt = x.dtype
    if k["kind"] == PLMS:
        b = _s(k["w"][0], dt) * q
        for j in range(1, k["terms"]):
            b = b + _s(k["w"][j], dt) * hist[j - 1]
        return _s(k["cx"], dt) * x - _s(k["ce"], dt) * b
    y = _s(k["cx"], dt) * x - _s(k["cd0"], dt) * q
    if k["kind"] == DPM2:
        d1 = _s(k["cr"], dt) * (q - hist[0])
        y = y - _s(k["cd1"], dt) * d1
    return y


def combine(mode, out_all, scales):
    """Guidance combine of the stacked branch outputs [R*B, ...] (difashion.py:525-566, the oracle's restatement)."""
    sc, sh, sm = scales
    return glue_ref.cfg_combine(mode, out_all, sc, sh, sm)


def multistep(mode, out_all, x, k, hist, scales=(1.0, 1.0, 1.0)):
    """One whole dfh_cfg_multistep call: (m, q, x')."""
    m = combine(mode, out_all, scales)
    q = convert(k, m, x)
    return m, q, update(k, x, q, hist)


def dpm_trajectory(outputs, x_T, n, dtype, **cfg):
    """The solver's own step loop over the fixed output sequence ``outputs`` (one per step): the list of x after every step."""
    tab, ts = tables(dtype), timesteps(n)
    x, prev_q, xs = x_T.to(dtype), None, []
    for i in range(len(ts)):
        k = dpm_coef(tab, ts, i, have_history=prev_q is not None, **cfg)
        q = convert(k, outputs[i].to(dtype), x)
        x = update(k, x, q, [prev_q])
        prev_q = q
        xs.append(x)
    return xs


# ---- closed form: data N(mu, s^2) per element
def gaussian_problem():
    rng = np.random.default_rng(0)
    mu = 0.5 * rng.normal(size=64)
    s = 0.3 + rng.random(64)
    x_T = rng.normal(size=64)
    return tuple(torch.from_numpy(v) for v in (mu, s, x_T))


def exact_eps(tab, t, x, mu, s):
    a, sg = tab["alpha"][t], tab["sigma"][t]
    return sg * (x - a * mu) / (a ** 2 * s ** 2 + sg ** 2)


def exact_x(tab, t, t_start, x_T, mu, s):
    a, sg, A, S = tab["alpha"][t], tab["sigma"][t], tab["alpha"][t_start], tab["sigma"][t_start]
    return a * mu + (x_T - A * mu) * torch.sqrt(a ** 2 * s ** 2 + sg ** 2) / torch.sqrt(A ** 2 * s ** 2 + S ** 2)


def solve_gaussian(n, solver_order, upto_last_entry=True):
    """fp64 solver run on the Gaussian problem with the exact epsilon; returns (x at the entry of the last step, t there, t_start)."""
    tab, ts = tables(torch.float64), timesteps(n)
    mu, s, x = gaussian_problem()
    prev_q = None
    for i in range(len(ts) - 1 if upto_last_entry else len(ts)):
        k = dpm_coef(tab, ts, i, have_history=prev_q is not None, solver_order=solver_order)
        q = convert(k, exact_eps(tab, ts[i], x, mu, s), x)
        x = update(k, x, q, [prev_q])
        prev_q = q
    return x, ts[-1], ts[0]


def ddim_step(tab, t, t_prev, x, eps):
    """DDIM, eta = 0, from t to t_prev on the same tables."""
    a_t, a_p = tab["ac"][t], tab["ac"][t_prev]
    x0 = (x - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
    return a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * eps


# ---- kernel cases of the GPU tests (tests/test_gpu_sched_multistep.py and its fp16-storage child process)
SENTINEL = -12345.0
GUARD = 64                       # floats on either side of every device buffer: a multiple of 4, so the 16-byte path stays reachable
SCALES = (12.0, 4.0, 5.0)
# conversions x kinds the kernel knows: (conv, kind, terms)
COMBOS = [(conv, kind, terms) for conv in (CONV_NONE, CONV_X0_EPS, CONV_X0_V)
          for kind, terms in ((PLMS, 1), (PLMS, 2), (PLMS, 3), (PLMS, 4), (DPM1, 1), (DPM2, 1))]


def kernel_coef(conv, kind, terms):
    """Fixed coefficients of the size the schedulers produce, already rounded to fp32 (what the C struct holds)."""
    r = lambda v: float(np.float32(v))
    return dict(conv=conv, kind=kind, terms=terms, c0=r(0.8317), c1=r(0.5552), w=[r(v) for v in PLMS_W[terms]] + [0.0] * (4 - terms),
                cx=r(1.0173), ce=r(0.0419), cd0=r(-0.2371), cr=r(0.9683), cd1=r(-0.1186))


def kernel_inputs(shape, mode, seed):
    """(out_all [R*B, C, H, W], x, [h1, h2, h3]) as CPU fp32 tensors."""
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    out_all = torch.randn((BRANCHES[mode] * B,) + tuple(shape[1:]), generator=g)
    x = torch.randn(shape, generator=g)
    return out_all, x, [torch.randn(shape, generator=g) for _ in range(3)]


def coef_struct(k):
    from difashion_amd import _lib
    c = _lib.MultistepCoef()
    c.conv, c.kind, c.terms = k["conv"], k["kind"], k["terms"]
    for name in ("c0", "c1", "cx", "ce", "cd0", "cr", "cd1"):
        setattr(c, name, float(k[name]))
    for j in range(4):
        c.w[j] = float(k["w"][j])
    return c


def run_kernel(mode, out_all, x, hist, k, *, taps=(True, True, True), in_place=True, misalign=0, dev="cuda"):
    """One dfh_cfg_multistep call on guarded device buffers -> dict(lat, m, q, x_save) of CPU tensors (None where the tap was not
    given).  Asserts that every guard word, and every tap buffer that was not passed, still holds the sentinel."""
    from difashion_amd import _lib
    n, G = x.numel(), GUARD + misalign
    bufs = []

    def guarded(src=None, count=n):
        buf = torch.full((count + 2 * G,), SENTINEL, dtype=torch.float32, device=dev)
        view = buf[G:G + count]
        if src is not None:
            view.copy_(src.flatten())
        bufs.append((buf, count))
        return view

    d_out = guarded(out_all, out_all.numel())
    d_x = guarded(x)
    d_lat = d_x if in_place else guarded()
    need = k["terms"] - 1 if k["kind"] == PLMS else (1 if k["kind"] == DPM2 else 0)
    d_h = [guarded(hist[j]) if j < need else None for j in range(3)]
    d_m, d_q, d_s = guarded(), guarded(), guarded()
    given = [b if t else None for b, t in zip((d_m, d_q, d_s), taps)]
    sc, sh, sm = SCALES
    _lib.call("dfh_cfg_multistep", _lib.ptr(d_out), _lib.ptr(d_x), _lib.ptr(d_lat), _lib.ptr(given[0]), _lib.ptr(given[1]), _lib.ptr(given[2]),
              _lib.ptr(d_h[0]), _lib.ptr(d_h[1]), _lib.ptr(d_h[2]), n, MODES.index(mode), sc, sh, sm, C.byref(coef_struct(k)), _lib.stream_ptr())
    torch.cuda.synchronize()
    for buf, count in bufs:
        assert bool((buf[:G] == SENTINEL).all()) and bool((buf[G + count:] == SENTINEL).all()), "a guard word was overwritten"
    for b, t in zip((d_m, d_q, d_s), taps):
        assert t or bool((b == SENTINEL).all()), "a tap that was not given was written"
    assert torch.equal(d_out.cpu(), out_all.flatten()), "the model outputs were modified"
    shape = x.shape
    res = [None if g is None else g.cpu().reshape(shape) for g in given]
    return dict(lat=d_lat.cpu().reshape(shape), m=res[0], q=res[1], x_save=res[2])


def check_kernel_case(mode, shape, conv, kind, terms, *, seed, taps=(True, True, True), in_place=True, misalign=0):
    """Kernel against the fp32 restatement, bit for bit.  Returns the kernel's result dict."""
    out_all, x, hist = kernel_inputs(shape, mode, seed)
    k = kernel_coef(conv, kind, terms)
    got = run_kernel(mode, out_all, x, hist, k, taps=taps, in_place=in_place, misalign=misalign)
    m, q, y = multistep(mode, out_all, x, k, hist, SCALES)
    what = (mode, tuple(shape), conv, kind, terms, taps, in_place, misalign)
    assert torch.equal(got["lat"], y), what
    for name, want in (("m", m), ("q", q), ("x_save", x)):
        assert got[name] is None or torch.equal(got[name], want), (name,) + what
    return got
