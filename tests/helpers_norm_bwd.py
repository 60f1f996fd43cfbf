"""Inputs, fp64 references and error bounds for the normalisation backward and pointwise training kernels (tests/test_gpu_norm_bwd.py and
tests/test_gpu_pointwise.py on the GPU, tests/test_norm_bwd_inputs_cpu.py for the conditions that keep those honest).  Everything here
runs on the CPU and needs no library; G, U, FACTOR, the offset / constant inputs, the affine, the two-kernel geometry, rel and
yardstick are tests/helpers_norm.py's.

  x^ = (x - mu) rstd,  z = gamma x^ + beta,  y = silu(z) | z,  dz = dy silu'(z) | dy
  dbeta_c = sum dz,  dgamma_c = sum dz x^,  per (image, group) s1 = sum gamma dz,  s2 = sum gamma dz x^,  n = HW cpg (LayerNorm: n = C)
  dx = rstd (gamma dz - s1 / n - x^ s2 / n)

Leg A hands the kernels data on which every one of these is a small dyadic rational: a sum is then exact in fp32 in ANY order (fp32
atomics included), so a disagreement with fp64 is a wrong set of elements, not rounding.  Leg B measures what the kernels lose on
badly conditioned data (u = 2^-24):
  * dx under the evaluation rows' rule (helpers_norm.FACTOR x yardstick, MAX_REL);
  * a channel's dbeta / dgamma is a sum of N terms added along chains of at most D dependent fp32 additions (the *_depth functions):
    |err| <= (D + 4) u sum|terms| -- Higham 4.2's D u, the rounding of the product dz x^, of x^ itself (two operations) and of the
    product dy silu'(z).  The terms are the fp64 |dz| (dbeta) and |dz x^| (dgamma) of the channel.  With SiLU a term is itself a sum,
    dz = dy s + dy s z (1 - s)  (s = sigmoid(z)), whose two addends cancel towards z = -1.28: what fp32 loses on it scales with
    |dy| s (1 + |z| (1 - s)), not with |dz|, and that is the term the bound sums (equal to |dz| for z >= 0, at most 1.3 x beyond z = -3).
    Both sums are compared with fp64 ON THE OPERANDS THE KERNEL RECEIVED, the fp32 statistics among them: a mean rounded to fp32 at
    |mean| / std = 64 moves x^ of a whole group by up to 64 u, which no kernel that is handed that mean can undo and which (D + 4) u of
    five terms does not cover (tests/test_norm_bwd_inputs_cpu.py shows both); dx, at bf16 resolution, is compared with fp64 autograd."""
import functools

import torch

from tests import helpers_norm as hn

G, U = hn.G, hn.U
BF16_TINY = 2.0 ** -133            # the smallest bf16 subnormal: the spacing of bf16 below 2^-126
SENTINEL = 1232.0                  # guard rows (exact in bf16)

# ----------------------------------------------------------------------------- GroupNorm backward: (B, C0, C1, HW), G = 32
GN_CASES = [
    (1, 320, 0, 1000),             # ragged chunks: 63 chunks of 16 pixels over 6 lanes, a last chunk of 8
    (2, 128, 0, 4100),             # image index > 0, last chunk (5 pixels) shorter than PL = 16
    (1, 1280, 640, 1024),          # cpg 60: group 21 straddles the two sources
    (1, 64, 0, 5),                 # HW below PL
    (3, 1280, 768, 1),             # one pixel, a 256-thread block, one chunk
    (1, 256, 0, 1024),             # n = HW cpg = 2^13: s1 / n and s2 / n are exact
    (2, 64, 64, 64),               # two sources, n = 2^8
]
GN_POW2_CASES = [(1, 256, 0, 1024), (2, 64, 64, 64)]
GN_KINDS = ("R8", "R32", "R64", "const")
MEANS = (-1.0, 0.0, 1.0, 2.0)
RSTDS = (0.5, 1.0, 2.0)
GAMMAS = (0.5, 1.0, 2.0)


def call_forms(C1):
    """(acc0, acc1) the call-form matrix runs"""
    return [(0, 0), (1, 0), (0, 1), (1, 1)] if C1 else [(0, 0), (1, 0)]


def gn_bwd_depth(B, C, HW):
    """gn_bwd_stats_kernel, per channel: a thread adds the ceil(ppc / PL) pixels of its lane in ascending order (the four-fold unrolled
    loop keeps that order), one thread adds the PL lanes in order, and the chunks x B blocks add their sums with one atomic each (any
    order: a chain of chunks * B at the worst).  D = ceil(ppc / PL) + PL + chunks * B.  The geometry is the forward's
    (hn.two_kernel_geometry: groupnorm_bwd_launch passes the same statistics target, 512)."""
    PL, chunks, ppc = hn.two_kernel_geometry(B, C, HW)
    return -(-ppc // PL) + PL + chunks * B


def ln_rows_per_wave():
    """layernorm_bwd_kernel: a workgroup of four waves owns 64 consecutive rows, wave w takes rows w, w + 4, ..."""
    return 64 // 4


def ln_bwd_depth(M):
    """layernorm_bwd_kernel, per column: a lane adds its wave's 16 rows in order, one thread adds the four waves, and the ceil(M / 64)
    workgroups add with one atomic each.  D = 16 + 4 + ceil(M / 64)."""
    return ln_rows_per_wave() + 4 + -(-M // 64)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _ints(lo, hi, shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).to(torch.bfloat16)


def _cycle(values, n, shift=0):
    return torch.tensor([values[(i + shift) % len(values)] for i in range(n)], dtype=torch.float32)


@functools.lru_cache(maxsize=2)
def gn_exact_operands(B, C, HW):
    """Leg A.  -> dict(x, dy bf16 [B][HW][C]; gamma, beta fp32 [C]; stats fp32 [B][G][2] = (mean, rstd), HANDED to the kernel, not the
    data's own; pre bf16 [B][HW][C], the gradient contents to accumulate into).  mean cycles through -1, 0, 1, 2 and rstd through
    0.5, 1, 2 over (image, group); x = mean + integers in [-2, 2], so x^ is a multiple of 0.5 in [-4, 4]; dy integers in [-3, 3];
    gamma from 0.5, 1, 2; pre integers in [-4, 4]."""
    cpg = C // G
    mean = _cycle(MEANS, B * G).view(B, G)
    rstd = _cycle(RSTDS, B * G).view(B, G)
    x = _ints(-2, 2, (B, HW, C), 41).float() + mean.repeat_interleave(cpg, dim=1)[:, None, :]
    perm = torch.randperm(C, generator=_gen(43))
    return dict(x=x.to(torch.bfloat16), dy=_ints(-3, 3, (B, HW, C), 42), gamma=_cycle(GAMMAS, C)[perm], beta=_cycle((0.25, -0.5, 1.0, 0.0), C),
                stats=torch.stack([mean, rstd], dim=-1), pre=_ints(-4, 4, (B, HW, C), 44))


def stats64_as_fp32(x, eps):
    """the data's own (mean, rstd) from fp64, rounded to fp32: [B][G][2].  Leg B hands these over, so it measures the backward kernels'
    own error and not the forward's."""
    mean, var, _ = hn.stats64(x)
    return torch.stack([mean, (var + hn.f32(eps)).rsqrt()], dim=-1).float()


def dsilu64(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def gn_bwd64(x, dy, gamma, beta, stats, silu):
    """fp64 on the operands as the kernel receives them, the statistics included.  x, dy [B][HW][C]; stats [B][G][2].
    -> dict(dx [B][HW][C], dgamma, dbeta [C], s1, s2 [B][G], tb, tg [C] = sum|dz|, sum|dz x^|, slack [B][HW][C] =
    rstd (|gamma dz| + |s1 / n| + |x^ s2 / n|), what the fp32 roundings inside dx scale with)."""
    B, HW, C = x.shape
    cpg = C // G
    n = HW * cpg
    st = stats.double()
    mu = st[..., 0].repeat_interleave(cpg, dim=1)[:, None, :]
    rs = st[..., 1].repeat_interleave(cpg, dim=1)[:, None, :]
    ga, be = gamma.double(), beta.double()
    xh = (x.double() - mu) * rs
    dz = dy.double() * dsilu64(ga * xh + be) if silu else dy.double()
    tz = dz.abs()
    if silu:                       # the two addends of the slope, s + s z (1 - s), before they cancel (the module's docstring)
        z = ga * xh + be
        sg = torch.sigmoid(z)
        tz = dy.double().abs() * sg * (1 + z.abs() * (1 - sg))
    gdz = ga * dz
    s1 = gdz.reshape(B, HW, G, cpg).sum(dim=(1, 3))
    s2 = (gdz * xh).reshape(B, HW, G, cpg).sum(dim=(1, 3))
    m1 = (s1 / n).repeat_interleave(cpg, dim=1)[:, None, :]
    m2 = (s2 / n).repeat_interleave(cpg, dim=1)[:, None, :]
    return dict(dx=rs * (gdz - m1 - xh * m2), dgamma=(dz * xh).sum(dim=(0, 1)), dbeta=dz.sum(dim=(0, 1)), s1=s1, s2=s2,
                tb=tz.sum(dim=(0, 1)), tg=(tz * xh.abs()).sum(dim=(0, 1)), slack=rs * (gdz.abs() + m1.abs() + (xh * m2).abs()))


def gn_autograd64(x, dy, gamma, beta, eps, silu):
    """fp64 autograd of group_norm(+silu) with the fp32 eps the kernel receives -> (dx [B][HW][C], dgamma, dbeta)"""
    xin = x.double().permute(0, 2, 1).requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = torch.nn.functional.group_norm(xin, G, gr, br, hn.f32(eps))
    y = torch.nn.functional.silu(y) if silu else y
    rx, rg, rb = torch.autograd.grad(y, (xin, gr, br), dy.double().permute(0, 2, 1))
    return rx.permute(0, 2, 1).contiguous(), rg, rb


def gn_dx_fp32_kernel_order(x, dy, gamma, stats, pre=None):
    """The kernel's dx (silu = 0) in fp32, operation by operation in gn_bwd_apply_kernel's order, from fp32 sums taken in torch's order
    -> bf16.  On the exact data of a power-of-two n nothing here rounds before the last step."""
    B, HW, C = x.shape
    cpg = C // G
    mu = stats[..., 0].repeat_interleave(cpg, dim=1)[:, None, :]
    rs = stats[..., 1].repeat_interleave(cpg, dim=1)[:, None, :]
    xh = (x.float() - mu) * rs
    dz = dy.float()
    n = torch.tensor(float(HW) * float(cpg))
    s1 = (gamma * dz).reshape(B, HW, G, cpg).sum(dim=(1, 3))
    s2 = (gamma * dz * xh).reshape(B, HW, G, cpg).sum(dim=(1, 3))
    m1 = (s1 / n).repeat_interleave(cpg, dim=1)[:, None, :]
    m2 = (s2 / n).repeat_interleave(cpg, dim=1)[:, None, :]
    dx = rs * (gamma * dz - m1 - xh * m2)
    return (dx if pre is None else pre.float() + dx).to(torch.bfloat16)


def half_ulp_bf16(ref64):
    """Half the spacing of bf16 at |ref|: 2^(floor(log2 |ref|) - 8), 2^-134 below 2^-126.  As a fraction of |ref| that is 2^-9 at the top
    of a binade and 2^-8 at its bottom: 2^-9 |ref| alone would refuse a correctly rounded result in the lower half of every binade, so
    the bounds written "2^-9 |ref|" in the legs are evaluated as this, the half ulp they stand for."""
    e = torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 8)


def rounded_bound(ref64, slack):
    """|got - ref64| allowed of a bf16 result correctly rounded from fp32 arithmetic whose only rounding operands are s1 / n and s2 / n:
    half a bf16 ulp plus the fp32 roundings of the five operations of dx, each at most u of an intermediate no larger than slack / rstd."""
    return half_ulp_bf16(ref64) + 16 * U * ref64.abs() + 16 * U * slack


def sum_ratio(got, ref64, terms, depth):
    """worst |err| / ((D + 4) u sum|terms|) over the channels (0 / 0 counts as 0) and the same without the (D + 4): the measured constant"""
    err = (got.double().cpu() - ref64).abs()
    k = torch.where(terms > 0, err / (U * terms).clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return float(k.max()) / (depth + 4), float(k.max())


def const_slices(t, B, C):
    """the constant groups of the last image out of t [B][HW][C]: [HW][2][cpg]"""
    return t.reshape(t.shape[0], t.shape[1], G, C // G)[B - 1][:, list(hn.CONST_GROUPS), :]


def gn_input(case, kind):
    B, C0, C1, HW = case
    return hn.constant_input(B, C0 + C1, HW) if kind == "const" else hn.offset_input(B, C0 + C1, HW, int(kind[1:]))


def randn_bf16(shape, seed):
    return torch.randn(shape, generator=_gen(seed)).to(torch.bfloat16)


def gn_sums_fp32(x, dy, gamma, beta, stats, silu):
    """dgamma, dbeta as gn_bwd_stats_kernel defines them, sum dz x^ and sum dz, in plain fp32 with torch's sums.  (torch's own
    native_group_norm_backward forms dgamma as (sum dy x - mean sum dy) rstd, which cancels at a large |mean| / std and returns noise on a
    constant group where every x^ is exactly 0: it is not a model of a kernel that sums dz x^.)"""
    cpg = x.shape[2] // G
    mu = stats[..., 0].repeat_interleave(cpg, dim=1)[:, None, :]
    rs = stats[..., 1].repeat_interleave(cpg, dim=1)[:, None, :]
    xh = (x.float() - mu) * rs
    dz = dy.float()
    if silu:
        z = gamma * xh + beta
        s = 1.0 / (1.0 + torch.exp(-z))
        dz = dz * (s * (1.0 + z * (1.0 - s)))
    return (dz * xh).sum(dim=(0, 1)), dz.sum(dim=(0, 1))


# ----------------------------------------------------------------------------- LayerNorm backward: (M, C)
LN_CASES = [(1, 8), (37, 32), (130, 512), (65, 520), (200, 1024), (64, 1032), (70, 2048), (300, 320), (129, 1280)]
LN_POW2_WIDTHS = (8, 32, 512, 1024, 2048)
LN_EPS = 1e-5
LN_CONST_ROWS = 2


def ln_instantiation(C):
    """MAXO of the layernorm_bwd_kernel<MAXO> the launcher picks: 64 lanes x 8 columns x MAXO >= C"""
    return 1 if C <= 512 else 2 if C <= 1024 else 4


@functools.lru_cache(maxsize=2)
def ln_exact_operands(M, C):
    """Leg A, eps = 0: row r holds +a_r and -a_r in equal number (randomly permuted), a_r cycling through 1, 2, 4: mean 0, variance
    a_r^2, x^ = +-1.  dy integers in [-3, 3], gamma from 0.5, 1, 2, pre integers in [-4, 4]."""
    g = _gen(51)
    a = _cycle((1.0, 2.0, 4.0), M)
    half = torch.cat([torch.ones(C // 2), -torch.ones(C // 2)])
    x = torch.stack([half[torch.randperm(C, generator=g)] * a[r] for r in range(M)])
    return dict(x=x.to(torch.bfloat16), dy=_ints(-3, 3, (M, C), 52), gamma=_cycle(GAMMAS, C)[torch.randperm(C, generator=g)],
                pre=_ints(-4, 4, (M, C), 53), a=a)


@functools.lru_cache(maxsize=2)
def ln_offset_operands(M, C):
    """Leg B: row r is randn shifted and scaled to mean 0 and std 1 exactly, plus R_r * sign_r with R_r cycling through 8, 32, 64 and the
    sign alternating; the last two rows (when M > 2) hold 3.140625 everywhere.  -> dict(x, dy, pre bf16 [M][C], gamma fp32 [C], const = bool [M])"""
    z = torch.randn(M, C, generator=_gen(61), dtype=torch.float64)
    z = z - z.mean(dim=1, keepdim=True)
    z = z / z.pow(2).mean(dim=1, keepdim=True).sqrt()
    R = _cycle(hn.OFFSETS, M).double() * _cycle((1.0, -1.0), M).double()
    x = (z + R[:, None]).to(torch.bfloat16)
    const = torch.zeros(M, dtype=torch.bool)
    if M > LN_CONST_ROWS:
        const[M - LN_CONST_ROWS:] = True
        x[const] = hn.CONST_VALUE
    gamma, _ = hn.affine(C)
    return dict(x=x, dy=randn_bf16((M, C), 62), pre=randn_bf16((M, C), 63), gamma=gamma, const=const)


def ln_bwd64(x, dy, gamma, eps):
    """fp64 LayerNorm backward on the operands as given (eps: the fp32 value the kernel receives) -> as gn_bwd64, plus rstd [M]"""
    xd, d, ga = x.double(), dy.double(), gamma.double()
    C = xd.shape[1]
    mean = xd.mean(dim=1, keepdim=True)
    rs = ((xd - mean).pow(2).mean(dim=1, keepdim=True) + hn.f32(eps)).rsqrt()
    xh = (xd - mean) * rs
    gd = ga * d
    m1, m2 = gd.sum(dim=1, keepdim=True) / C, (gd * xh).sum(dim=1, keepdim=True) / C
    return dict(dx=rs * (gd - m1 - xh * m2), dgamma=(d * xh).sum(dim=0), dbeta=d.sum(dim=0), tb=d.abs().sum(dim=0), tg=(d * xh).abs().sum(dim=0),
                slack=rs * (gd.abs() + m1.abs() + (xh * m2).abs()), rstd=rs[:, 0], xh=xh)


def ln_dx_fp32_kernel_order(x, dy, gamma, eps, pre=None):
    """layernorm_bwd_kernel's arithmetic in fp32, operation by operation (sums in torch's order), rsqrt as torch's -> bf16"""
    xf, d = x.float(), dy.float()
    C = torch.tensor(float(xf.shape[1]))
    mean = xf.sum(dim=1, keepdim=True) / C
    q = ((xf - mean) * (xf - mean)).sum(dim=1, keepdim=True)
    rs = torch.rsqrt(q / C + eps)
    xh = (xf - mean) * rs
    gd = d * gamma
    s1, s2 = gd.sum(dim=1, keepdim=True) / C, (gd * xh).sum(dim=1, keepdim=True) / C
    dx = rs * (gd - s1 - xh * s2)
    return (dx if pre is None else pre.float() + dx).to(torch.bfloat16)


def ln_sums_fp32(x, dy, eps):
    """dgamma, dbeta as layernorm_bwd_kernel defines them, sum dy x^ and sum dy over the rows, in plain fp32 with torch's sums (torch's own
    layer_norm backward, like its group_norm's, forms dgamma from sum dy x and mean sum dy, which cancels at a large |mean| / std)"""
    xf = x.float()
    mean = xf.mean(dim=1, keepdim=True)
    rs = torch.rsqrt(((xf - mean) * (xf - mean)).mean(dim=1, keepdim=True) + eps)
    return (dy.float() * ((xf - mean) * rs)).sum(dim=0), dy.float().sum(dim=0)


def torch_fp32_ln_bwd(x, dy, gamma, eps):
    """torch's fp32 layer_norm autograd -> (dx bf16, dgamma, dbeta)"""
    xr, gr = x.float().requires_grad_(True), gamma.clone().requires_grad_(True)
    br = torch.zeros_like(gamma).requires_grad_(True)
    rx, rg, rb = torch.autograd.grad(torch.nn.functional.layer_norm(xr, (x.shape[1],), gr, br, eps), (xr, gr, br), dy.float())
    return rx.to(torch.bfloat16), rg, rb


# ----------------------------------------------------------------------------- pointwise kernels: every finite bf16 value
ACT_SILU, ACT_LEAKY, ACT_TANH = 1, 2, 3
LEAKY_SLOPE = hn.f32(0.01)         # the kernel's fp32 constant: an operand, as the reference takes it
SCALES = (1.0, 0.5, 1.0 / 3.0)
DY_CYCLE = (1.0, -3.0, 0.0625, 96.0, -2.0 ** -20)
SILU_TAIL, EXP_M32 = -87.0, torch.tensor(1.2664165549094176e-14, dtype=torch.float32)   # act_fwd_kernel's: below, sigmoid(x) = e^(x + 32) e^-32
F32_FORM = 0.75                    # the fp32 operand forms hold 0.75 x the bf16 sweep: finite everywhere, and not bf16 values
GEGLU_VALUES = (1.0, -0.375, 96.0, 2.0 ** -20)
GEGLU_DY = (1.0, -2.0, 3.0, -1.0, 2.0)
GEGLU_WIDTHS = (32, 256)
# K of the bound (2^-9 + K u)|ref| + 2^-133: the smallest power of two with which torch's fp32 CPU evaluation of the kernel's formula
# passes on the sweep (tests/test_norm_bwd_inputs_cpu.py measures it again and pins these), and 4 x that for the device, whose rcp and
# exp2 are 1-ulp each where libm's are not.  Measured CPU figures: worst (|err| - 2^-9|ref| - 2^-133) / (u |ref|).
CPU_K_FWD_MEASURED, CPU_K_FWD, K_FWD = 0.0, 1, 4          # every fp32 result rounds to bf16(fp64) itself: 2^0
CPU_K_BWD_MEASURED, CPU_K_BWD, K_BWD = 1.0658, 2, 8       # silu, scale 1/3: the product dy * scale rounds before the slope


@functools.lru_cache(maxsize=1)
def bf16_sweep():
    """all 65 280 finite bf16 bit patterns in bit order, then the first five again: 65 285 values, 5 past a multiple of 256"""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[((bits >> 7) & 0xFF) != 0xFF]
    bits = torch.cat([bits, bits[:5]])
    v = bits.to(torch.uint16).view(torch.bfloat16) if hasattr(torch, "uint16") else bits.to(torch.int16).view(torch.bfloat16)
    assert v.numel() == 65285 and bool(torch.isfinite(v.float()).all())
    return v


def cycle_like(values, n, dtype=torch.bfloat16):
    return torch.tensor(values, dtype=torch.float64)[torch.arange(n) % len(values)].to(dtype)


def act_fwd64(kind, x):
    x = x.double()
    if kind == ACT_SILU:
        return x * torch.sigmoid(x)
    if kind == ACT_LEAKY:
        return torch.where(x > 0, x, LEAKY_SLOPE * x)
    return torch.tanh(x)


def act_slope64(kind, r):
    """the slope as act_bwd_kernel defines it: silu from the pre-activation, leaky_relu and tanh from the OUTPUT"""
    r = r.double()
    if kind == ACT_SILU:
        return dsilu64(r)
    if kind == ACT_LEAKY:
        return torch.where(r > 0, 1.0, LEAKY_SLOPE).double()
    return 1 - r * r


def act_fwd_fp32(kind, x):
    """the kernel's formula in torch's fp32 on the CPU -> bf16"""
    x = x.float()
    if kind == ACT_SILU:
        y = torch.where(x < SILU_TAIL, x * torch.exp(x + 32.0) * EXP_M32, x * (1.0 / (1.0 + torch.exp(-x))))
    elif kind == ACT_LEAKY:
        y = torch.where(x > 0, x, torch.tensor(LEAKY_SLOPE, dtype=torch.float32) * x)
    else:
        y = torch.tanh(x)
    return y.to(torch.bfloat16)


def act_bwd_fp32(kind, r, dy, scale):
    r = r.float()
    d = dy.float() * torch.tensor(scale, dtype=torch.float32)
    if kind == ACT_SILU:
        s = 1.0 / (1.0 + torch.exp(-r))
        g = torch.where(r < SILU_TAIL, torch.exp(r + 32.0) * (1.0 + r) * EXP_M32, s * (1.0 + r * (1.0 - s)))
    elif kind == ACT_LEAKY:
        g = torch.where(r > 0, 1.0, LEAKY_SLOPE).float()
    else:
        g = 1.0 - r * r
    return (d * g).to(torch.bfloat16)


def act_bwd_ref64(kind, r, dy, scale):
    """fp64 on the operands the kernel receives: the scale as fp32"""
    return dy.double() * hn.f32(scale) * act_slope64(kind, r)


def measured_k(got, ref64, mask=None):
    """worst (|err| - 2^-9 |ref| - 2^-133) / (u |ref|) over the elements whose fp64 result bf16 holds as a finite number; an element the
    kernel rounded exactly as bf16(fp64) counts as 0.  -> (K, elements that are neither equal nor finite-and-comparable)"""
    got = got.double()
    rb = ref64.to(torch.bfloat16).double()
    same = (got == rb)
    err = (got - ref64).abs()
    k = (err - half_ulp_bf16(ref64) - BF16_TINY) / (U * ref64.abs()).clamp_min(1e-300)
    k = torch.where(same, torch.zeros_like(k), k)
    bad = ~same & ~torch.isfinite(k)
    if mask is not None:
        k, bad = k[mask], bad[mask]
    k = torch.where(torch.isfinite(k), k, torch.zeros_like(k))
    return float(k.max().clamp_min(0)), int(bad.sum())


def within(got, ref64, bound):
    """elementwise: the kernel's value is bf16(fp64) itself (this is what covers an infinite result), or within the bound"""
    got = got.double()
    return (got == ref64.to(torch.bfloat16).double()) | ((got - ref64).abs() <= bound)


def worst_over_bound(got, ref64, bound):
    """worst |err| / bound over the elements that are not bf16(fp64) itself (inf / nan if one of those is not comparable)"""
    got = got.double()
    same = got == ref64.to(torch.bfloat16).double()
    r = (got - ref64).abs() / bound.clamp_min(1e-300)
    r = torch.where(same, torch.zeros_like(r), r)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def gelu64(g):
    g = g.double()
    return g * 0.5 * torch.erfc(-g * 0.5 ** 0.5)


def dgelu64(g):
    g = g.double()
    return 0.5 * torch.erfc(-g * 0.5 ** 0.5) + g * torch.exp(-0.5 * g * g) * 0.3989422804014327


def geglu_rows(N2):
    """M: the sweep fills the gates of M rows of N2 / 2 gates each (the tail repeats the sweep from its start)"""
    return -(-bf16_sweep().numel() // (N2 // 2))


def geglu_operands(N2, values=GEGLU_VALUES, dys=GEGLU_DY):
    """-> (v, g, dy) bf16 [M][N2 / 2] in standard column order"""
    M, n = geglu_rows(N2), bf16_sweep().numel()
    idx = torch.arange(M * (N2 // 2))
    g = bf16_sweep()[idx % n].view(M, N2 // 2)
    return cycle_like(values, idx.numel()).view(M, N2 // 2), g, cycle_like(dys, idx.numel()).view(M, N2 // 2)


def geglu_packed_cols(N2):
    """packed column of the value and of the gate of standard column j: blocks of 16 values then 16 gates"""
    j = torch.arange(N2 // 2)
    vcol = (j // 16) * 32 + j % 16
    return vcol, vcol + 16


def geglu_row_of(n, N):
    """geglu_row of bwd_elementwise.hip: packed row of master row n of a [value | gate] parameter of N rows"""
    half = N // 2
    j = n if n < half else n - half
    return (j >> 4) * 32 + (0 if n < half else 16) + (j & 15)


# The GEGLU bounds: half a bf16 ulp, the absolute term of the approximation, and GEGLU_K u |ref| for the fp32 products around it (two or
# three roundings at u / 2 each and the library's erfc / exp at a few ulp): without the last a kernel that evaluates the exact function
# in fp32 fails wherever its last bit moves a result across a bf16 tie and the absolute term is below u |ref| (every gate above 6).
GEGLU_K = 4


def geglu_fwd_bound(v, g, ref64):
    """2^-9 |ref| + 1e-8 |v| max(1, |g|): gelu_erf_f's fit error and its clamp tail, 2^P(4 sqrt 2) ~ 7.7e-9 per unit of |g| (beyond the
    clamp the kernel returns about -7.7e-9 |g| for a negative gate where the value is -0: intended), + 2^-133 for a
    result bf16 holds as a subnormal"""
    return half_ulp_bf16(ref64) + GEGLU_K * U * ref64.abs() + 1e-8 * v.double().abs() * g.double().abs().clamp_min(1.0) + BF16_TINY


def geglu_dv_bound(d, g, ref64):
    """2^-9 |ref| + 1e-7 |d| min(|g|, 6): erf_as_f is good to 1.5e-7 absolute (halved in Phi) and saturates to +-1 exactly beyond"""
    return half_ulp_bf16(ref64) + GEGLU_K * U * ref64.abs() + 1e-7 * d.double().abs() * g.double().abs().clamp_max(6.0) + BF16_TINY


def geglu_dg_bound(d, v, ref64):
    return half_ulp_bf16(ref64) + GEGLU_K * U * ref64.abs() + 2e-7 * (d.double() * v.double()).abs() + BF16_TINY


def gelu_erf_f_fp32(x):
    """gelu_erf_f (dfh_common.h) restated in fp32 on the CPU: each fmaf as an fp64 multiply-add rounded once"""
    x = x.float()
    ax = x.abs().clamp_max(5.65685424949)
    p = torch.full_like(x, 1.917432119e-05)
    for c in (-6.586021110e-04, 7.754402186e-03, -5.296538429e-02, -4.590602584e-01, -1.151122051e+00):
        p = (p.double() * ax.double() + float(torch.tensor(c, dtype=torch.float32))).float()
    c0 = torch.tensor(3.063254510e-07, dtype=torch.float32) - 1.0
    p = (p.double() * ax.double() + float(c0)).float()
    h = x * torch.exp2(p)
    return x.clamp_min(0.0) - h.abs()


def geglu_fwd_gelu_fp32(x):
    """geglu_fwd_kernel's gelu: x / 2 * erfc(-x / sqrt 2) with the library's erfc"""
    x = x.float()
    return 0.5 * x * torch.erfc(x * -0.70710678118654752440)


def erf_as_f_fp32(x):
    """erf_as_f (dfh_common.h) in fp32 on the CPU"""
    x = x.float()
    ax = x.abs()
    t = 1.0 / (1.0 + 0.3275911 * ax)
    p = torch.full_like(x, 1.061405429)
    for c in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        p = p * t + c
    e = torch.exp2(-ax * ax * 1.44269504088896340736)
    return torch.copysign(1.0 - p * t * e, x)


def geglu_fwd_fp32(v, g):
    return (v.float() * geglu_fwd_gelu_fp32(g)).to(torch.bfloat16)


def geglu_bwd_fp32(v, g, d):
    x, v, d = g.float(), v.float(), d.float()
    cdf = 0.5 * (1.0 + erf_as_f_fp32(x * 0.70710678118654752440))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * x * x)
    return (d * (x * cdf)).to(torch.bfloat16), (d * v * (cdf + x * pdf)).to(torch.bfloat16)
