"""Inputs, fp64 references, the rounding model and the bounds of the attention parity tests (tests/test_gpu_attention_parity.py on the
GPU, tests/test_attention_inputs_cpu.py for the conditions that keep those honest).  Everything here runs on the CPU and needs no library.

Tensors are bf16 [B][N][C] with C = heads * d (head h in columns h * d .. h * d + d), as the C ABI takes them; scores, the log-sum-exp
(LSE) and every bound on them are in log2 units of the SCALED scores, c = d^-0.5 * log2(e), as the kernels report them.

Legs:
  A1  Q = 0, integer V / dO: the softmax is exactly uniform, every sum is exact in fp32 -- a disagreement is a wrong element set;
  A2  one-hot rows (Q[q] = g K[j(q)], K rows of +-1): O[q] = V[j(q)] bit for bit -- pins the query-to-key mapping of the three kernels;
  B   fp64 parity on randn data with planted aligned keys, against the rounding model below under the 3 x rule;
  C   the training walk's call forms (column slices of wider buffers) with canaries.

The model (`model`) is fp64 arithmetic with EXPLICIT roundings, written from what the kernels document about themselves:
  * the operand that carries scale * log2(e) is rounded once to bf16: Q in the 32x32 forward (attention_x32.hip header: "Q is pre-scaled
    by scale * log2(e)"), in the 16x16 forward when it reports an LSE at d = 40 / 80 (attention.hip `prescale`) and in the dQ pass at
    d = 40 / 80, K in the dK / dV pass at d = 40 / 80 (attention_bwd.hip, PADS), Q in both passes at d = 64 behind the 32x32 forward
    (attention_bwd.hip, QSC: dK is then formed from the rounded Q); the 16x16 forward and the backward of the other head dims scale the
    fp32 score instead (attention.hip: "the scale c is folded into the exp2 argument");
  * P, unnormalised against the row maximum, is rounded to bf16 ahead of P V; the denominator adds the ROUNDED P where it comes out of
    the ones row of V^T or its v_dot2 stand-in (attention.hip ONES_ROW: d % 16 != 0; attention_x32_steps.h LSUM comment: every d of the
    32x32 kernel), the unrounded fp32 P elsewhere;
  * the backward rounds the normalised P and dS to bf16 ahead of their products; at d = 40 / 80 -lse and -delta ride in two bf16
    contraction slots each (attention_bwd.hip split2: 16 mantissa bits);
  * the outputs are rounded to bf16; the LSE comes from the rounded scores;
  * scores, P, the denominator, its log2 and the LSE are rounded to fp32 where the kernels hold them in fp32 (one rounding per 16- or
    32-deep MFMA step for the scores): the precision of the format, which is all that separates the 16x16 forward's LSE from fp64."""
import functools
import math

import torch

LOG2E = 1.4426950408889634
B, HEADS = 2, 2
FACTOR = 3.0                       # the evaluation rows' rule and helpers_norm.output_ok: measured <= FACTOR x the model's own error
U_BF16 = 2.0 ** -8                 # the unit taken for one bf16 rounding in the elementwise LSE bound
GAP = 40.0                         # leg A2: the selected score leads its row by this many log2 units
LEAK = 2.0 ** -39                  # ... so no other key's P exceeds this in the kernels' arithmetic (the bf16 scale may take 2^-8 of the gap)
X32, K16 = "attention_x32", "attention_16"          # census keys of the two forward kernels

# ----------------------------------------------------------------------------- the cases: (d, Nq, Nk), B = 2, heads = 2
# 32x32 forward WITH an LSE pointer (the short-key kernel takes no LSE): one key tile, a second tile of one key, the text length, two
# full tiles, a third tile of one key, a later ragged tile; d = 64 is eligible from 1024 x 1024 on only
X32_CASES = [(d, nq, nk) for d in (40, 80) for nq in (256, 300) for nk in (64, 65, 77, 128, 129, 200)] + [(64, 1024, 1024)]
K16_CASES = [(d, nq, nk) for d in (32, 40, 64, 80, 128, 160) for nq, nk in ((4, 4), (65, 63), (200, 77), (129, 127))]
# the backward streams 64-row tiles; a workgroup owns 128 columns (64 in the dK / dV pass at d > 80): every value on each side
BWD_PAIRS = [(63, 129), (64, 128), (65, 127), (127, 65), (128, 64), (129, 63)]
BWD_CASES = [(d, nq, nk) for d in (40, 80, 160) for nq, nk in BWD_PAIRS]
ALL_CASES = X32_CASES + K16_CASES + BWD_CASES
CONSISTENCY_CASES = [(d, nk) for d in (40, 80) for nk in (64, 65, 77, 128, 129, 200)]      # x32 at Nq = 256 against 16x16 at Nq = 200
DATA_KINDS = ("randn", "aligned", "gain2", "gain4")                                      # leg B; gain4 is printed, not bounded


def case_id(c):
    return "x".join(str(v) for v in c)


def forward_kernel(d, nq, nk):
    """the census key dfh_attention_lse bumps at this shape (attention_x32.hip attention_x32_eligible)"""
    if d == 64:
        return X32 if nq >= 1024 and nk >= 1024 else K16
    return X32 if d in (40, 80) and nq >= 256 and nk >= 64 else K16


def pads(d):
    """attention_bwd.hip PADS: head dims whose 32-deep contraction steps leave a free 8-slot chunk"""
    return d in (40, 80)


def scale_of(d):
    """d^-0.5 as the fp32 the C ABI receives"""
    return float(torch.tensor(d ** -0.5, dtype=torch.float32))


def c_of(d):
    """scale * log2(e) as the kernels form it in fp32"""
    return float(torch.tensor(scale_of(d), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


# ----------------------------------------------------------------------------- inputs (seeded, CPU, bf16 [B][N][C])
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _seed(case, salt):
    d, nq, nk = case
    return salt * 1000003 + d * 10007 + nq * 101 + nk


def _integers(shape, seed, cap=64):
    """integers from {+-1, +-2, +-3}, never 0, whose sum over dim 1 stays within +-cap in every (batch, channel): elements of the sign
    of an oversized sum are negated in index order (one bf16 ulp of a mean is then less than one unit of its sum, see the CPU test)"""
    g = _gen(seed)
    x = torch.randint(1, 4, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    for _ in range(64):
        s = x.sum(dim=1, keepdim=True)
        big = s.abs() > cap
        if not bool(big.any()):
            break
        same = (torch.sign(x) == torch.sign(s)) & big
        first = same & (same.cumsum(dim=1) <= ((s.abs() - cap // 2) // 6).clamp(min=1))
        x = torch.where(first, -x, x)
    return x.to(torch.bfloat16)


@functools.lru_cache(maxsize=4)
def uniform_input(case):
    """Leg A1 -> (q = 0, k randn, v, do integers)"""
    d, nq, nk = case
    C = HEADS * d
    k = torch.randn(B, nk, C, generator=_gen(_seed(case, 1))).to(torch.bfloat16)
    return (torch.zeros(B, nq, C, dtype=torch.bfloat16), k, _integers((B, nk, C), _seed(case, 2)), _integers((B, nq, C), _seed(case, 3)))


def selected_key(nq, nk):
    """j(q) = (7 q + 3) mod Nk"""
    return (7 * torch.arange(nq) + 3) % nk


@functools.lru_cache(maxsize=4)
def one_hot_input(case):
    """Leg A2 -> (q, k, v, do, g): K rows of random +-1 per head, Q[q] = g K[j(q)], g the smallest power of two for which the selected
    score leads every other score of its row by GAP log2 units in fp64 (every batch element and head)."""
    d, nq, nk = case
    C = HEADS * d
    k = (torch.randint(0, 2, (B, nk, C), generator=_gen(_seed(case, 4))) * 2 - 1).double()
    j = selected_key(nq, nk)
    kh = heads_view(k, d)
    dots = kh[:, :, j, :] @ kh.transpose(-1, -2)                                           # [B][H][Nq][Nk]
    lead = d - dots.masked_fill(torch.nn.functional.one_hot(j, nk).bool(), -math.inf).amax(dim=-1)
    g = 1.0
    while g * c_of(d) * float(lead.min()) < GAP and g < 2 ** 20:
        g *= 2
    q = g * k[:, j, :]
    return (q.to(torch.bfloat16), k.to(torch.bfloat16), _integers((B, nk, C), _seed(case, 5)), _integers((B, nq, C), _seed(case, 6)), g)


def planted(case):
    """Leg B: [(query, key)] -- one aligned key per 64 queries, in the last 64-key tile (as many as that tile has keys)"""
    d, nq, nk = case
    tail0 = (nk - 1) // 64 * 64
    blocks = (nq + 63) // 64
    return [(min(64 * i + 5, nq - 1), nk - 1 - i) for i in range(min(blocks, nk - tail0))]


@functools.lru_cache(maxsize=4)
def hard_input(case, kind):
    """Leg B -> (q, k, v, do).  randn: gain 1.  aligned: the same with k[key] = 3 q[query] for the planted pairs (all heads).
    gain2 / gain4: q and k times 2 / 4, then the planted keys."""
    d, nq, nk = case
    C = HEADS * d
    gain = {"randn": 1.0, "aligned": 1.0, "gain2": 2.0, "gain4": 4.0}[kind]
    g = _gen(_seed(case, 7))
    q = (torch.randn(B, nq, C, generator=g) * gain).to(torch.bfloat16)
    k = (torch.randn(B, nk, C, generator=g) * gain).to(torch.bfloat16)
    v = torch.randn(B, nk, C, generator=g).to(torch.bfloat16)
    do = torch.randn(B, nq, C, generator=g).to(torch.bfloat16)
    if kind != "randn":
        for qi, ki in planted(case):
            k[:, ki] = (q[:, qi].float() * 3.0).to(torch.bfloat16)
    return q, k, v, do


# ----------------------------------------------------------------------------- fp64 references
def heads_view(t, d):
    """[B][N][C] -> fp64 [B][H][N][d]"""
    b, n, C = t.shape
    return t.double().view(b, n, C // d, d).transpose(1, 2)


def flat(t):
    """[B][H][N][d] -> [B][N][C]"""
    b, h, n, d = t.shape
    return t.transpose(1, 2).reshape(b, n, h * d)


def scores64(q, k, d):
    """fp64 scaled scores in log2 units [B][H][Nq][Nk]"""
    return heads_view(q, d) @ heads_view(k, d).transpose(-1, -2) * (d ** -0.5 * LOG2E)


def lse2(s):
    return torch.logsumexp(s * math.log(2.0), dim=-1) / math.log(2.0)


def ref64(q, k, v, do, d):
    """fp64 softmax attention and fp64 autograd of it on the operands as given -> dict(lse [B][H][Nq] log2 units, o, dq, dk, dv [B][N][C])"""
    qh, kh, vh = (heads_view(t, d).detach().requires_grad_(True) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * d ** -0.5
    o = torch.softmax(s, dim=-1) @ vh
    gq, gk, gv = torch.autograd.grad(o, (qh, kh, vh), heads_view(do, d))
    return dict(lse=lse2(s.detach() * LOG2E), o=flat(o.detach()), dq=flat(gq), dk=flat(gk), dv=flat(gv))


def lse_bound(q, k, d):
    """[B][H][Nq]: 2^-8 (max_j sum_i |q_i k_i| c + 2).  One bf16 rounding per operand element moves a score by at most u sum_i |q_i k_i| c
    (u = 2^-8 taken for the unit), and the LSE moves by no more than the largest score shift; + 2 covers the bf16-rounded P in the
    denominator (relative 2^-9: 2^-9 log2(e) log2 units) and the fp32 exp / log."""
    a = heads_view(q, d).abs() @ heads_view(k, d).abs().transpose(-1, -2)
    return U_BF16 * (a.amax(dim=-1) * (d ** -0.5 * LOG2E) + 2.0)


# ----------------------------------------------------------------------------- the rounding model
def r32(x):
    return x.float().double()


def rbf(x):
    """fp32, then bf16 (the kernels pack fp32 registers)"""
    return x.float().to(torch.bfloat16).double()


def split16(x):
    """attention_bwd.hip split2: v ~ hi + lo, both bf16"""
    hi = rbf(x)
    return hi + rbf(r32(x - hi))


def dot32(a, b, step):
    """a [..][M][d] . b [..][N][d]^T accumulated in fp32 over `step`-deep MFMA steps (one rounding per step)"""
    acc = torch.zeros(a.shape[:-1] + (b.shape[-2],), dtype=torch.float64)
    for i in range(0, a.shape[-1], step):
        acc = r32(acc + a[..., i:i + step] @ b[..., i:i + step].transpose(-1, -2))
    return acc


def model(q, k, v, do, d, kernel):
    """The stated roundings (module docstring) in fp64 -> the same dict as ref64.  kernel: the forward kernel's census key."""
    qh, kh, vh, gh = (heads_view(t, d) for t in (q, k, v, do))
    scale, c = scale_of(d), c_of(d)
    # ---- forward
    if kernel == X32:
        s = dot32(rbf(r32(qh * c)), kh, 16)
    elif pads(d):                                                # attention.hip `prescale`: with an LSE pointer at d = 40 / 80
        s = dot32(rbf(r32(qh * c)), kh, 32)
    else:
        s = r32(dot32(qh, kh, 32) * c)
    m = s.amax(dim=-1, keepdim=True)
    p = r32(torch.exp2(s - m))
    pb = rbf(p)
    den_rounded = kernel == X32 or d % 16 != 0
    den = r32((pb if den_rounded else p).sum(dim=-1, keepdim=True))
    lse = r32(m + r32(torch.log2(den))).squeeze(-1)
    o = rbf(r32(pb @ vh) * r32(1.0 / den))
    # ---- backward: delta from the bf16 O, P recomputed against the forward's LSE
    delta = r32((gh * o).sum(dim=-1))
    dp = r32(gh @ vh.transpose(-1, -2))
    k_scale = scale                                               # what dK = dS^T Q is multiplied by at the store
    if pads(d):
        L, Dl = split16(lse).unsqueeze(-1), split16(delta).unsqueeze(-1)
        s_q = r32(dot32(rbf(r32(qh * c)), kh, 32) - L)            # dQ pass: Q carries the scale
        s_k = r32(dot32(qh, rbf(r32(kh * c)), 32) - L)            # dK / dV pass: K carries it
    elif d == 64 and kernel == X32:                               # attention_bwd.hip QSC: both passes take the forward's rounded Q
        L, Dl = lse.unsqueeze(-1), delta.unsqueeze(-1)
        qh = rbf(r32(qh * c))
        s_q = s_k = r32(dot32(qh, kh, 32) - L)
        k_scale = float(torch.tensor(scale, dtype=torch.float32) / torch.tensor(c, dtype=torch.float32))
    else:
        L, Dl = lse.unsqueeze(-1), delta.unsqueeze(-1)
        s_q = s_k = r32(dot32(qh, kh, 32) * c - L)
    p_q, p_k = r32(torch.exp2(s_q)), r32(torch.exp2(s_k))
    ds_q, ds_k = rbf(r32(p_q * r32(dp - Dl))), rbf(r32(p_k * r32(dp - Dl)))
    dq = rbf(r32(ds_q @ kh) * scale)
    dk = rbf(r32(ds_k.transpose(-1, -2) @ qh) * k_scale)
    dv = rbf(r32(rbf(p_k).transpose(-1, -2) @ gh))
    return dict(lse=lse, o=flat(o), dq=flat(dq), dk=flat(dk), dv=flat(dv), rowsum=p_k.sum(dim=-1))


# ----------------------------------------------------------------------------- figures
def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


def max_rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def yardstick(ref):
    """rel L2 between the fp64 result rounded once to bf16 and itself: what a perfect kernel's output is off by"""
    return rel(ref.to(torch.bfloat16), ref)


def rms(x):
    return float(x.double().pow(2).mean().sqrt())


def bf16_ulp(v):
    """the spacing of bf16 at |v| (fp64 tensor; the smallest normal's spacing at 0)"""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - 7)


def one_hot_dv(do, nq, nk):
    """Leg A2 -> (want, allowance): want[j] = the exact integer sum of the dO rows that select j; the allowance on |dV - want| is one bf16
    ulp where want != 0.  Where want == 0 (no query selects j, or the selected rows cancel) no ulp exists, and exact arithmetic does
    not give 0 either (fp64 autograd leaves up to 1e-12 there: every other query contributes P dO with P <= 2^-40): the allowance is
    that leak, 3 Nq LEAK, plus the fp32 accumulation of the n_j selected rows, (n_j + 1) 2^-24 sum |dO| (the MFMA aligns its addends to
    the largest and truncates: a negative leak of 1e-13 beside partial sums of 2 .. 4 comes back as -2^-23)."""
    j = selected_key(nq, nk)
    want = torch.zeros(do.shape[0], nk, do.shape[2], dtype=torch.float64).index_add_(1, j, do.double())
    mag = torch.zeros_like(want).index_add_(1, j, do.double().abs())
    n_j = torch.zeros(nk, dtype=torch.float64).index_add_(0, j, torch.ones(nq, dtype=torch.float64)).view(1, nk, 1)
    zero_allow = 3.0 * nq * LEAK + (n_j + 1) * 2.0 ** -24 * mag
    return want, torch.where(want != 0, bf16_ulp(want), zero_allow)


def ulps(got, want):
    """largest |got - want| in bf16 ulps of want"""
    return float(((got.double() - want).abs() / bf16_ulp(want)).max())


@functools.lru_cache(maxsize=4)
def hard_reference(case, kind):
    """Leg B: (fp64 reference, model, elementwise LSE bound) of hard_input(case, kind), computed once"""
    d = case[0]
    q, k, v, do = hard_input(case, kind)
    return ref64(q, k, v, do, d), model(q, k, v, do, d, forward_kernel(*case)), lse_bound(q, k, d)


def parity_figures(got, ref, mdl, bound):
    """got: dict(lse, o, dq, dk, dv) of CPU tensors -> dict of figures: lse_max (worst |err| / elementwise bound), lse_abs (worst |err|),
    lse_rms, lse_rms_model, and per output x in (o, dq, dk, dv): x (rel L2), x_model, x_yard, x_max (max |err| / max |ref|), finite"""
    e = (got["lse"].double() - ref["lse"]).abs()
    f = dict(lse_max=float((e / bound).max()), lse_abs=float(e.max()), lse_rms=rms(e), lse_rms_model=rms(mdl["lse"] - ref["lse"]),
             lse_model_max=float(((mdl["lse"] - ref["lse"]).abs() / bound).max()),
             finite=all(bool(torch.isfinite(got[x].float()).all()) for x in ("lse", "o", "dq", "dk", "dv")))
    for x in ("o", "dq", "dk", "dv"):
        f[x], f[x + "_model"], f[x + "_yard"], f[x + "_max"] = rel(got[x], ref[x]), rel(mdl[x], ref[x]), yardstick(ref[x]), max_rel(got[x], ref[x])
    return f


def parity_ok(f):
    """the bounded part of leg B: elementwise LSE bound, LSE rms and every rel L2 within FACTOR x the model's (equivalently: the ratio
    to the single-rounding yardstick within FACTOR x the model's own ratio), everything finite"""
    return (f["finite"] and f["lse_max"] <= 1.0 and f["lse_rms"] <= FACTOR * f["lse_rms_model"] and
            all(f[x] <= FACTOR * f[x + "_model"] for x in ("o", "dq", "dk", "dv")))


def legacy_ok(f):
    """gain-1 randn data: the bounds of test_attention / test_attention_backward, unchanged"""
    return (f["lse_abs"] < 2e-2 and f["o"] <= 1e-2 and f["o_max"] <= 4e-2 and
            all(f[x] <= 1.5e-2 and f[x + "_max"] <= 6e-2 for x in ("dq", "dk", "dv")))
