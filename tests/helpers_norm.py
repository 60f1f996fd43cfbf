"""Inputs, fp64 references and error bounds for the GroupNorm statistics tests (tests/test_gpu_norm_stats.py on the GPU,
tests/test_norm_inputs_cpu.py for the conditions that keep those honest).  Everything here runs on the CPU and needs no library.

The four GroupNorm paths (norm.hip gn_select) do not compute the variance the same way: the one-slab kernel, the group-quad kernel
and the Winograd prologue centre the values on the mean first (two passes), the two-kernel path and the producer statistics carry raw
(sum, sum of squares) records and form  sum(x^2) / n - mean^2  in fp32 (one pass).  The one-pass difference cancels: its relative
error grows with  kappa = 1 + R^2,  R = |group mean| / group std.  The inputs below set R; the bounds below say what each path may
lose at that R.

Bounds (u = 2^-24, the fp32 unit roundoff):
  * a sum of n non-negative terms added along chains of at most D dependent fp32 additions has relative error <= D u (Higham, Accuracy
    and Stability of Numerical Algorithms, 4.2); with the rounding of each square and of the division  q / n  is off by (D + 2) u (q / n),
    and q / n = kappa var.  The tests hold the variance  q / n - mean^2  to  2 (D + 4) u kappa var:  twice that chain plus the roundings of
    mean^2, the subtraction and + eps.  (Every worst case at once -- the sum behind the mean off by its full D u as well, against the sign
    of the error of q -- would allow (3 D + 5) u kappa; the narrower figure is the one asserted.)
  * a two-pass path sums (x - mean)^2, non-negative terms again, with nothing left to cancel: the same bound with kappa = 1;
  * the mean is a sum of at most n terms of size <= max|x| over n: |mean - mean64| <= (D + 2) u max|x|.
D is the longest chain the path's documented summation order allows (the *_depth functions, each with its derivation)."""
import functools
import math

import torch

G = 32
U = 2.0 ** -24
TINY = 2.0 ** -149
FACTOR = 3.0                       # the evaluation rows' rule (tests/test_gpu_eval_scores.py): measured <= FACTOR x the reference's own rounding
MAX_REL = 2e-2                     # of max|ref|: test_groupnorm_silu's
OFFSETS = (8, 32, 64)              # R; at 64 bf16 data runs out (4-5 distinct levels per sigma)
CONST_VALUE = 3.140625             # 201 / 64, exact in bf16
CONST_GROUPS = (0, 17)
ONE_PASS = ("gn_stats", "gn_pre")  # census keys of the paths that form sum(x^2) / n - mean^2


def f32(v: float) -> float:
    """v as the fp32 the C ABI receives (eps)."""
    return float(torch.tensor(v, dtype=torch.float32))


# ----------------------------------------------------------------------------- the cases: (B, C0, C1, HW), G = 32 throughout
# two-kernel path (gn_stats + apply).  B = 1 keeps a shape on it whatever its size (the one-slab kernel wants B * G >= 64 blocks, the
# group-quad kernel 128).
TWO_KERNEL_CASES = [
    (1, 320, 0, 4096),             # 64 chunks of 64 pixels, PL = 6
    (1, 320, 0, 1000),             # ragged: chunks of 16 pixels over 6 lanes, a short last chunk of 8
    (1, 128, 0, 2470),             # cpg 4, PL = 16, ragged (39-pixel chunks, 13 in the last)
    (2, 128, 0, 4100),             # the same at B = 2: image index > 0 (above the one-slab limit of 4096 units), last chunk of 5 pixels < PL
    (1, 128, 0, 16384),            # VAE-like, 64 chunks of 256 pixels
    (1, 512, 0, 4096),             # VAE mid block
    (1, 1280, 640, 1024),          # cpg 60: group 21 straddles the two sources
    (1, 64, 0, 5),                 # HW below PL
]
# (2, 128, 0, 2470) has 2470 four-channel units per (image, group) slab and B * G = 64 blocks: gn_select gives it to the one-slab
# kernel (<= 16 units per thread), ragged there too (2470 = 9 * 256 + 166).  It is tested on the path it takes.
ONE_SLAB_CASES = [(3, 1280, 1280, 16), (2, 128, 0, 2470)]
GROUP_QUAD_CASES = [(8, 264, 248, 16), (8, 1280, 640, 256)]
FOLD_CASES = [(1, 320, 4096), (2, 128, 1000)]                                   # (B, C, HW), dfh_groupnorm_fold with pre = None
PRODUCER_CASES = [(C, HW, tile) for C in (320, 640) for HW in (256, 1024) for tile in (6, 10, 21)]   # linear C -> C, B = 2
PRODUCER_B = 2
BACKWARD_CASES = [(1, 320, 0, 4096), (1, 320, 0, 1000), (1, 1280, 640, 1024)]


def case_id(c):
    return "x".join(str(v) for v in c)


# ----------------------------------------------------------------------------- launch geometry and summation depth
def two_kernel_geometry(B, C, HW, stats_target=512):
    """(PL, chunks, pix_per_chunk) as norm.h gn_two_kernel_geometry computes them (DFH_GN_SC at its default; norm.h points back here:
    the two change together)."""
    C8 = C // 8
    PL = max(1, min(256 // C8, HW))
    max_by_pix = -(-HW // PL)
    chunks = max(1, min(-(-stats_target // B), max_by_pix, 64))
    ppc = -(-HW // chunks)
    return PL, -(-HW // ppc), ppc


def two_kernel_depth(B, C, HW):
    """gn_stats_kernel: a thread adds the ceil(ppc / PL) pixels of its lane in ascending order (one channel per accumulator), thread g adds
    the PL lanes x cpg channels of its group one after the other, and gn_chunk_sums adds the chunks (one thread: `chunks` additions in a
    row; eight runs: fewer).  D = ceil(ppc / PL) + PL * cpg + chunks."""
    PL, chunks, ppc = two_kernel_geometry(B, C, HW)
    return -(-ppc // PL) + PL * (C // G) + chunks


def producer_depth(C, HW, rows):
    """256-row epilogues (gemm_wide_epilogue.h): a thread adds 16 rows of each of the four 64-row passes of its column (64 additions),
    the four row quarters are added in order, then the cpg columns of the group.  128-row epilogue (gemm.hip, the eight-wave tile): a
    thread adds the 64 rows of its half of the column, the two halves, then the cpg columns.  gn_chunk_sums then adds the HW / rows
    chunks.  One figure that covers both: D = 64 + 4 + cpg + HW / rows."""
    return 64 + 4 + C // G + HW // rows


def one_slab_depth(C, HW):
    """gn_small_kernel<UNITS>: a thread adds the four centred squares of each of its UNITS four-channel units one after the other
    (4 * UNITS in a row; the sum behind the mean adds one pairwise term per unit, a shorter chain), the wave sum is 6 butterfly steps,
    then (r0 + r1) + (r2 + r3).  D = 4 * UNITS + 8."""
    slab = HW * (C // G // 4)
    units = 8 if slab <= 256 * 8 else 16 if slab <= 256 * 16 else 32
    return 4 * units + 8


def group_quad_geometry(B, C, HW):
    """(gq, threads, ppb, UNITS) as norm.hip gn_select computes them for the group-quad kernel (the caller knows the shape takes it)."""
    upp = C // G // 4
    for gq in (4, 2):
        if G % gq or B * (G // gq) < 128 or gq * upp > 256:
            continue
        uppb = gq * upp

        def units_at(t):
            return 1 << 30 if t // uppb < 1 else -(-HW // (t // uppb))
        threads = 256
        while threads < 1024 and units_at(threads) > 24:
            threads *= 2
        if threads == 1024 and units_at(1024) > 16:
            threads = 512
        ppb = threads // uppb
        if ppb < 1:
            continue
        units = -(-HW // ppb)
        if units > 24:
            continue
        return gq, threads, ppb, 4 if units <= 4 else 8 if units <= 8 else 16 if units <= 16 else 24
    raise ValueError("not a group-quad shape")


def group_quad_depth(B, C, HW):
    """gn_mid_kernel<UNITS>: a thread adds one term per unit, (d0^2 + d1^2) + (d2^2 + d3^2), itself two additions deep (UNITS + 2), one
    thread per unit column adds the ppb pixel lanes in order, then the cpg / 4 unit columns of the group.  D = UNITS + 2 + ppb + cpg / 4."""
    _, _, ppb, units = group_quad_geometry(B, C, HW)
    return units + 2 + ppb + C // G // 4


# ----------------------------------------------------------------------------- inputs (seeded, CPU, bf16 [B][HW][C])
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _grouped(x):
    B, HW, C = x.shape
    return x.reshape(B, HW, G, C // G)


@functools.lru_cache(maxsize=4)
def exact_input(B, C, HW, seed=7):
    """Integers in [-3, 3]: exact in bf16, and with n * 9 < 2^24 every sum and sum of squares is exact in fp32 IN ANY ORDER, so a path
    that disagrees with fp64 summed the wrong set of elements."""
    return torch.randint(-3, 4, (B, HW, C), generator=_gen(seed)).to(torch.bfloat16)


def _unit_groups(B, C, HW, seed):
    """randn, each (image, group) shifted and scaled to mean 0 and std 1 exactly (fp64): what makes R_g = R hold at n = 10 as at n = 65536"""
    z = _grouped(torch.randn(B, HW, C, generator=_gen(seed), dtype=torch.float64))
    z = z - z.mean(dim=(1, 3), keepdim=True)
    return z / z.pow(2).mean(dim=(1, 3), keepdim=True).sqrt()


def group_signs():
    return torch.tensor([1.0 if g % 2 == 0 else -1.0 for g in range(G)], dtype=torch.float64)


@functools.lru_cache(maxsize=4)
def offset_input(B, C, HW, R, seed=11):
    """randn + R * sign_g (the sign alternates by group), rounded to bf16: |group mean| / group std = R up to that rounding."""
    z = _unit_groups(B, C, HW, seed) + R * group_signs().view(1, 1, G, 1)
    return z.reshape(B, HW, C).to(torch.bfloat16)


@functools.lru_cache(maxsize=4)
def constant_input(B, C, HW, seed=13):
    """offset_input at R = 8 with groups 0 and 17 of the LAST image set to 3.140625 everywhere (variance exactly 0: the one-pass
    difference lands on either side of zero and the clamp decides)."""
    x = _grouped(offset_input(B, C, HW, 8, seed).clone())
    for g in CONST_GROUPS:
        x[B - 1, :, g, :] = CONST_VALUE
    return x.reshape(B, HW, C)


def affine(C, seed=17):
    """gamma in [0.75, 1.25] (never near zero: the fold test divides by it), beta ~ 0.5 randn and at least 0.25 in size on every channel
    (so "the output is beta" on a constant group is a relative statement)."""
    g = _gen(seed)
    gamma = 1.0 + 0.5 * (torch.rand(C, generator=g) - 0.5)
    beta = 0.5 * torch.randn(C, generator=g)
    beta = torch.where(beta.abs() < 0.25, torch.where(beta < 0, -0.25, 0.25), beta)
    return gamma.float(), beta.float()


@functools.lru_cache(maxsize=4)
def producer_operands(C, HW, R, seed=19):
    """A linear GEMM C -> C whose bf16 OUTPUT is the test data, summed by its epilogue: A = the data without the offset, W = the
    identity (exact on the MFMA: one product per output), bias = R * sign_g, so the epilogue adds the offset and rounds once.
    R = 0: the exact-sum integers, no bias.  -> (A bf16 [B * HW][C], W bf16 [C][C], bias fp32 [C], the output bf16 [B][HW][C])."""
    B = PRODUCER_B
    w = torch.eye(C).to(torch.bfloat16)
    if R == 0:
        a = exact_input(B, C, HW, seed)
        bias = torch.zeros(C)
        return a.reshape(B * HW, C), w, bias, a
    a = _unit_groups(B, C, HW, seed).reshape(B, HW, C).to(torch.bfloat16)
    bias = (R * group_signs()).float().repeat_interleave(C // G)
    out = (a.float() + bias).to(torch.bfloat16)                 # fp32 accumulator + fp32 bias, one rounding to bf16
    return a.reshape(B * HW, C), w, bias, out


# ----------------------------------------------------------------------------- fp64 references
def stats64(x):
    """x bf16 / float [B][HW][C] -> (mean [B][G], biased variance [B][G], max|x| [B][G]) in fp64"""
    xg = _grouped(x.double())
    mean = xg.mean(dim=(1, 3))
    var = (xg - mean[:, None, :, None]).pow(2).mean(dim=(1, 3))
    return mean, var, xg.abs().amax(dim=(1, 3))


def groupnorm64(x, gamma, beta, eps, silu, affine_on=True):
    """fp64 GroupNorm(+SiLU) of x [B][HW][C] on the operands as given (eps: the fp32 value the kernel receives)"""
    mean, var, _ = stats64(x)
    xg = _grouped(x.double())
    y = ((xg - mean[:, None, :, None]) / (var[:, None, :, None] + f32(eps)).sqrt()).reshape(x.shape)
    if affine_on:
        y = y * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if silu else y


def rel(a, b) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


def yardstick(ref64) -> float:
    """relative L2 between the fp64 result rounded once to bf16 and itself: what a perfect kernel's output is off by"""
    return rel(ref64.to(torch.bfloat16), ref64)


def output_figures(got, ref64):
    """-> (rel L2, yardstick, max |err| / max|ref|, all finite)"""
    got = got.double().cpu()
    return rel(got, ref64), yardstick(ref64), float((got - ref64).abs().max() / ref64.abs().max()), bool(torch.isfinite(got).all())


def output_ok(figs) -> bool:
    e, y, m, finite = figs
    return finite and e <= FACTOR * y and m <= MAX_REL


def constant_mask(B):
    """[B][G] bool: the groups constant_input made constant"""
    m = torch.zeros(B, G, dtype=torch.bool)
    m[B - 1, list(CONST_GROUPS)] = True
    return m


# ----------------------------------------------------------------------------- the statistics legs
def exact_leg(stats, x, eps, one_pass, depth):
    """Leg A on exact-sum data.  stats [B][G][2] = (mean, rstd) fp32.  -> dict(mean_err / bound, rstd_err / bound), worst group; <= 1 passes.
    mean: one division of an exact sum, |mean - mean64| <= 2u |mean64| + 2^-149.  rstd, one pass: q / n, mean^2, the subtraction and
    the + eps are four roundings at condition ~1 (|mean| < 1 << std ~ 2 here), rsqrtf is good to 1 ulp = 2u: 8u carries a factor 2
    of margin.  Two passes: the variance bound with kappa = 1."""
    mean64, var64, _ = stats64(x)
    st = stats.double().cpu().view(*mean64.shape, 2)
    mean_ratio = float(((st[..., 0] - mean64).abs() / (2 * U * mean64.abs() + TINY)).max())
    if one_pass:
        rstd64 = (var64 + f32(eps)).rsqrt()
        rstd_ratio = float(((st[..., 1] - rstd64).abs() / rstd64).max() / (8 * U))
    else:
        var = st[..., 1].pow(-2) - f32(eps)
        rstd_ratio = float(((var - var64).abs() / var64).max() / (2 * (depth + 4) * U))
    return dict(mean=mean_ratio, rstd=rstd_ratio)


def conditioning_leg(stats, x, eps, one_pass, depth, skip=None):
    """Leg B.  -> dict(var = worst err / bound, mean = worst err / bound, K = worst measured err / (u kappa_g), R = (min, max) R_g,
    rstd_err = worst relative rstd error).  skip: [B][G] bool, groups left out (constant ones: no relative error there)."""
    mean64, var64, amax = stats64(x)
    st = stats.double().cpu().view(*mean64.shape, 2)
    keep = torch.ones_like(mean64, dtype=torch.bool) if skip is None else ~skip
    Rg = mean64.abs() / var64.sqrt()
    kappa = (1 + Rg * Rg) if one_pass else torch.ones_like(Rg)
    var = st[..., 1].pow(-2) - f32(eps)
    err = ((var - var64).abs() / var64)[keep]
    kap = kappa[keep]
    merr = ((st[..., 0] - mean64).abs() / ((depth + 2) * U * amax))[keep]
    rstd64 = (var64 + f32(eps)).rsqrt()
    return dict(var=float((err / (2 * (depth + 4) * U * kap)).max()), mean=float(merr.max()), K=float((err / (U * kap)).max()),
                R=(float(Rg[keep].min()), float(Rg[keep].max())), rstd_err=float(((st[..., 1] - rstd64).abs() / rstd64)[keep].max()))


def torch_fp32_stats(x, eps):
    """torch's own fp32 statistics [B][G][2] = (mean, rstd) (torch.native_group_norm), for the CPU test of the bounds"""
    B, HW, C = x.shape
    xn = x.float().permute(0, 2, 1).reshape(B, C, HW, 1).contiguous()
    _, mean, rstd = torch.native_group_norm(xn, None, None, B, C, HW, G, eps)
    return torch.stack([mean, rstd], dim=-1)


def torch_fp32_groupnorm(x, gamma, beta, eps, silu):
    y = torch.nn.functional.group_norm(x.float().permute(0, 2, 1), G, gamma, beta, eps).permute(0, 2, 1)
    return (torch.nn.functional.silu(y) if silu else y).to(torch.bfloat16)
