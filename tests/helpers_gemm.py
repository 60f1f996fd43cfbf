"""Inputs, fp64 references and case tables of the exact GEMM / conv / weight-gradient tests (tests/test_gpu_gemm_exact.py on the GPU,
tests/test_gemm_inputs_cpu.py for the conditions that keep those honest).  Everything here runs on the CPU and needs no library.

Why integers: with small-integer operands every product and every fp32 partial sum is an integer below 2^24, so the fp32 accumulator
equals the fp64 result whatever the order of the additions, split-K and slab reduces included.  The epilogue (gemm.h:
v = acc + bias + rowvec; v = act(v); v += resid) stays exact too with an integer fp32 bias / row vector and an integer bf16 residual, and the
only rounding left is the one round-to-nearest-even store: the kernel must equal rounded_once(ref64) bit for bit.  The bias spans
[-400, 400] and the residual the even numbers of [-512, 512], so that a good share of the outputs lies in (256, 1024) where bf16 keeps
every second / fourth integer: odd sums there are exact ties (test_gemm_inputs_cpu.py counts them).

Every case of the tables NAMES the instantiation it is meant to run (INST) together with the K split and the tile order it expects;
test_gemm_inputs_cpu.py holds dfh_gemm_plan to that on the CPU, the GPU tests hold the census to the plan."""
import math

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
CANARY16 = 0x7FA5                  # a bf16 NaN with a payload no kernel produces
CANARY32 = 0x7FA5A5A5              # the same as fp32
GUARD_BYTES = 4096
FACTOR_ULPS = 2                    # leg C: bf16 ulps of the reference an activation may be off where its fp32 model is not worse


# ----------------------------------------------------------------------------- inputs
def int_operand(shape, lo, hi, seed, dtype=BF16, scale=1.0):
    """seeded CPU integers of [lo, hi] (times a power of two `scale`) in `dtype`: exact in bf16 for |value / scale| <= 256"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(lo, hi + 1, tuple(shape), generator=g).double() * scale).to(dtype)


def even_operand(shape, half, seed):
    """even integers of [-2 half, 2 half] as bf16 (exact up to 512): the residual"""
    return (int_operand(shape, -half, half, seed, torch.float64) * 2).to(BF16)


def rounded_once(ref64, dtype=BF16):
    """the fp64 result rounded once, to nearest even, to the storage type"""
    return ref64.to(dtype)


def bf16_ulp(ref64):
    """the bf16 ulp at every element of an fp64 tensor (normal range)"""
    _, e = torch.frexp(ref64.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref64), e - 8)


def tie_share(ref64):
    """share of elements that lie exactly half way between two bf16 numbers"""
    r = ref64.to(BF16).double()
    return float(((ref64 - r).abs() == bf16_ulp(ref64) / 2).double().mean())


class Poisoned:
    """A tensor inside a larger allocation filled with a NaN canary: `rows_after` rows and `cols_after` columns beyond the 2-D tensor and
    `guard` bytes on either side.  .view is the tensor (row stride .ld), .intact() whether every element outside it still holds the canary,
    compared as integers.  fill: another value for the surroundings (finite poison)."""

    def __init__(self, t, rows_after=8, cols_after=8, guard=GUARD_BYTES, device=None, fill=None, blank=False):
        assert t.dim() == 2
        R, Cn = t.shape
        self.itype = {2: torch.int16, 4: torch.int32}[t.element_size()]
        ge = guard // t.element_size()
        self.ld, self.R, self.C, self.ge = Cn + cols_after, R, Cn, ge
        n = (R + rows_after) * self.ld
        self.alloc = torch.empty(n + 2 * ge, dtype=t.dtype, device=device or t.device)
        if fill is None:
            self.alloc.view(self.itype).fill_(CANARY16 if t.element_size() == 2 else CANARY32)
        else:
            self.alloc.fill_(fill)
        self.pristine = self.alloc.clone()
        self.view = self._view_of(self.alloc)
        if not blank:
            self.view.copy_(t)

    def _view_of(self, alloc):
        return alloc[self.ge:self.ge + (self.alloc.numel() - 2 * self.ge)].view(-1, self.ld)[:self.R, :self.C]

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        chk = self.alloc.clone()
        self._view_of(chk).copy_(self._view_of(self.pristine))
        return bool(torch.equal(chk.view(self.itype), self.pristine.view(self.itype)))


def poisoned(t, rows_after=8, cols_after=8, guard=GUARD_BYTES, device=None, fill=None, blank=False):
    """-> Poisoned: .view (the tensor, inside) and .alloc (the allocation around it).  blank: an output -- only the shape and type of `t`
    are used, the view starts as canaries too, so an element the kernel never writes shows as well"""
    return Poisoned(t, rows_after, cols_after, guard, device, fill, blank)


# ----------------------------------------------------------------------------- fp64 references
def pack_conv64(w_oihw):
    """OIHW -> the packed [O][9 I] matrix, column = tap * I + c (dfh_pack_conv3x3)"""
    O, I = w_oihw.shape[:2]
    return w_oihw.permute(0, 2, 3, 1).reshape(O, 9 * I)


def unpack_conv64(w_packed, I):
    return w_packed.reshape(w_packed.shape[0], 3, 3, I).permute(0, 3, 1, 2)


def conv64(x_nhwc, w_packed, stride=1, ups=0):
    """3x3 / pad 1 conv of an NHWC tensor with a packed [N][9 C] matrix, fp64 -> [B Ho Wo][N].  ups 1: nearest-2x upsample first; ups 2:
    the input with zeros inserted between its pixels (the data gradient of a stride-2 conv)"""
    x = x_nhwc.double().permute(0, 3, 1, 2)
    if ups == 1:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    elif ups == 2:
        z = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], dtype=torch.float64)
        z[:, :, ::2, ::2] = x
        x = z
    y = F.conv2d(x, unpack_conv64(w_packed.double(), x.shape[1]), stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w_packed.shape[0])


def gelu64(x):
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))      # (1 + erf cancels to 0 in fp64 below x = -8.3; erfc keeps the tail)


ACT64 = {0: lambda x: x, 1: lambda x: x * torch.sigmoid(x), 2: lambda x: torch.where(x > 0, x, 0.01 * x), 3: torch.tanh,
         5: gelu64, 6: lambda x: x * torch.sigmoid(1.702 * x)}


def geglu_split(h):
    """packed GEGLU columns (16-column blocks of values and gates alternate: dfh_pack_matrix's interleave) -> (values, gates)"""
    v, g = h.view(h.shape[0], h.shape[1] // 32, 2, 16).unbind(2)
    return v.reshape(h.shape[0], -1), g.reshape(h.shape[0], -1)


def pre64(acc, bias=None, rowvec=None, rv_off=0, rows_per_b=0):
    """acc + bias[n] + rowvec[m / rows_per_b][rv_off + n] in fp64"""
    M, N = acc.shape
    v = acc.clone()
    if bias is not None:
        v += bias.double()
    if rowvec is not None:
        v += rowvec.double()[:, rv_off:rv_off + N].repeat_interleave(rows_per_b, 0)[:M]
    return v


def ref64(acc, bias=None, rowvec=None, rv_off=0, rows_per_b=0, act=0, resid=None):
    """the documented epilogue (gemm.h) in fp64: v = acc + bias + rowvec; v = act(v); v += resid"""
    v = pre64(acc, bias, rowvec, rv_off, rows_per_b)
    if act == 4:
        val, gate = geglu_split(v)
        v = val * gelu64(gate)
    else:
        v = ACT64[act](v)
    if resid is not None:
        v = v + resid.double()
    return v


# ----------------------------------------------------------------------------- the activations as the kernels evaluate them (dfh_common.h)
def _f32(x):
    return x.to(torch.float32).double()


def _fma32(a, b, c):
    return _f32(a * b + c)              # a, b fp32 values held in fp64: the product is exact there, one rounding of the sum


def act_model32(x64, act):
    """The kernel's own fp32 formula for `act` (dfh_common.h silu_f / gelu_erf_f, gemm.hip), every operation rounded to fp32 and the
    hardware reciprocal / exp2 taken as correctly rounded, evaluated on fp32-exact inputs -> fp64 tensor of fp32 values.  This is the
    documented approximation alone: what it is off by against ACT64 is not the epilogue's fault."""
    x = _f32(x64)
    if act == 1 or act == 6:
        k = -1.44269504088896340736 if act == 1 else float(torch.tensor(-1.702, dtype=torch.float32)) * 1.44269504088896340736   # (folded at compile time)
        e = _f32(torch.exp2(_f32(x * _f32(torch.tensor(k)))))
        return _f32(x * _f32(1.0 / _f32(1.0 + e)))
    if act == 2:
        return torch.where(x > 0, x, _f32(x * _f32(torch.tensor(0.01))))
    if act == 3:
        return _f32(torch.tanh(x))
    if act in (4, 5):
        ax = x.abs().clamp_max(float(torch.tensor(5.65685424949, dtype=torch.float32)))
        co = [1.917432119e-05, -6.586021110e-04, 7.754402186e-03, -5.296538429e-02, -4.590602584e-01, -1.151122051e+00]
        co = [float(torch.tensor(c, dtype=torch.float32)) for c in co]
        last = float(torch.tensor(3.063254510e-07, dtype=torch.float32) - 1.0)
        p = torch.full_like(x, co[0])
        for c in co[1:] + [last]:
            p = _fma32(p, ax, torch.full_like(x, c))
        h = _f32(x * _f32(torch.exp2(p)))
        return _f32(x.clamp_min(0.0) - h.abs())
    return x


def ulps(got, ref64_):
    """|got - ref| in bf16 ulps of the reference, elementwise (fp64)"""
    return (got.double() - ref64_).abs() / bf16_ulp(ref64_)


def yardstick(ref64_):
    """relative L2 of the reference rounded once to bf16 against itself: what storing the exact result costs"""
    return float((ref64_.to(BF16).double() - ref64_).norm() / ref64_.norm())


def rel_l2(got, ref64_):
    return float((got.double() - ref64_).norm() / ref64_.norm())


# ----------------------------------------------------------------------------- instantiations
# name -> (force_tile that pins it, kernel, tile, bm, bn, stages, lean, wide) as dfh_gemm_plan reports them.  kernel: 0 gemm_bf16_kernel
# tile, 1 its 256 x 320 tile, 2 its 256 x 256 GEGLU tile, 3 gemm_wide_kernel.  For kernel 3 `tile` is the heuristic tile the plan's checks
# were made against (gemm_plan.h), not a different kernel: both values of the golden table are kept so that both sets of checks run.
INST = {
    "ring256x160": (1, 0, 0, 256, 160, 3, 0, 0),
    "ring256x128": (2, 0, 1, 256, 128, 3, 0, 0),
    "t128x64": (3, 0, 2, 128, 64, 3, 0, 0),
    "t128x160": (4, 0, 3, 128, 160, 2, 0, 0),
    "t128x128": (5, 0, 4, 128, 128, 2, 0, 0),
    "e8_s4_lean": (10, 0, 5, 128, 160, 4, 1, 0),
    "e8_s4": (10, 0, 5, 128, 160, 4, 0, 0),
    "e8_s2_lean": (10, 0, 5, 128, 160, 2, 1, 0),
    "e8_s2": (10, 0, 5, 128, 160, 2, 0, 0),
    "big_lean": (21, 1, 5, 256, 320, 2, 1, 0),
    "big": (21, 1, 5, 256, 320, 2, 0, 0),
    "bigg_lean": (23, 2, 4, 256, 256, 2, 1, 0),
    "wide160_t5": (6, 3, 5, 256, 160, 3, 0, 1),
    "wide160_t4": (6, 3, 4, 256, 160, 3, 0, 1),
    "wide128_t4": (9, 3, 4, 256, 128, 3, 0, 4),
    "wide128_t5": (9, 3, 5, 256, 128, 3, 0, 4),
}
# Instantiations of the golden table that no test can launch, by name.  The list may not grow beyond two entries
# (test_gemm_inputs_cpu.py asserts it): anything else must be reached by a case, pinned at a small shape if need be.
UNREACHABLE = {
    # force ids 7 / 30 plan gemm_wide_launch variants 2 / 25; the product library holds neither (gemm_wide.hip: "variants 2 / 3 / 8-13 are
    # probe instantiations", unknown ids end in the same refusal), so the launch is refused whatever the shape
    "wide variants the product library does not contain": lambda k: k[0] == "wide" and k[5] in (2, 25),
    # the training GEGLU launch with pre_out (variant 5): only the training walk sets GemmArgs::pre_out, dfh_gemm_plan_extra plans it but no
    # entry point of the C ABI launches it
    "wide variant 5 (GEGLU with pre_out): no C ABI entry point": lambda k: k[0] == "wide" and k[5] == 5,
}
KERNEL_NAMES = ("tile", "big", "big_geglu", "wide")


def inst_key(name):
    _, kernel, tile, bm, bn, stages, lean, wide = INST[name]
    return (KERNEL_NAMES[kernel], tile, f"{bm}x{bn}", stages, lean, wide)


# ----------------------------------------------------------------------------- forward cases (leg A)
def lin(inst, M, N, K0, K1=0, **kw):
    return dict(dict(kind="lin", inst=inst, M=M, N=N, K0=K0, K1=K1), **kw)


def conv(inst, B, H, W, C, N, stride=1, ups=0, K0=0, K1=0, **kw):
    Ho, Wo = (2 * H, 2 * W) if ups else ((H + stride - 1) // stride if stride == 1 else H // 2, W if stride == 1 else W // 2)
    return dict(dict(kind="conv", inst=inst, B=B, H=H, W=W, C=C, N=N, stride=stride, ups=ups, K0=K0, K1=K1, M=B * Ho * Wo,
                     rows_per_b=Ho * Wo), **kw)


def _per_inst(inst, bm, bn, ks, n_small=4, lean=False, **kw):
    """M in {bm - 1, bm + 1, 3, a multiple} against N in {n_small, bn - n_small, bn + 8, a multiple} and the K segments `ks`, paired
    diagonally (each value of each list occurs; the cross product would be 64 launches per instantiation)"""
    Ms, Ns = (bm - 1, bm + 1, 3, 2 * bm), (n_small, bn - n_small, bn + 8, bn)
    return [lin(inst, M, N, K, **kw) for M, N, K in zip(Ms, Ns, ks)]


GENERAL_K = (8, 72, 200, 128)       # virtual padding to 64 through the zero page; the last one whole slices
LEAN_K = (64, 128, 192, 2048)       # the LEAN k-loop: whole 64-channel slices only


def forward_cases():
    t = []
    # --- gemm_bf16_kernel tiles 1..5 (never LEAN): N % 4 is all they need
    for inst, bm, bn in (("ring256x160", 256, 160), ("ring256x128", 256, 128), ("t128x64", 128, 64), ("t128x160", 128, 160), ("t128x128", 128, 128)):
        t += _per_inst(inst, bm, bn, GENERAL_K)
    t.append(lin("t128x128", 300, 136, 2048, split=4))                      # the heuristic's own split of a deep, small launch
    # --- the eight-wave 128 x 160 tile: four-stage ring up to 320 workgroups, LEAN on whole slices
    t += _per_inst("e8_s4", 128, 160, GENERAL_K[:3] + (264,))
    t += _per_inst("e8_s4_lean", 128, 160, LEAN_K[:3] + (1024,), fsplit=1)
    t.append(lin("e8_s4_lean", 130, 320, 2048, split=4))                     # heuristic split-K on the LEAN loop
    t.append(lin("e8_s2", 2305, 2568, 72))                                    # 19 x 17 = 323 workgroups: the two-stage ring
    t.append(lin("e8_s2_lean", 2305, 2568, 64))
    t.append(lin("e8_s2_lean", 2305, 2568, 128, K1=64))                       # ... and the LEAN loop re-basing its A pointers
    # --- 256 x 320 eight-wave tile and gemm_wide_kernel: N % 8 (16-byte output rows); what N % 8 != 0 does to the pin is in FALLBACK_CASES
    # (N <= 64 would make the heuristic tile, which these plans carry along, the 128 x 64 one: the golden table has no such line)
    for M, N, K, KL in ((255, 168, 8, 64), (257, 312, 72, 128), (3, 328, 200, 192), (512, 320, 72, 1024)):
        t += [lin("big", M, N, K), lin("big_lean", M, N, KL, fsplit=1)]
    t += [lin("wide160_t5", 255, 160, 8), lin("wide160_t5", 257, 152 + 160, 72), lin("wide160_t5", 3, 168, 200), lin("wide160_t5", 512, 320, 64)]
    t += [lin("wide160_t4", 255, 72, 8), lin("wide160_t4", 257, 128, 72), lin("wide160_t4", 3, 104, 200), lin("wide160_t4", 512, 256, 128)]
    t += [lin("wide128_t4", 255, 72, 8), lin("wide128_t4", 257, 120, 72), lin("wide128_t4", 3, 128, 200), lin("wide128_t4", 512, 256, 128)]
    t += [lin("wide128_t5", 255, 160, 8), lin("wide128_t5", 257, 136, 72), lin("wide128_t5", 3, 168, 200), lin("wide128_t5", 512, 320, 128)]
    # --- two plain segments (channel concat), the split-K boundary inside segment 1
    t.append(lin("e8_s4", 256, 160, 192, K1=96))                               # ragged lengths: the general k-step iterator
    t.append(lin("e8_s4_lean", 300, 320, 256, K1=64, fsplit=1))
    t.append(lin("big_lean", 300, 320, 256, K1=64, fsplit=1))
    t.append(lin("e8_s4_lean", 200, 160, 128, K1=320, fsplit=3))              # slices 2 and 3 START inside segment 1
    t.append(lin("ring256x160", 200, 164, 72, K1=200, fsplit=2))
    t.append(lin("wide160_t5", 300, 320, 200, K1=72))
    # --- split-K 2 and 5 (test_gemm_splitk_matches_single_pass's shape class, smaller), bf16 and fp32; the single pass is the same table's
    for fs in (1, 2, 5):
        for om in (0, 2):
            t.append(lin("e8_s4_lean", 200, 320, 640, fsplit=fs, out_mode=om))
            t.append(lin("t128x128", 200, 132, 328, fsplit=fs, out_mode=om))
    # --- tile order pinned n-major on three kernels (placement never changes results)
    t.append(lin("ring256x160", 300, 328, 72, order=2))
    t.append(lin("wide160_t5", 300, 320, 72, order=2))
    t.append(lin("big", 300, 648, 72, order=2))
    # --- 3x3 convs: non-square images, conv_c in {8, 64, 72}, stride 2, upsample, fused 1x1 shortcut segments
    # (fsplit=1: at 16 k-steps and more the heuristic splits these small launches, and a split launch takes no wide / 256 x 320 pin;
    #  nm=1: a conv whose weights outweigh its pixels walks its tiles n-major when N > 160)
    for inst in ("e8_s4", "ring256x160", "wide160_t5", "big"):
        t.append(conv(inst, 3, 2, 2, 64, 160, fsplit=1))                      # every tap hits padding somewhere
        t.append(conv(inst, 2, 5, 3, 72, 168 if inst != "ring256x160" else 164, fsplit=1, nm=1))
        t.append(conv(inst, 2, 12, 20, 64, 320, fsplit=1, nm=1))              # the lean tap staging, 480 rows
        t.append(conv(inst, 3, 16, 1, 8, 160))
    t.append(conv("wide128_t4", 2, 12, 20, 64, 128, fsplit=1))
    t.append(conv("t128x64", 2, 5, 3, 72, 4, out_mode=3, fsplit=1))           # conv_out: fp32, transposed per image
    for inst in ("e8_s4", "wide160_t5", "big", "t128x160"):
        t.append(conv(inst, 2, 12, 20, 64, 160, stride=2, fsplit=1))
        t.append(conv(inst, 2, 5, 3, 72, 160, ups=1, fsplit=1))
        t.append(conv(inst, 2, 6, 10, 64, 320, K0=64, K1=72, fsplit=1, nm=1)) # conv2 + the 1x1 shortcut over (x0, x1)
    t.append(conv("e8_s4", 1, 16, 16, 64, 320, fsplit=2, nm=1))               # weights outweigh pixels: n-major by the heuristic; slices of the tap-major walk
    # --- transposed outputs (attention's V^T with 77 keys padded; conv_out's NCHW is above) and per-image weights
    t.append(lin("e8_s4", 3 * 77, 64 + 96, 72, out_mode=1, rows_per_b=77))
    t.append(lin("e8_s4_lean", 2 * 256, 160, 128, out_mode=1, rows_per_b=256, fsplit=1))      # tiles inside one batch element: staged transposed
    t.append(lin("t128x160", 2 * 136, 96, 64, out_mode=1, rows_per_b=136))
    t.append(lin("t128x64", 3 * 77, 64, 128, out_mode=3, rows_per_b=77))
    t.append(lin("e8_s4_lean", 3 * 128, 168, 64, rows_per_b=128, w_img=1, fsplit=1))
    t.append(lin("t128x128", 2 * 256, 132, 72, rows_per_b=256, w_img=1))
    return t


# a pinned kernel that cannot take the launch falls back to the heuristic tile (gemm_plan.hip); these name where N % 8 != 0 sends the pins
FALLBACK_CASES = [
    dict(lin("e8_s4", 255, 156, 72), force_tile=6), dict(lin("t128x128", 257, 124, 72), force_tile=9), dict(lin("e8_s4", 255, 316, 72), force_tile=21),
    dict(lin("t128x64", 3, 4, 200), force_tile=6), dict(lin("t128x64", 3, 4, 200), force_tile=21),
]

# GEGLU (packed value / gate blocks), bias only: leg C compares against fp64, here only the plan is named.  (M, C): N = 8 C
GEGLU_CASES = [lin("bigg_lean", 255, 256, 64, act=4), lin("bigg_lean", 257, 640, 128, act=4), lin("bigg_lean", 3, 128, 192, act=4), lin("bigg_lean", 512, 256, 64, act=4),
               lin("t128x128", 300, 320, 40, act=4, force_tile=0), lin("wide128_t4", 300, 256, 72, act=4), lin("wide160_t4", 520, 320, 200, act=4)]


def case_id(c):
    s = f"{c['inst']}-" + (f"conv{c['B']}x{c['H']}x{c['W']}x{c['C']}s{c['stride']}u{c['ups']}" if c["kind"] == "conv" else "lin") + f"-M{c['M']}N{c['N']}K{c['K0']}+{c['K1']}"
    for k in ("fsplit", "split", "order", "out_mode", "w_img", "act", "force_tile"):
        if k in c:
            s += f"-{k}{c[k]}"
    return s


def want_plan(c):
    """(kernel, tile, bm, bn, stages, lean, wide, split, n_major) the case names"""
    _, kernel, tile, bm, bn, stages, lean, wide = INST[c["inst"]]
    return (kernel, tile, bm, bn, stages, lean, wide, c.get("split", max(c.get("fsplit", 1), 1)), c.get("nm", 1 if c.get("order") == 2 else 0))


def k_total(c):
    return (9 * c["C"] if c["kind"] == "conv" else 0) + c["K0"] + c["K1"]


def desc_scalars(c):
    """the scalar fields of dfh_gemm_desc for a case (pointers are the caller's)"""
    d = dict(M=c["M"], N=c["N"], a0_c=c["K0"], a1_c=c["K1"], act=c.get("act", 0), out_mode=c.get("out_mode", 0),
             force_tile=c.get("force_tile", INST[c["inst"]][0]), force_split=c.get("fsplit", 0), force_order=c.get("order", -1),
             rows_per_b=c.get("rows_per_b", 0))
    if c["kind"] == "conv":
        d.update(conv=1, conv_c=c["C"], batch=c["B"], Hin=c["H"], Win=c["W"], stride=c["stride"], upsample=c["ups"])
    return d


def out_cols(c):
    return c["N"] // 2 if c.get("act") == 4 else c["N"]


def fill_desc(d, c, ptr, pad=8):
    """fills a dfh_gemm_desc (any object with its fields) for a case.  ptr(name) -> the address of operand `name` ("W", "out", "zero",
    "conv_src", "a0", "a1", "bias", "rowvec", "resid"); W rows, output rows and (row-major) output columns are `pad` elements longer than
    they need be, as the GPU tests allocate them.  The CPU tests pass a made-up address: the plan tests pointers for presence only."""
    for k, v in desc_scalars(c).items():
        setattr(d, k, v)
    K, N = k_total(c), c["N"]
    d.W, d.ldw, d.out, d.zero_page = ptr("W"), K + pad, ptr("out"), ptr("zero")
    if c["kind"] == "conv":
        d.conv_src = ptr("conv_src")
    if c["K0"]:
        d.a0 = ptr("a0")
    if c["K1"]:
        d.a1 = ptr("a1")
    has_b, has_rv, has_res = epilogue_flags(c)
    if has_b:
        d.bias = ptr("bias")
    if has_rv:
        d.rowvec, d.rv_ld, d.rv_off = ptr("rowvec"), 2 * N, N
    if has_res:
        d.resid, d.ld_res = ptr("resid"), N
    nb, rpb = n_batches(c)
    d.ld_out = (rpb if c.get("out_mode", 0) in (1, 3) else out_cols(c)) + pad
    if c.get("w_img"):
        d.w_img_stride = (N + pad) * (K + pad)
    return d


def epilogue_flags(c):
    """(bias, rowvec, resid) of a case: everything the launch can carry"""
    plain = c.get("act", 0) != 4 and not c.get("w_img")
    return True, plain and c.get("out_mode", 0) in (0, 2), plain and c.get("out_mode", 0) in (0, 2) and c.get("resid", True)


def n_batches(c):
    rpb = c.get("rows_per_b", 0) or c["M"]
    return -(-c["M"] // rpb), rpb


def forward_inputs(c, seed=0, a_scale=1.0):
    """-> dict of CPU tensors: a0, a1 ([M][K]), x (NHWC), w ([N][K] or per image [nb][N][K]), bias, rowvec ([nb][2 N], read at offset N),
    resid, and acc (fp64 [M][N])"""
    M, N, K = c["M"], c["N"], k_total(c)
    nb, rpb = n_batches(c)
    s = 1000 * seed + 17
    out = dict(a0=None, a1=None, x=None, rowvec=None, resid=None)
    cols = []
    if c["kind"] == "conv":
        out["x"] = int_operand((c["B"], c["H"], c["W"], c["C"]), -3, 3, s + 1, scale=a_scale)
    if c["K0"]:
        out["a0"] = int_operand((M, c["K0"]), -3, 3, s + 2, scale=a_scale)
        cols.append(out["a0"].double())
    if c["K1"]:
        out["a1"] = int_operand((M, c["K1"]), -3, 3, s + 3, scale=a_scale)
        cols.append(out["a1"].double())
    wshape = (nb, N, K) if c.get("w_img") else (N, K)
    out["w"] = int_operand(wshape, -3, 3, s + 4)
    w = out["w"].double()
    acc = torch.zeros(M, N, dtype=torch.float64)
    kc = 9 * c["C"] if c["kind"] == "conv" else 0
    if kc:
        acc += conv64(out["x"], w[:, :kc], c["stride"], c["ups"])
    if cols:
        a = torch.cat(cols, 1)
        if c.get("w_img"):
            acc += torch.einsum("bmk,bnk->bmn", a.view(nb, rpb, -1), w[:, :, kc:]).reshape(M, N)
        else:
            acc += a @ w[:, kc:].T
    has_b, has_rv, has_res = epilogue_flags(c)
    out["bias"] = int_operand((N,), -400, 400, s + 5, torch.float32)
    if has_rv:
        out["rowvec"] = int_operand((nb, 2 * N), -64, 64, s + 6, torch.float32)
    if has_res:
        out["resid"] = even_operand((M, N), 256, s + 7)
    out["acc"] = acc
    return out


def forward_ref64(c, inp):
    _, rpb = n_batches(c)
    return ref64(inp["acc"], inp["bias"], inp["rowvec"], c["N"], rpb, c.get("act", 0), inp["resid"])


# ----------------------------------------------------------------------------- Winograd (leg B)
# (B, cin, cout, H, W, resid, temb).  The smallest of test_conv3x3_winograd's, a plane of at most 256 rows and one above (wino_gemm_tile's
# threshold), the non-square 6 x 10, cout in {40, 160, 320}
WINO_CASES = [(2, 64, 96, 2, 2, False, True), (1, 72, 40, 4, 4, True, True), (3, 128, 160, 6, 10, True, False), (4, 64, 320, 16, 16, True, True),
              (5, 64, 160, 16, 16, True, True)]
WINO_G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1.]], dtype=torch.float64)
WINO_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1.]], dtype=torch.float64)


def wino_inputs(case, seed=0):
    """x in [-1, 1]; every output channel reads two input channels with taps of {-8, -4, 0, 4, 8}: U = G g G^T is an integer of at most 18
    in size, V = B^T d B one of at most 4, M = sum over the two channels at most 2 * 18 * 4 = 144 < 256 -- every intermediate is exact as
    stored in bf16, and the output is the conv exactly.  The bias, the time-embedding row and the residual are large enough that outputs
    pass 256 and round."""
    B, cin, cout, H, W, resid, temb = case
    s = 5000 + 100 * seed
    x = int_operand((B, H, W, cin), -1, 1, s + 1)
    g = torch.Generator().manual_seed(s + 2)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    for o in range(cout):
        ch = torch.randperm(cin, generator=g)[:2]
        w[o, ch] = (torch.randint(-2, 3, (2, 3, 3), generator=g) * 4).double()
    bias = int_operand((cout,), -400, 400, s + 3, torch.float32)
    rv = int_operand((B, 3 * cout), -64, 64, s + 4, torch.float32) if temb else None
    res = even_operand((B * H * W, cout), 256, s + 5) if resid else None
    return dict(x=x, w=w, bias=bias, rowvec=rv, resid=res)


def wino_intermediates(inp):
    """fp64 U [16][N][C], V [16][tiles][C], M [16][tiles][N]"""
    x, w = inp["x"].double(), inp["w"]
    cout, cin = w.shape[:2]
    U = torch.einsum("ij,ncjk,lk->ilnc", WINO_G, w, WINO_G).reshape(16, cout, cin)
    patches = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)
    V = torch.einsum("ij,bcyxjk,lk->ilbyxc", WINO_BT, patches, WINO_BT).reshape(16, -1, cin)
    return U, V, torch.einsum("pmc,pnc->pmn", V, U)


def wino_ref64(case, inp):
    B, cin, cout, H, W, resid, temb = case
    acc = conv64(inp["x"], pack_conv64(inp["w"]))
    return ref64(acc, inp["bias"], inp["rowvec"], cout, H * W, 0, inp["resid"])


# ----------------------------------------------------------------------------- activations (leg C)
# (act, inst, M, N, K): operands scaled by 2^-4, row-vector offsets of -6 .. 6 per batch of rows: pre-activations on a 1/16 grid over about
# [-12, 12], exact 0 and both sides of the minimum of SiLU (x = -1.2785, where SiLU' changes sign) included
ACT_SCALE = 2.0 ** -4
ACT_CASES = [(1, "e8_s4_lean", 390, 160, 64), (1, "wide160_t5", 390, 168, 72), (1, "big", 390, 320, 72), (2, "e8_s4", 390, 164, 72),
             (3, "e8_s4_lean", 390, 160, 64), (3, "wide128_t4", 390, 128, 72), (5, "e8_s2_lean", 390, 168, 64), (6, "e8_s2_lean", 390, 160, 128)]
ACT_GEGLU = [("bigg_lean", 300, 512, 64), ("t128x128", 300, 320, 72), ("wide128_t4", 300, 256, 64), ("wide160_t4", 300, 320, 64)]


def act_case(act, inst, M, N, K):
    # GELU / quick-GELU always run on the eight-wave tile, two stages, single pass, whatever is pinned (gemm_plan.hip xact)
    return lin(inst, M, N, K, act=act, rows_per_b=30, resid=False, **({} if act in (5, 6) else dict(fsplit=1)))


def act_inputs(c, seed=3):
    """integer operands times 2^-4 -> accumulators on a 1/16 grid; bias of {-1 .. 1} / 16, row vector of -6 .. 6 per batch of 30 rows"""
    M, N = c["M"], c["N"]
    nb, rpb = n_batches(c)
    s = 9000 + seed
    a = int_operand((M, c["K0"]), -3, 3, s + 1, scale=ACT_SCALE)
    w = int_operand((N, c["K0"]), -3, 3, s + 2)
    bias = int_operand((N,), -1, 1, s + 3, torch.float32, scale=ACT_SCALE)
    rv = None
    if c.get("act") != 4:
        rv = (torch.arange(nb, dtype=torch.float64) % 13 - 6)[:, None].expand(nb, 2 * N).to(torch.float32).contiguous()
    acc = a.double() @ w.double().T
    return dict(a0=a, a1=None, x=None, w=w, bias=bias, rowvec=rv, resid=None, acc=acc)


# ----------------------------------------------------------------------------- weight gradients (leg E)
# dW[n][k] += sum_m dY[m][n] A[m][k] on integers: fp32 and exact.  Each case names dfh_gemm_wgrad_plan's (tiles, whole tiles, slices).
def wg(kind, M, N, msplit, plan, **kw):
    return dict(dict(kind=kind, M=M, N=N, msplit=msplit, plan=plan, K0=0, K1=0), **kw)


def wgrad_cases():
    t = []
    for (M, N, K), plans in (((8, 4, 200), None), ((130, 36, 72), None), ((300, 160, 64), None), ((300, 164, 328), None)):
        for ms in (0, 1, 3, 7, -4):
            t.append(wg("lin", M, N, ms, None, K0=K))
    t.append(wg("lin", 300, 36, 3, None, K0=192, K1=64, col_off=16))          # two sources inside a wider packed matrix
    for ms in (0, 3):
        t.append(wg("conv", 2 * 16 * 12, 160, ms, None, B=2, H=16, W=12, C=8, stride=1, ups=0))
        t.append(wg("conv", 2 * 8 * 6, 36, ms, None, B=2, H=16, W=12, C=72, stride=2, ups=0))
        t.append(wg("conv", 2 * 10 * 6, 164, ms, None, B=2, H=5, W=3, C=72, stride=1, ups=1))
        t.append(wg("conv", 3 * 2 * 2, 160, ms, None, B=3, H=2, W=2, C=64, stride=1, ups=0))       # every tap hits padding
    t.append(wg("conv", 2 * 6 * 10, 36, 7, None, B=2, H=6, W=10, C=64, stride=1, ups=0, K0=64, K1=8))   # conv2 + the shortcut segments
    return t


def wgrad_id(c):
    s = f"{c['kind']}-M{c['M']}N{c['N']}K{k_total(c)}-ms{c['msplit']}"
    return s + (f"-conv{c['B']}x{c['H']}x{c['W']}x{c['C']}s{c['stride']}u{c['ups']}" if c["kind"] == "conv" else "")


def wgrad_inputs(c, seed=0):
    """A as forward_inputs builds it, dY integers of [-3, 3], dW0 a non-zero integer start; -> dict with ref (fp64 [N][K])"""
    M, N, K = c["M"], c["N"], k_total(c)
    s = 7000 + seed
    out = dict(a0=None, a1=None, x=None)
    dy = int_operand((M, N), -3, 3, s + 1)
    blocks = []
    if c["kind"] == "conv":
        out["x"] = int_operand((c["B"], c["H"], c["W"], c["C"]), -3, 3, s + 2)
        # the im2col matrix through the same conv64: one-hot weights would be slow; unfold instead
        x = out["x"].double().permute(0, 3, 1, 2)
        if c["ups"] == 1:
            x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        cols = F.unfold(x, 3, padding=1, stride=c["stride"])                  # [B][C * 9][L], row = c * 9 + tap
        cols = cols.view(x.shape[0], c["C"], 9, -1).permute(0, 3, 2, 1).reshape(M, 9 * c["C"])      # column = tap * C + c
        blocks.append(cols)
    if c["K0"]:
        out["a0"] = int_operand((M, c["K0"]), -3, 3, s + 3)
        blocks.append(out["a0"].double())
    if c["K1"]:
        out["a1"] = int_operand((M, c["K1"]), -3, 3, s + 4)
        blocks.append(out["a1"].double())
    out["dy"] = dy
    out["dw0"] = int_operand((N, K), -50, 50, s + 5, torch.float32)
    out["ref"] = out["dw0"].double() + dy.double().T @ torch.cat(blocks, 1)
    return out


# dfh_gemm_wgrad_plan's (output tiles, tiles that run whole, pixel slices of the rest) per case, as each case names it
WGRAD_PLANS = {
    "lin-M8N4K200-ms0": (2, 0, 1),
    "lin-M8N4K200-ms1": (2, 0, 1),
    "lin-M8N4K200-ms3": (2, 0, 3),
    "lin-M8N4K200-ms7": (2, 0, 7),
    "lin-M8N4K200-ms-4": (2, 0, 4),
    "lin-M130N36K72-ms0": (1, 0, 1),
    "lin-M130N36K72-ms1": (1, 0, 1),
    "lin-M130N36K72-ms3": (1, 0, 3),
    "lin-M130N36K72-ms7": (1, 0, 7),
    "lin-M130N36K72-ms-4": (1, 0, 4),
    "lin-M300N160K64-ms0": (1, 0, 1),
    "lin-M300N160K64-ms1": (1, 0, 1),
    "lin-M300N160K64-ms3": (1, 0, 3),
    "lin-M300N160K64-ms7": (1, 0, 7),
    "lin-M300N160K64-ms-4": (1, 0, 4),
    "lin-M300N164K328-ms0": (6, 0, 1),
    "lin-M300N164K328-ms1": (6, 0, 1),
    "lin-M300N164K328-ms3": (6, 0, 3),
    "lin-M300N164K328-ms7": (6, 0, 7),
    "lin-M300N164K328-ms-4": (6, 0, 4),
    "lin-M300N36K256-ms3": (3, 0, 3),
    "conv-M384N160K72-ms0-conv2x16x12x8s1u0": (9, 0, 1),
    "conv-M96N36K648-ms0-conv2x16x12x72s2u0": (9, 0, 1),
    "conv-M120N164K648-ms0-conv2x5x3x72s1u1": (18, 0, 1),
    "conv-M12N160K576-ms0-conv3x2x2x64s1u0": (9, 0, 1),
    "conv-M384N160K72-ms3-conv2x16x12x8s1u0": (9, 0, 3),
    "conv-M96N36K648-ms3-conv2x16x12x72s2u0": (9, 0, 3),
    "conv-M120N164K648-ms3-conv2x5x3x72s1u1": (18, 0, 3),
    "conv-M12N160K576-ms3-conv3x2x2x64s1u0": (9, 0, 3),
    "conv-M120N36K648-ms7-conv2x6x10x64s1u0": (11, 0, 7),
}
