"""-m gpu: the implicit GEMM (gemm.hip, gemm_wide.hip), the batched Winograd path (winograd.hip), the weight gradient (wgrad.hip) and the
data-gradient call forms of the forward GEMM on EXACT data (inputs, fp64 references, case tables: tests/helpers_gemm.py; the conditions
that keep them honest, on the CPU: tests/test_gemm_inputs_cpu.py).  Legs, as the docstrings name them:
  A  forward on integer operands: the output equals the fp64 result rounded once, bit for bit (fp32 outputs: equals it);
  B  Winograd F(2x2, 3x3) on data whose U, V and M are exact in bf16: the same;
  C  the activations against fp64 act() of the exactly known pre-activation;
  D  (in every test) outputs, split-K slabs and dW live in NaN-canary allocations that must come back untouched outside M x N, and NaN
     surrounds A, W (rows after N, columns [K, ldw)) and dY;
  E  weight gradients (fp32, accumulated onto a non-zero start) and data gradients through the library's packers, exact.
Every test resets the census, asserts that it equals the plan's census key (plus splitk_reduce / conv_phase where planned) and prints one
"gemm exact" line before asserting (profiles/gemm_exact_parity.txt holds one run's lines)."""
import ctypes as C

import pytest
import torch

from difashion_amd import _lib
from tests import gpu_util as gu
from tests import helpers_gemm as hg
from tests import helpers_norm as hn
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

FORWARD = hg.forward_cases() + hg.FALLBACK_CASES


def _say(*parts):
    print("gemm exact", *parts)


def _dev(t):
    return None if t is None else t.to(DEV)


def _census():
    return {k: v for k, v in _lib.census().items() if v}


def _census_want(info, **more):
    want = {_lib.raw().dfh_census_name(info.census).decode(): 1}
    if info.split > 1:
        want["splitk_reduce"] = 1
    want.update(more)
    return want


def _plan(d, **extra):
    info = _lib.GemmPlanInfo()
    _lib.call("dfh_gemm_plan", C.byref(d), C.byref(_lib.GemmPlanExtra(**extra)), C.byref(info))
    return info


def _plan_text(info):
    return f"{info.line.decode().split('| ')[1]}"


class Operands:
    """the operands of a forward case on the device: A, W inside NaN allocations (8 NaN rows after M / N, W rows 8 NaN columns longer than
    K), the output and the split-K slabs as canary allocations (ld_out = N + 8, 8 rows after M, 4 KB either side)"""

    def __init__(self, c, inp, out_dtype=None):
        M, N = c["M"], c["N"]
        nb, rpb = hg.n_batches(c)
        om = c.get("out_mode", 0)
        self.keep = {}
        self.poison = {}
        if inp["x"] is not None:
            self.poison["conv_src"] = hg.poisoned(inp["x"].view(-1, c["C"]), 8, 0, device=DEV)
        for name in ("a0", "a1"):
            if inp[name] is not None:
                self.poison[name] = hg.poisoned(inp[name], 8, 0, device=DEV)
        w = inp["w"]
        if w.dim() == 3:                  # per-image weights: images of N rows, 8 NaN rows between them (w_img_stride = (N + 8) * ldw)
            st = torch.full((nb * (N + 8) - 8, w.shape[2]), float("nan"), dtype=w.dtype)
            for i in range(nb):
                st[i * (N + 8):i * (N + 8) + N] = w[i]
            w = st
        self.poison["W"] = hg.poisoned(w, 8, 8, device=DEV)
        for name in ("bias", "rowvec", "resid"):
            self.keep[name] = _dev(inp.get(name))
        dt = out_dtype or (torch.float32 if om in (2, 3) else torch.bfloat16)
        shape = (nb * N, rpb) if om in (1, 3) else (M, hg.out_cols(c))
        self.out = hg.poisoned(torch.empty(shape, dtype=dt), 8, 8, device=DEV, blank=True)
        self.keep["zero"] = gu.zero_page()
        self.d = hg.fill_desc(_lib.GemmDesc(), c, self.ptr)
        self.partial = None
        need = _lib.raw().dfh_gemm_partial_floats(C.byref(self.d))
        if need:
            self.partial = hg.poisoned(torch.empty((1, need), dtype=torch.float32), 0, 0, device=DEV, blank=True)
            self.d.partial, self.d.partial_floats = self.partial.ptr(), need

    def ptr(self, name):
        if name == "out":
            return self.out.ptr()
        return self.poison[name].ptr() if name in self.poison else self.keep[name].data_ptr()

    def result(self, c):
        """the output as the reference is laid out ([M][N]), on the CPU"""
        o = self.out.view.cpu()
        if c.get("out_mode", 0) in (1, 3):
            nb, rpb = hg.n_batches(c)
            o = o.view(nb, c["N"], rpb).transpose(1, 2).reshape(c["M"], c["N"])
        return o

    def broken(self):
        bad = [] if self.out.intact() else ["out"]
        if self.partial is not None and not self.partial.intact():
            bad.append("partial")
        return bad + [n for n, p in self.poison.items() if not p.intact()]


def _launch(c, inp, entry="dfh_gemm", out_dtype=None):
    """-> (Operands, plan info, census) of one launch of a forward case"""
    ops = Operands(c, inp, out_dtype)
    info = _plan(ops.d)
    _lib.census_reset()
    _lib.call(entry, C.byref(ops.d), gu.stream())
    torch.cuda.synchronize()
    return ops, info, _census()


# ----------------------------------------------------------------------------- leg A (and D)
@pytest.mark.parametrize("c", FORWARD, ids=hg.case_id)
def test_forward_is_the_fp64_result_rounded_once(c):
    """Leg A.  Linears and 3x3 convs (stride 1 / 2, nearest-2x upsample, two plain segments, fused 1x1 shortcut segments, transposed and fp32
    outputs, per-image weights, split-K 1 / 2 / 5 and the heuristic's own) on every instantiation the walks launch, at M in {bm - 1, bm + 1,
    3, a multiple}, N in {4, bn - 4, bn + 8, a multiple}, K segments in {8, 72, 200, 64 k}.  Integer operands, bias, row vector and
    residual: out == rounded_once(ref64) bit for bit; for fp32 outputs out == ref64.  Split-K 2 and 5 equal the single pass bit for bit
    because all three equal the same reference.  Leg D: every byte around the output and the split-K slabs is still the canary."""
    inp = hg.forward_inputs(c)
    ref = hg.forward_ref64(c, inp)
    ops, info, census = _launch(c, inp)
    got = ops.result(c)
    want = ref.float() if c.get("out_mode", 0) in (2, 3) else hg.rounded_once(ref)
    wrong = int((got != want).sum())
    broken = ops.broken()
    _say(hg.case_id(c), _plan_text(info), "census", census, "wrong", wrong, "of", want.numel(), "canaries_written", broken or "none")
    assert hg.want_plan(c) == (info.kernel, info.tile, info.bm, info.bn, info.stages, info.lean, info.wide, info.split, info.n_major)
    assert census == _census_want(info)
    assert torch.equal(got, want), f"{wrong} of {want.numel()} outputs differ from the fp64 result rounded once"
    assert not broken, broken


@pytest.mark.parametrize("nb,M,N,K,tile,inst", [(16, 130, 160, 64, 0, "e8_s4_lean"), (16, 300, 160, 72, 0, "e8_s4"), (4, 257, 328, 128, 21, "big_lean"),
                                                (3, 129, 136, 192, 5, "t128x128")])
def test_batched_planes_are_exact(nb, M, N, K, tile, inst):
    """Leg A, dfh_gemm_batched: 16 (4, 3) planes in one launch, each with its own A and W, planes of the output 8 canary rows apart.  (W in
    16 x 64 blocks is not reachable through dfh_gemm_batched; leg B runs it through dfh_conv3x3_wino.)"""
    c = dict(hg.lin(inst, M, N, K), force_tile=tile)
    a = hg.int_operand((nb, M, K), -3, 3, 41)
    w = hg.int_operand((nb, N, K), -3, 3, 42)
    bias = hg.int_operand((N,), -400, 400, 43, torch.float32)
    ref = torch.einsum("zmk,znk->zmn", a.double(), w.double()) + bias.double()
    nan = float("nan")
    a_st = torch.full((nb * (M + 8) - 8, K), nan, dtype=hg.BF16)
    w_st = torch.full((nb * (N + 8) - 8, K), nan, dtype=hg.BF16)
    for z in range(nb):
        a_st[z * (M + 8):z * (M + 8) + M] = a[z]
        w_st[z * (N + 8):z * (N + 8) + N] = w[z]
    pa, pw = hg.poisoned(a_st, 8, 0, device=DEV), hg.poisoned(w_st, 8, 8, device=DEV)
    out = hg.poisoned(torch.empty((nb * (M + 8) - 8, N), dtype=hg.BF16), 8, 8, device=DEV, blank=True)
    bias_d, z = _dev(bias), gu.zero_page()
    keep = dict(W=pw.ptr(), out=out.ptr(), a0=pa.ptr(), bias=bias_d.data_ptr(), zero=z.data_ptr())
    d = hg.fill_desc(_lib.GemmDesc(), dict(c, resid=False), keep.get)
    d.rowvec = None
    info = _plan(d, nbatch=nb)
    _lib.census_reset()
    _lib.call("dfh_gemm_batched", C.byref(d), nb, (M + 8) * K, (N + 8) * (K + 8), (M + 8) * (N + 8), gu.stream())
    torch.cuda.synchronize()
    census = _census()
    got = out.view.cpu()
    wrong, gaps = 0, 0
    for z in range(nb):
        wrong += int((got[z * (M + 8):z * (M + 8) + M] != hg.rounded_once(ref[z])).sum())
        if z + 1 < nb:
            gaps += int((got[z * (M + 8) + M:(z + 1) * (M + 8)].view(torch.int16) != hg.CANARY16).sum())
    _say(f"batched nb{nb} M{M} N{N} K{K} tile{tile}", _plan_text(info), "census", census, "wrong", wrong, "rows_between_planes_written", gaps,
         "canaries_written", "none" if out.intact() else "out")
    want = hg.INST[inst]         # (the 256 x 320 tile carries the batched default tile along as `tile`: not a property of the kernel that runs)
    assert (info.kernel, info.bm, info.bn, info.lean, info.split) == (want[1], want[3], want[4], want[6], 1) and (info.kernel or info.tile == want[2])
    assert census == _census_want(info)
    assert wrong == 0 and gaps == 0 and out.intact()


@pytest.mark.parametrize("B,rows,Cc,tile", [(3, 256, 160, 0), (2, 136, 128, 0), (2, 130, 160, 10)])
def test_second_destination_is_exact(B, rows, Cc, tile):
    """Leg A, dfh_gemm_out2: q | k row-major and V^T transposed per batch element from one launch."""
    M, N, K = B * rows, 3 * Cc, 72
    c = dict(hg.lin("e8_s4" if Cc == 160 else "t128x128", M, N, K), force_tile=tile, rows_per_b=rows)
    inp = hg.forward_inputs(c)
    ref = inp["acc"] + inp["bias"].double()
    pa, pw = hg.poisoned(inp["a0"], 8, 0, device=DEV), hg.poisoned(inp["w"], 8, 8, device=DEV)
    qk = hg.poisoned(torch.empty((M, 2 * Cc), dtype=hg.BF16), 8, 8, device=DEV, blank=True)
    vt = hg.poisoned(torch.empty((B * Cc, rows), dtype=hg.BF16), 8, 8, device=DEV, blank=True)
    bias, z = _dev(inp["bias"]), gu.zero_page()
    d = _lib.GemmDesc()
    d.a0, d.a0_c, d.W, d.ldw, d.M, d.N, d.bias, d.rows_per_b = pa.ptr(), K, pw.ptr(), K + 8, M, N, bias.data_ptr(), rows
    d.out, d.ld_out, d.zero_page, d.force_tile, d.force_order = qk.ptr(), 2 * Cc + 8, z.data_ptr(), tile, -1
    info = _plan(d, n_split=2 * Cc)
    _lib.census_reset()
    _lib.call("dfh_gemm_out2", C.byref(d), C.c_void_p(vt.ptr()), rows + 8, 2 * Cc, gu.stream())
    torch.cuda.synchronize()
    census = _census()
    want_qk = hg.rounded_once(ref[:, :2 * Cc])
    want_vt = hg.rounded_once(ref[:, 2 * Cc:]).view(B, rows, Cc).transpose(1, 2).reshape(B * Cc, rows)
    wrong = int((qk.view.cpu() != want_qk).sum()) + int((vt.view.cpu() != want_vt).sum())
    broken = [n for n, p in (("qk", qk), ("vt", vt)) if not p.intact()]
    _say(f"out2 B{B} rows{rows} C{Cc} tile{tile}", _plan_text(info), "census", census, "wrong", wrong, "canaries_written", broken or "none")
    assert census == _census_want(info)
    assert wrong == 0 and not broken


@pytest.mark.parametrize("B,cin,cout,H,W", [(3, 72, 40, 5, 7), (2, 64, 160, 1, 1), (2, 64, 320, 4, 6)])
def test_phase_planes_are_exact(B, cin, cout, H, W):
    """Leg A, dfh_conv_up2x: nearest-2x upsample + 3x3 conv as four 2x2 convs with summed taps.  Integer taps of [-1, 1]: the summed
    weights (dfh_ups_phase_fold) are integers of at most 4, exactly the fp64 tap sums, and the launch is the conv over the upsampled image."""
    x = hg.int_operand((B, H, W, cin), -3, 3, 51)
    w = hg.int_operand((cout, 9 * cin), -1, 1, 52)
    bias = hg.int_operand((cout,), -400, 400, 53, torch.float32)
    ref = hg.conv64(x, w, ups=1) + bias.double()
    px, pw = hg.poisoned(x.view(-1, cin), 8, 0, device=DEV), hg.poisoned(w, 8, 8, device=DEV)
    wp = hg.poisoned(torch.empty((4 * cout, 4 * cin), dtype=hg.BF16), 8, 0, device=DEV, blank=True)
    out = hg.poisoned(torch.empty((B * 4 * H * W, cout), dtype=hg.BF16), 8, 0, device=DEV, blank=True)
    bias_d, z = _dev(bias), gu.zero_page()
    _lib.call("dfh_ups_phase_fold", C.c_void_p(pw.ptr()), 9 * cin + 8, C.c_void_p(wp.ptr()), cout, cin, gu.stream())
    d = _lib.GemmDesc()
    d.conv_src, d.conv_c, d.conv, d.batch, d.Hin, d.Win, d.stride = px.ptr(), cin, 1, B, H, W, 1
    d.W, d.ldw, d.M, d.N, d.bias, d.out, d.ld_out, d.zero_page, d.force_order = wp.ptr(), 4 * cin, B * H * W, cout, bias_d.data_ptr(), out.ptr(), cout, z.data_ptr(), -1
    info = _plan(d, phase2x=1)
    _lib.census_reset()
    _lib.call("dfh_conv_up2x", C.c_void_p(px.ptr()), B, H, W, cin, C.c_void_p(wp.ptr()), cout, _lib.ptr(bias_d), C.c_void_p(out.ptr()), _lib.ptr(z), gu.stream())
    torch.cuda.synchronize()
    census = _census()
    # the fp64 tap sums per phase: [4][N][4 C]
    w4 = w.double().view(cout, 3, 3, cin)
    grp = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
    sums = torch.zeros(4, cout, 4, cin, dtype=torch.float64)
    for py in (0, 1):
        for pxx in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    for ky in grp[py][a]:
                        for kx in grp[pxx][b]:
                            sums[py * 2 + pxx, :, a * 2 + b] += w4[:, ky, kx]
    wp_wrong = int((wp.view.cpu() != sums.reshape(4 * cout, 4 * cin).to(hg.BF16)).sum())
    wrong = int((out.view.cpu() != hg.rounded_once(ref)).sum())
    broken = [n for n, p in (("out", out), ("wp", wp)) if not p.intact()]
    _say(f"phase planes B{B} {cin}->{cout}@{H}x{W}", _plan_text(info), "census", census, "summed_weights_wrong", wp_wrong, "wrong", wrong,
         "canaries_written", broken or "none")
    assert census == _census_want(info, conv_phase=1)
    assert wp_wrong == 0 and wrong == 0 and not broken


# ----------------------------------------------------------------------------- leg B
@pytest.mark.parametrize("case", hg.WINO_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_winograd_is_exact(case):
    """Leg B.  x in [-1, 1] and two-channel taps of {-8 .. 8} keep U, V and M exact in bf16 (helpers_gemm.wino_inputs), so dfh_wino_weights
    equals the fp64 U bit for bit in both layouts, dfh_wino_input the fp64 V, and dfh_conv3x3_wino with an integer bias, time-embedding row
    and residual the conv rounded once.  Where the shape allows it the fused GroupNorm input transform and the chained form run on the same
    weights too, held to their own tolerance (rel L2 <= 2e-3 between fused and unfused: tests/test_gpu_ops.py), where a wrong channel or tap
    is a gross error."""
    B, cin, cout, H, W, resid, temb = case
    inp = hg.wino_inputs(case)
    U64, V64, _ = hg.wino_intermediates(inp)
    ref = hg.wino_ref64(case, inp)
    mt = B * (H // 2) * (W // 2)
    pw = hg.poisoned(hg.pack_conv64(inp["w"]).to(hg.BF16), 8, 8, device=DEV)
    px = hg.poisoned(inp["x"].view(-1, cin), 8, 0, device=DEV)
    u_wrong = {}
    blocked = _lib.raw().dfh_wino_blocked(cout, cin)
    layouts = [0] + ([1] if cout % 16 == 0 and cin % 64 == 0 else [])
    Us = {}
    for lay in layouts:
        U = hg.poisoned(torch.empty((16 * cout, cin), dtype=hg.BF16), 8, 0, device=DEV, blank=True)
        _lib.call("dfh_wino_weights", C.c_void_p(pw.ptr()), 9 * cin + 8, C.c_void_p(U.ptr()), cout, cin, lay, gu.stream())
        torch.cuda.synchronize()
        u = U.view.cpu().view(16, cout, cin)
        if lay:
            u = U.view.cpu().view(16, cout // 16, cin // 64, 16, 64).permute(0, 1, 3, 2, 4).reshape(16, cout, cin)
        u_wrong[lay] = int((u != U64.to(hg.BF16)).sum()) + (0 if U.intact() else 1)
        Us[lay] = U
    V = hg.poisoned(torch.empty((16 * mt, cin), dtype=hg.BF16), 8, 0, device=DEV, blank=True)
    _lib.call("dfh_wino_input", C.c_void_p(px.ptr()), C.c_void_p(V.ptr()), B, H, W, cin, gu.stream())
    torch.cuda.synchronize()
    v_wrong = int((V.view.cpu().view(16, mt, cin) != V64.to(hg.BF16)).sum()) + (0 if V.intact() else 1)
    out = hg.poisoned(torch.empty((B * H * W, cout), dtype=hg.BF16), 8, 0, device=DEV, blank=True)
    nbytes = _lib.raw().dfh_conv3x3_wino_scratch_bytes(B, H, W, cin, cout)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    bias, rv, res, z = _dev(inp["bias"]), _dev(inp["rowvec"]), _dev(inp["resid"]), gu.zero_page()
    use = blocked if blocked in Us else 0
    d = _lib.GemmDesc()
    d.a0, d.a0_c, d.W, d.ldw, d.M, d.N, d.out, d.ld_out, d.zero_page, d.force_order = V.ptr(), cin, Us[use].ptr(), cin, mt, cout, out.ptr(), cout, z.data_ptr(), -1
    info = _plan(d, nbatch=16, w_blocked=use)
    _lib.census_reset()
    _lib.call("dfh_conv3x3_wino", C.c_void_p(px.ptr()), B, H, W, cin, C.c_void_p(Us[use].ptr()), use, cout, _lib.ptr(bias), _lib.ptr(rv),
              3 * cout if temb else 0, cout if temb else 0, _lib.ptr(res), C.c_void_p(out.ptr()), _lib.ptr(scratch), nbytes, _lib.ptr(z), gu.stream())
    torch.cuda.synchronize()
    census = _census()
    wrong = int((out.view.cpu() != hg.rounded_once(ref)).sum())
    _say(f"winograd B{B} {cin}->{cout}@{H}x{W} blocked{use}", _plan_text(info), "census", census, "U_wrong", u_wrong, "V_wrong", v_wrong, "wrong", wrong,
         "of", ref.numel(), "canaries_written", "none" if out.intact() else "out")
    gemm_key = _lib.raw().dfh_census_name(info.census).decode()
    assert census.get(gemm_key) == 1 and not [k for k in census if k.startswith("gemm_") and k != gemm_key], census
    assert not any(u_wrong.values()) and v_wrong == 0
    assert wrong == 0 and out.intact()
    if _lib.raw().dfh_gn_wino_input_ok(cin, 0, 32, H, W) and cin % 32 == 0:
        _fused_groupnorm_transforms(case, inp, px, mt)


def _fused_groupnorm_transforms(case, inp, px, mt):
    """dfh_gn_wino_input against dfh_groupnorm + dfh_wino_input, and dfh_gn_wino_input_chain against the materialised path, on the exact
    case's tensors: rel L2 <= 2e-3, the bound those pairs have in tests/test_gpu_ops.py"""
    B, cin, cout, H, W, resid, temb = case
    G = 32
    gamma, beta = 1.0 + 0.1 * gu.rnd(cin, seed=42), 0.1 * gu.rnd(cin, seed=43)
    Vf = torch.empty(16, mt, cin, dtype=hg.BF16, device=DEV)
    _lib.call("dfh_gn_wino_input", C.c_void_p(px.ptr()), cin, None, 0, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, G, _lib.ptr(Vf), B, H, W, gu.stream())
    gn = torch.empty(B * H * W, cin, dtype=hg.BF16, device=DEV)
    part = torch.empty(B * 64 * G * 2, dtype=torch.float32, device=DEV)
    _lib.call("dfh_groupnorm", C.c_void_p(px.ptr()), cin, None, 0, B, H * W, G, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, 1, _lib.ptr(gn), _lib.ptr(part), gu.stream())
    Vu = torch.empty_like(Vf)
    _lib.call("dfh_wino_input", _lib.ptr(gn), _lib.ptr(Vu), B, H, W, cin, gu.stream())
    torch.cuda.synchronize()
    fused = gu.rel_err(Vf.float(), Vu.float())
    # the chained form: conv1's planes M (here: the exact V of the case as stand-in planes of cin channels) -> output transform + bias ->
    # GroupNorm + SiLU -> input transform, against the same steps materialised
    Mp = Vu
    pb = hg.int_operand((cin,), -2, 2, 61, torch.float32).to(DEV)
    Vc = torch.empty_like(Vf)
    _lib.call("dfh_gn_wino_input_chain", _lib.ptr(Mp), _lib.ptr(pb), None, 0, 0, cin, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, G, _lib.ptr(Vc), B, H, W, gu.stream())
    AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1.]], device=DEV)
    y = torch.einsum("ij,jkbyxc,lk->byixlc", AT, Mp.float().view(4, 4, B, H // 2, W // 2, cin), AT).reshape(B, H, W, cin) + pb
    h1 = y.to(hg.BF16)
    Vm = torch.empty_like(Vf)
    _lib.call("dfh_gn_wino_input", _lib.ptr(h1), cin, None, 0, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, G, _lib.ptr(Vm), B, H, W, gu.stream())
    torch.cuda.synchronize()
    chain = gu.rel_err(Vc.float(), Vm.float())
    _say(f"winograd B{B} C{cin}@{H}x{W} fused GroupNorm transform vs two launches rel_l2 {fused:.3e} chained vs materialised {chain:.3e} (<= 2e-3)")
    assert fused <= 2e-3 and chain <= 2e-3


# ----------------------------------------------------------------------------- leg C
def _act_check(name, got, ref, model):
    """the project's rule (helpers_norm.FACTOR x the reference's own rounding, relative L2) and, elementwise where the reference is a normal
    bf16 number, at most FACTOR_ULPS bf16 ulps of the reference -- or, where the documented fp32 approximation (helpers_gemm.act_model32,
    stored as bf16 like the kernel's) is further off, what that model is off by plus one bf16 ulp of the value stored: the hardware
    reciprocal and exp2 are 1-ulp fp32 operations, not correctly rounded ones, and a few fp32 ulps can move the bf16 store by one step.
    (In GELU's negative tail the polynomial's 5.5e-7 absolute error dwarfs a reference of 1e-30: there the model is the only meaningful
    bound.)  -> the figures, printed before they are asserted"""
    rel, yard = hg.rel_l2(got, ref), hg.yardstick(ref)
    normal = ref.abs() >= 2.0 ** -126
    u = hg.ulps(got, ref)[normal]
    stored = model.to(hg.BF16).double()
    mu = hg.ulps(stored, ref)[normal]
    step = torch.maximum(hg.bf16_ulp(stored), hg.bf16_ulp(ref))[normal] / hg.bf16_ulp(ref)[normal]
    allowed = torch.maximum(torch.full_like(mu, float(hg.FACTOR_ULPS)), mu + step)
    over = int((u > allowed).sum()) + int((got.double()[ref == 0] != 0).sum())          # act(0) = 0 exactly, for all six
    worst_plain = float(u[mu <= 1.0].max()) if bool((mu <= 1.0).any()) else 0.0
    for i in torch.nonzero(u > allowed).flatten()[:6].tolist():        # the first offenders, for the record
        _say(name.split()[0], f"over: ref {float(ref[normal][i]):.9e} got {float(got.double()[normal][i]):.9e} model {float(model[normal][i]):.9e} "
                              f"ulps {float(u[i]):.3f} allowed {float(allowed[i]):.3f}")
    _say(name, f"rel_l2 {rel:.3e} yardstick {yard:.3e} ratio {rel / yard:.3f} (<= {hn.FACTOR}) max_ulps {float(u.max()):.3f} "
               f"max_ulps_where_model_within_1 {worst_plain:.3f} (<= {hg.FACTOR_ULPS}) model_max_ulps {float(mu.max()):.3e} elements_over {over}")
    return rel, yard, over


@pytest.mark.parametrize("a", hg.ACT_CASES, ids=lambda a: f"act{a[0]}-{a[1]}")
def test_activation_of_an_exact_preactivation(a):
    """Leg C.  Operands on a 2^-4 grid: the epilogue's input acc + bias + rowvec is known exactly, spans about [-12, 12] and holds exact
    0 and both sides of SiLU's minimum; the stored output is held to fp64 act() of it.  SiLU, leaky-ReLU, tanh on the eight-wave, wide and
    256 x 320 epilogues; exact-erf GELU and quick-GELU on the XACT instantiation (the plan sends them there whatever is pinned)."""
    c = hg.act_case(*a)
    inp = hg.act_inputs(c)
    _, rpb = hg.n_batches(c)
    pre = hg.pre64(inp["acc"], inp["bias"], inp["rowvec"], c["N"], rpb)
    ref = hg.ACT64[c["act"]](pre)
    ops, info, census = _launch(c, inp)
    got = ops.result(c)
    broken = ops.broken()
    rel, yard, over = _act_check(f"{hg.case_id(c)} {_plan_text(info)} census {census} canaries_written {broken or 'none'}", got, ref,
                                 hg.act_model32(pre, c["act"]))
    assert hg.want_plan(c) == (info.kernel, info.tile, info.bm, info.bn, info.stages, info.lean, info.wide, info.split, info.n_major)
    assert census == _census_want(info) and not broken
    assert rel <= hn.FACTOR * yard and over == 0


@pytest.mark.parametrize("inst,M,N,K", hg.ACT_GEGLU, ids=lambda v: str(v))
def test_geglu_of_exact_preactivations(inst, M, N, K):
    """Leg C, GEGLU (packed value / gate blocks, bias only) on the 256 x 256 tile, the 128 x 128 tile, the wide 256 x 128 sibling's
    in-register epilogue and the wide 256 x 160 kernel.  (The training launch with pre_out, gemm_wide variant 5, has no C ABI entry.)"""
    c = hg.lin(inst, M, N, K, act=4)
    inp = hg.act_inputs(c)
    pre = hg.pre64(inp["acc"], inp["bias"])
    val, gate = hg.geglu_split(pre)
    ref = val * hg.gelu64(gate)
    ops, info, census = _launch(c, inp)
    got = ops.result(c)
    broken = ops.broken()
    model = (val * hg.act_model32(gate, 4)).to(torch.float32).double()
    rel, yard, over = _act_check(f"{hg.case_id(c)} {_plan_text(info)} census {census} canaries_written {broken or 'none'}", got, ref, model)
    assert hg.want_plan(c) == (info.kernel, info.tile, info.bm, info.bn, info.stages, info.lean, info.wide, info.split, info.n_major)
    assert census == _census_want(info) and not broken
    assert rel <= hn.FACTOR * yard and over == 0


# ----------------------------------------------------------------------------- leg E
def _wgrad(c, inp):
    """dfh_gemm_wgrad of a case: dW [N][K] inside a sentinel matrix of ldw = K + 8 (+ col_off) columns and 8 rows after N; dY rows of
    ldy = ((N + 7) & ~7) + 8 columns (the launcher wants ldy % 8 == 0).  The kernel's contract ldy >= (N + 7) & ~7 lets it load up to
    the next multiple of 8, so finite poison 1e30 fills columns [N, (N + 7) & ~7) and NaN the eight after them and the rows after M"""
    M, N, K = c["M"], c["N"], hg.k_total(c)
    off = c.get("col_off", 0)
    poison = {}
    if inp["x"] is not None:
        poison["conv_src"] = hg.poisoned(inp["x"].view(-1, c["C"]), 8, 0, device=DEV)
    for name in ("a0", "a1"):
        if inp[name] is not None:
            poison[name] = hg.poisoned(inp[name], 8, 0, device=DEV)
    n8 = (N + 7) & ~7
    dy_wide = torch.full((M, n8), 1e30, dtype=hg.BF16)
    dy_wide[:, :N] = inp["dy"]
    pdy = hg.poisoned(dy_wide, 8, 8, device=DEV)
    wide = torch.full((N, off + K), -7.0, dtype=torch.float32)          # columns [0, off) belong to someone else: a sentinel that is a number
    wide[:, off:] = inp["dw0"]
    pdw = hg.poisoned(wide, 8, 8, device=DEV)
    z = gu.zero_page()
    keep = dict(zero=z.data_ptr(), W=0, out=0, **{n: p.ptr() for n, p in poison.items()})
    d = hg.fill_desc(_lib.GemmDesc(), dict(c, inst="e8_s4"), lambda n: keep.get(n))
    d.bias, d.rowvec, d.resid, d.W, d.out = None, None, None, None, None
    need = _lib.raw().dfh_gemm_wgrad_partial_floats(C.byref(d), c["msplit"])
    part = hg.poisoned(torch.empty((1, max(need, 1)), dtype=torch.float32), 0, 0, device=DEV, blank=True)
    d.partial, d.partial_floats = part.ptr(), need
    ldw = off + K + 8
    _lib.call("dfh_gemm_wgrad", C.byref(d), C.c_void_p(pdy.ptr()), n8 + 8, C.c_void_p(pdw.ptr() + 4 * off), ldw, c["msplit"], gu.stream())
    torch.cuda.synchronize()
    got = pdw.view.cpu()
    broken = [n for n, p in (("dW", pdw), ("partial", part)) if not p.intact()]
    if off and not bool((got[:, :off] == -7.0).all()):
        broken.append("dW columns before the offset")
    return got[:, off:], broken


@pytest.mark.parametrize("c", hg.wgrad_cases(), ids=hg.wgrad_id)
def test_weight_gradient_is_exact(c):
    """Leg E.  dW += dY^T A on integers, onto a non-zero integer start: dW == ref64 as fp32, for the linear, the two-source form at a
    column offset, conv3x3 (stride 1 / 2, upsample, conv_c 8 and 72, H = 2, non-square) and conv + shortcut segments; msplit in
    {0, 1, 3, 7, -4}, M in {8, 130, 300} (ragged slices), N in {4, 36, 160, 164}.  Sentinel columns [K, ldw), the columns before the
    offset, the rows after N and the slab buffer beyond its size come back unchanged.  (The fused dbias of WgradArgs is not reachable
    through dfh_gemm_wgrad.)"""
    inp = hg.wgrad_inputs(c)
    got, broken = _wgrad(c, inp)
    want = inp["ref"].float()
    wrong = int((got != want).sum())
    _say("wgrad", hg.wgrad_id(c), "plan (tiles, whole, slices)", hg.WGRAD_PLANS[hg.wgrad_id(c)], "wrong", wrong, "of", want.numel(), "canaries_written", broken or "none")
    assert torch.equal(got, want) and not broken


@pytest.mark.parametrize("groups,rows,N", [(1, 300, 168), (3, 100, 160), (5, 7, 40)])
def test_colsum_is_exact(groups, rows, N):
    """Leg E, dfh_colsum (bias gradient: one group; time-embedding gradient: a group per image), accumulated onto a non-zero start inside a
    wider matrix whose other columns must not change (N and ldy multiples of 8: the launcher's contract)."""
    dy = hg.int_operand((groups * rows, N), -3, 3, 71)
    start = hg.int_operand((groups, N), -50, 50, 72, torch.float32)
    pdy = hg.poisoned(dy, 8, 8, device=DEV)
    out = hg.poisoned(start, 8, 8, device=DEV)
    _lib.call("dfh_colsum", C.c_void_p(pdy.ptr()), N + 8, N, groups, rows, C.c_void_p(out.ptr()), N + 8, gu.stream())
    torch.cuda.synchronize()
    want = (start.double() + dy.double().view(groups, rows, N).sum(1)).float()
    wrong = int((out.view.cpu() != want).sum())
    _say(f"colsum groups{groups} rows{rows} N{N} wrong {wrong} canaries_written {'none' if out.intact() else 'out'}")
    assert wrong == 0 and out.intact()


@pytest.mark.parametrize("M,N,K,tile", [(300, 328, 200, 0), (130, 160, 72, 6)])
def test_data_gradient_of_a_linear_is_exact(M, N, K, tile):
    """Leg E.  dX = dY W through dfh_pack_matrix_t (the transposed pack) and the forward GEMM."""
    w = hg.int_operand((N, K), -3, 3, 81, torch.float32)
    dy = hg.int_operand((M, N), -3, 3, 82)
    wt = hg.poisoned(torch.empty((K, N), dtype=hg.BF16), 8, 8, device=DEV, blank=True)
    _lib.call("dfh_pack_matrix_t", _lib.ptr(_dev(w)), C.c_void_p(wt.ptr()), N, K, N + 8, 0, 0, 0, gu.stream())
    torch.cuda.synchronize()
    packed_wrong = int((wt.view.cpu() != w.T.to(hg.BF16)).sum()) + (0 if wt.intact() else 1)
    pdy = hg.poisoned(dy, 8, 0, device=DEV)
    out = hg.poisoned(torch.empty((M, K), dtype=hg.BF16), 8, 8, device=DEV, blank=True)
    z = gu.zero_page()
    d = _lib.GemmDesc()
    d.a0, d.a0_c, d.W, d.ldw, d.M, d.N, d.out, d.ld_out, d.zero_page, d.force_tile, d.force_order = pdy.ptr(), N, wt.ptr(), N + 8, M, K, out.ptr(), K + 8, z.data_ptr(), tile, -1
    info = _plan(d)
    _lib.census_reset()
    _lib.call("dfh_gemm", C.byref(d), gu.stream())
    torch.cuda.synchronize()
    census = _census()
    wrong = int((out.view.cpu() != hg.rounded_once(dy.double() @ w.double())).sum())
    _say(f"dgrad linear M{M} N{N} K{K}", _plan_text(info), "census", census, "pack_wrong", packed_wrong, "wrong", wrong, "canaries_written", "none" if out.intact() else "out")
    assert census == _census_want(info)
    assert packed_wrong == 0 and wrong == 0 and out.intact()


@pytest.mark.parametrize("cin,cout,H,W,stride,ups", [(64, 72, 6, 10, 1, 0), (8, 72, 5, 3, 1, 0), (64, 64, 12, 20, 2, 0), (72, 64, 5, 3, 1, 1), (64, 128, 2, 2, 1, 0)])
def test_data_gradient_of_a_conv_is_exact(cin, cout, H, W, stride, ups):
    """Leg E.  dX = conv3x3(dY, flipped / transposed W) through dfh_pack_conv3x3_t: stride 1 directly, stride 2 over the zero-inserted dY
    (upsample = 2), nearest-2x upsample + conv as the data gradient at 2H x 2W followed by dfh_pool2x2_sum, whose sums of four integers
    round once more.  The reference is the fp64 autograd gradient of the forward conv.  (The phase-plane data gradient, GemmArgs::phase2x = 2,
    is set by the training walk only: no C ABI entry reaches it.)"""
    B = 2
    Ho, Wo = (2 * H, 2 * W) if ups else (H // stride, W // stride)
    w = hg.int_operand((cout, cin, 3, 3), -3, 3, 91, torch.float32)
    dy = hg.int_operand((B, Ho, Wo, cout), -3, 3, 92)
    x = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
    xin = x.repeat_interleave(2, 2).repeat_interleave(2, 3) if ups else x
    y = torch.nn.functional.conv2d(xin, w.double(), stride=stride, padding=1)
    (ref,) = torch.autograd.grad(y, x, dy.double().permute(0, 3, 1, 2))
    ref = ref.permute(0, 2, 3, 1).reshape(B * H * W, cin)
    wt = hg.poisoned(torch.empty((cin, 9 * cout), dtype=hg.BF16), 8, 8, device=DEV, blank=True)
    _lib.call("dfh_pack_conv3x3_t", _lib.ptr(_dev(w)), C.c_void_p(wt.ptr()), cout, cin, 9 * cout + 8, 0, cout, gu.stream())
    pdy = hg.poisoned(dy.view(-1, cout), 8, 0, device=DEV)
    Hd, Wd = (H, W) if stride == 2 else (Ho, Wo)                  # the image the data-gradient conv writes
    out = hg.poisoned(torch.empty((B * Hd * Wd, cin), dtype=hg.BF16), 8, 8, device=DEV, blank=True)
    z = gu.zero_page()
    d = _lib.GemmDesc()
    d.conv_src, d.conv_c, d.conv, d.batch, d.Hin, d.Win, d.stride, d.upsample = pdy.ptr(), cout, 1, B, Ho, Wo, 1, 2 if stride == 2 else 0
    d.W, d.ldw, d.M, d.N, d.out, d.ld_out, d.zero_page, d.force_order = wt.ptr(), 9 * cout + 8, B * Hd * Wd, cin, out.ptr(), cin + 8, z.data_ptr(), -1
    need = _lib.raw().dfh_gemm_partial_floats(C.byref(d))
    part = hg.poisoned(torch.empty((1, max(need, 1)), dtype=torch.float32), 0, 0, device=DEV, blank=True)
    d.partial, d.partial_floats = part.ptr(), need
    info = _plan(d)
    _lib.census_reset()
    _lib.call("dfh_gemm", C.byref(d), gu.stream())
    torch.cuda.synchronize()
    census = _census()
    got = out.view.cpu()
    broken = [n for n, p in (("out", out), ("partial", part), ("wt", wt)) if not p.intact()]
    if ups:
        # the conv's own result is exact (|dX| < 256 * ... integers): check it, then the pool's single rounding of the sums of four
        full = got.contiguous().to(DEV)
        pooled = hg.poisoned(torch.empty((B * H * W, cin), dtype=hg.BF16), 8, 0, device=DEV, blank=True)
        _lib.call("dfh_pool2x2_sum", _lib.ptr(full), C.c_void_p(pooled.ptr()), B, H, W, cin, gu.stream())
        torch.cuda.synchronize()
        four = got.double().view(B, H, 2, W, 2, cin).sum((2, 4)).reshape(B * H * W, cin)
        wrong = int((pooled.view.cpu() != hg.rounded_once(four)).sum())
        # the conv at 2H x 2W against fp64: the sum over the four pixels of its exact value is the reference
        xg = torch.zeros(B, cin, Ho, Wo, dtype=torch.float64, requires_grad=True)
        (r2,) = torch.autograd.grad(torch.nn.functional.conv2d(xg, w.double(), padding=1), xg, dy.double().permute(0, 3, 1, 2))
        wrong += int((got != hg.rounded_once(r2.permute(0, 2, 3, 1).reshape(-1, cin))).sum())
        if not pooled.intact():
            broken.append("pooled")
    else:
        wrong = int((got != hg.rounded_once(ref)).sum())
    _say(f"dgrad conv {cin}->{cout}@{H}x{W} s{stride} u{ups}", _plan_text(info), "census", census, "wrong", wrong, "canaries_written", broken or "none")
    assert census == _census_want(info)
    assert wrong == 0 and not broken
