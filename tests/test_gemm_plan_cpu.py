"""CPU (-m "not gpu"): which kernel, tile, K split, tile order and statistics chunk every GEMM launch of the walks gets -- dfh_gemm_plan
(host code, nothing is launched) against tests/golden/gemm_plan_table.txt.

The golden file was recorded from the PARENT of the commit that split gemm_launch into gemm_plan + dispatch: the parent built with
profiles/gemm_plan/parent_dump.patch (a stub dfh_gemm_plan over its own selection code), loaded through DFH_LIB, then

    DFH_LIB=<parent>/libdifashion_hip.so DFH_LIB_ALLOW_ABI_MISMATCH=1 python -m tests.test_gemm_plan_cpu --record

so the yardstick is the old selection, never the code under test.  The file holds one line per row of TABLE under [default], and under
[<VAR>=<value>] the rows whose line that switch changes ("<row index>: <line>"), each recorded from the parent in a fresh process."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from difashion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_table.txt")
KNOBS = ["DFH_GEMM_BIG=0", "DFH_DEEP4=0", "DFH_DEEP4=1", "DFH_TMAP=4,8", "DFH_GSTAT128=0"]
PTR = 4096                      # a made-up address: the plan tests pointers for presence only
EXTRA = ("nbatch", "phase2x", "w_blocked", "n_split", "want_rowstat", "ln_cnt", "pre_out")


def lin(M, K, N, K1=0, **kw):
    kw.setdefault("ld_out", N // 2 if kw.get("act") == 4 else N)
    return dict(M=M, N=N, a0=PTR, a0_c=K, a1=PTR if K1 else None, a1_c=K1, ldw=K + K1, **kw)


def conv(B, H, C, N, K0=0, stride=1, ups=0, W=None, **kw):
    W = W or H
    Ho, Wo = (H * 2, W * 2) if ups else (H // stride, W // stride)
    kw.setdefault("rows_per_b", Ho * Wo)
    return dict(M=B * Ho * Wo, N=N, conv=1, conv_src=PTR, conv_c=C, batch=B, Hin=H, Win=W, stride=stride, upsample=ups,
                a0=PTR if K0 else None, a0_c=K0, ldw=9 * C + K0, **dict(dict(ld_out=N), **kw))


def gn(N, hw):
    return dict(gstat_cpg=N // 32, gstat_hw=hw)


def build_table():
    t = []
    for B in (16, 1):
        for H, Cc in ((64, 320), (32, 640), (16, 1280), (8, 1280)):
            hw, M = H * H, B * H * H
            # resnet convs: conv1 (time-embedding row vector, statistics for norm2), conv2 (+ residual), with the concatenated skip and
            # with the 1x1 shortcut as a plain segment
            t.append(conv(B, H, Cc, Cc, rowvec=PTR, rv_ld=2 * Cc, **gn(Cc, hw)))
            t.append(conv(B, H, Cc, Cc, resid=PTR, ld_res=Cc, **gn(Cc, hw)))
            t.append(conv(B, H, 2 * Cc, Cc, rowvec=PTR, rv_ld=2 * Cc, **gn(Cc, hw)))
            t.append(conv(B, H, Cc, Cc, K0=2 * Cc, **gn(Cc, hw)))
            if Cc > 320:
                t.append(conv(B, H, Cc // 2, Cc, rowvec=PTR, rv_ld=2 * Cc, **gn(Cc, hw)))
                t.append(conv(B, H, Cc, Cc, K0=Cc // 2, **gn(Cc, hw)))
                t.append(conv(B, H, Cc + Cc // 2, Cc, rowvec=PTR, rv_ld=2 * Cc, **gn(Cc, hw)))
            if H > 8:
                t.append(conv(B, H, Cc, Cc, stride=2, **gn(Cc, hw // 4)))                    # downsampler
                t.append(conv(B, H // 2, Cc, Cc, ups=1, **gn(Cc, hw)))                       # upsampler, direct ...
                t.append(dict(conv(B, H // 2, Cc, Cc), phase2x=1))                           # ... and as four phase planes
            if H == 8:
                continue
            # transformer block: token linears K = C with / without residual and row statistics, q | k | v, GEGLU, 4C + C -> C
            t.append(lin(M, Cc, Cc))
            t.append(lin(M, Cc, Cc, resid=PTR, ld_res=Cc))
            t.append(lin(M, Cc, Cc, resid=PTR, ld_res=Cc, want_rowstat=1))
            t.append(lin(M, Cc, Cc, ln_cnt=160))
            t.append(lin(M, Cc, 3 * Cc, rows_per_b=hw, n_split=2 * Cc, ln_cnt=160))
            t.append(lin(M, Cc, 3 * Cc, rows_per_b=hw, n_split=2 * Cc))
            t.append(lin(M, Cc, Cc, rows_per_b=hw, out_mode=1, ld_out=hw))                   # V^T
            t.append(lin(M, Cc, 8 * Cc, act=4))
            t.append(lin(M, Cc, 8 * Cc, act=4, ln_cnt=160))
            t.append(lin(M, Cc, 8 * Cc, act=4, pre_out=1))
            t.append(lin(M, 4 * Cc, Cc, resid=PTR, ld_res=Cc, want_rowstat=1))
            t.append(lin(M, 4 * Cc, Cc, K1=Cc, **gn(Cc, hw)))
            t.append(lin(M, Cc, Cc, rows_per_b=hw, rowvec=PTR, rv_ld=Cc, w_img_stride=Cc * Cc, want_rowstat=1))   # GroupNorm folded into proj_in
            for ctx in (768, 1024):                                                           # text K / V (SD-1.5 / SD-2-base widths)
                t.append(lin(B * 77, ctx, Cc))
                t.append(lin(B * 77, ctx, Cc, rows_per_b=77, out_mode=1, ld_out=80))
        t.append(conv(B, 64, 8, 320, **gn(320, 4096)))                                      # conv_in: K = 8 * 9
        t.append(conv(B, 64, 320, 8, out_mode=3, ld_out=4096))                              # conv_out: N = 8, fp32 NCHW
        t.append(lin(B, 320, 1280, act=1))                                                    # time embedding
        t.append(lin(B, 1280, 1280))
        t.append(lin(B, 1280, 1280, act=1))
    # Winograd planes: 16 planes of 256 / 1024 rows, U blocked and not; a 4096-row level for the batched 256 x 320 tile
    for rows in (256, 1024, 4096):
        for K in (1280, 2560):
            for blocked in (1, 0):
                t.append(lin(rows, K, 1280 if rows < 4096 else 640, nbatch=16, w_blocked=blocked))
    t.append(lin(1024, 1280, 1280, nbatch=16, force_tile=1))
    # the VAE's convs at 256 x 256 and 512 x 512, batch 1
    for H in (256, 512):
        for Cv in (128, 256, 512):
            t.append(conv(1, H, Cv, Cv, **gn(Cv, H * H)))
            t.append(conv(1, H, Cv, Cv, resid=PTR, ld_res=Cv))
        t.append(conv(1, H, 256, 128, **gn(128, H * H)))
        t.append(conv(1, H, 128, 8, act=3, out_mode=3, ld_out=H * H))
    t.append(lin(4096, 512, 512, rows_per_b=4096, rowvec=PTR, rv_ld=512, w_img_stride=512 * 512))
    # a 96 x 96 latent level: 72 chunks of 128 rows exceed what the consuming GroupNorm takes -> the 128-row writer must refuse
    t.append(conv(1, 96, 320, 320, **gn(320, 9216)))
    t.append(conv(2, 96, 320, 320, **gn(320, 9216)))
    t.append(conv(16, 96, 320, 320, **gn(320, 9216)))
    unforced = len(t)
    # every force id the tests and scripts use, on a launch that can take it and on launches that cannot (fp32 output, GEGLU)
    for ft in (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 20, 21, 23, 24, 30):
        t.append(lin(57344, 640, 640, resid=PTR, ld_res=640, force_tile=ft, **gn(640, 4096)))
        t.append(lin(4096, 320, 320, out_mode=2, force_tile=ft))
        t.append(lin(57344, 320, 2560, act=4, force_tile=ft))
    t.append(conv(14, 64, 128, 320, force_tile=21))
    t.append(lin(4096, 1280, 320, force_split=2))
    t.append(lin(4096, 320, 320, force_split=100))                                            # clamped to the 5 k-steps
    t.append(lin(4096, 320, 2560, act=4, force_split=2))
    t.append(lin(4096, 1280, 320, force_order=2))
    t.append(conv(16, 16, 1280, 1280, force_order=3))
    t.append(lin(1024, 1280, 1280, nbatch=16, force_split=2))
    # launches that must be refused
    t.append(lin(4096, 320, 322))
    t.append(lin(4096, 324, 320))
    t.append(lin(4096, 320, 2560, act=4, resid=PTR, ld_res=1280))
    t.append(lin(4096, 320, 320, n_split=100))
    t.append(lin(256, 5120, 320, ln_cnt=160))
    t.append(lin(4096, 320, 640, act=4, pre_out=1, ln_cnt=160))
    t.append(lin(4096, 320, 320, rows_per_b=100, w_img_stride=320 * 320))
    t.append(lin(4096, 320, 200, nbatch=16, w_blocked=1))
    return t, unforced


TABLE, UNFORCED = build_table()


def plan(row):
    d = _lib.GemmDesc()
    d.force_order, d.W, d.out, d.zero_page = -1, PTR, PTR, PTR
    x = _lib.GemmPlanExtra()
    for k, v in row.items():
        setattr(x if k in EXTRA else d, k, v if k != "want_rowstat" else 1)
    info = _lib.GemmPlanInfo()
    rc = _lib.raw().dfh_gemm_plan(C.byref(d), C.byref(x), C.byref(info))
    return rc, info, d


def lines():
    return [plan(r)[1].line.decode() for r in TABLE]


def read_golden():
    sections, cur = {}, None
    for ln in open(GOLDEN).read().splitlines():
        if ln.startswith("["):
            cur = sections.setdefault(ln[1:-1], [])
        elif ln:
            cur.append(ln)
    return sections


def child_lines(env_assign):
    k, v = env_assign.split("=", 1)
    out = subprocess.run([sys.executable, "-m", "tests.test_gemm_plan_cpu", "--lines"], cwd=ROOT, env=dict(os.environ, **{k: v}),
                         capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def test_every_launch_of_the_table_gets_the_parents_plan():
    gold = read_golden()["default"]
    got = lines()
    assert len(got) == len(gold) == len(TABLE) and len(TABLE) > 250
    for i, (g, w) in enumerate(zip(got, gold)):
        assert g == w, f"row {i}: {TABLE[i]}"
    refused = [g for g in got if " refused: " in g]
    assert len(refused) >= 20 and all("gemm_launch: " in g for g in refused)


def test_partial_floats_is_the_plans_split():
    lib = _lib.raw()
    for row in TABLE[:UNFORCED]:
        if row.get("nbatch", 0) > 1 or row.get("phase2x"):
            continue
        rc, info, d = plan(row)
        if rc == 0 and not row.get("w_img_stride"):
            assert lib.dfh_gemm_partial_floats(C.byref(d)) == (info.split * row["M"] * row["N"] if info.split > 1 else 0), row


def test_statistics_are_promised_exactly_where_the_kernel_writes_them():
    asked_g = asked_r = 0
    for row in TABLE:
        rc, info, _ = plan(row)
        if rc:
            continue
        eight = info.kernel == 0 and info.tile == 5
        if "gstat_cpg" in row:
            asked_g += 1
            hw, cpg, M, N = row["gstat_hw"], row["gstat_cpg"], row["M"], row["N"]
            rows = 256 if (info.kernel == 1 or (info.kernel == 3 and info.wide == 1)) else 128 if eight else 0
            gbn = 320 if info.kernel == 1 else 160
            can = (rows and info.split == 1 and M % rows == 0 and hw % rows == 0 and hw // rows <= 64 and gbn % cpg == 0 and N % gbn == 0 and
                   not row.get("out_mode") and not row.get("n_split") and row.get("nbatch", 0) <= 1 and not row.get("phase2x"))
            assert info.gstat_rows == (rows if can else 0), row
        else:
            assert info.gstat_rows == 0
        if row.get("want_rowstat"):
            asked_r += 1
            bn = 320 if info.kernel == 1 else {1: 160, 4: 128, 5: 128}.get(info.wide, 0) if info.kernel == 3 else info.bn
            can = info.split == 1 and not row.get("out_mode") and row.get("act") != 4 and row["N"] % 8 == 0 and bn and row["N"] % bn == 0
            assert info.rowstat_bn == (bn if can else 0), row
        else:
            assert info.rowstat_bn == 0
    assert asked_g > 60 and asked_r > 15


@pytest.mark.parametrize("knob", KNOBS)
def test_switch_reproduces_the_parents_lines(knob):
    gold = read_golden()
    changed = dict((int(ln.split(": ", 1)[0]), ln.split(": ", 1)[1]) for ln in gold[knob])
    assert changed, "the switch must change some row of the table"
    got = child_lines(knob)
    assert len(got) == len(TABLE)
    for i, g in enumerate(got):
        assert g == changed.get(i, gold["default"][i]), f"{knob} row {i}: {TABLE[i]}"


if __name__ == "__main__":
    if sys.argv[1:] == ["--lines"]:
        print("\n".join(lines()))
    elif sys.argv[1:] == ["--record"]:
        base = lines()
        with open(GOLDEN, "w") as f:
            f.write("[default]\n" + "\n".join(base) + "\n")
            for knob in KNOBS:
                f.write(f"[{knob}]\n" + "".join(f"{i}: {g}\n" for i, (g, b) in enumerate(zip(child_lines(knob), base)) if g != b))
