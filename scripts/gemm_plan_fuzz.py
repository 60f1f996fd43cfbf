#!/usr/bin/env python3
"""Random launches through dfh_gemm_plan, one text line each (host code, no GPU): run it against two builds of the library and diff.

    python scripts/gemm_plan_fuzz.py 30000 > a.txt;  DFH_LIB=<other build>/libdifashion_hip.so DFH_LIB_ALLOW_ABI_MISMATCH=1 python scripts/gemm_plan_fuzz.py 30000 > b.txt

The other build needs a dfh_gemm_plan of its own (for the commit before the plan / dispatch split: profiles/gemm_plan/parent_dump.patch)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import random

from tests.test_gemm_plan_cpu import lin, conv, plan, PTR
random.seed(7)
Ms = [16, 77, 128, 200, 256, 300, 1024, 1232, 4096, 9216, 16384, 57344, 65536]
Cs = [8, 64, 72, 128, 160, 192, 256, 320, 512, 640, 960, 1280, 1920, 2560, 5120]
Ns = [8, 64, 128, 160, 200, 256, 320, 328, 512, 640, 960, 1280, 2560, 5120, 10240]
ids = [0]*6 + [1,2,3,4,5,6,7,8,9,10,11,12,15,19,20,21,22,23,24,30,-1]
for i in range(int(sys.argv[1])):
    kw = {}
    if random.random() < .3: kw.update(resid=PTR, ld_res=random.choice([0, 4]) + 0)
    if random.random() < .2: kw.update(rowvec=PTR, rv_ld=4096)
    if random.random() < .3: kw.update(act=random.choice([1, 2, 3, 4, 4]))
    if random.random() < .2: kw.update(out_mode=random.choice([1, 2, 3]))
    if random.random() < .3: kw.update(gstat_cpg=random.choice([4, 10, 20, 40, 16]), gstat_hw=random.choice([64, 128, 256, 1024, 4096, 9216]))
    if random.random() < .2: kw.update(want_rowstat=1)
    if random.random() < .15: kw.update(ln_cnt=random.choice([64, 128, 160, 320]))
    if random.random() < .1: kw.update(n_split=random.choice([128, 160, 320, 640]))
    if random.random() < .1: kw.update(pre_out=1)
    if random.random() < .15: kw.update(nbatch=random.choice([1, 4, 16]), w_blocked=random.choice([0, 1]))
    if random.random() < .1: kw.update(w_img_stride=64, rows_per_b=random.choice([128, 256, 100, 4096]))
    kw.update(force_tile=random.choice(ids), force_split=random.choice([0]*5 + [1, 2, 5, 100]), force_order=random.choice([-1]*4 + [2, 3]))
    if random.random() < .4:
        B, H = random.choice([(1, 8), (1, 16), (2, 32), (16, 8), (16, 16), (16, 32), (4, 64), (14, 64), (1, 96)])
        r = conv(B, H, random.choice(Cs), random.choice(Ns), K0=random.choice([0, 0, 320, 100]), stride=random.choice([1, 1, 2]), **kw)
        if random.random() < .2: r = dict(r, phase2x=1)
    else:
        r = lin(random.choice(Ms), random.choice(Cs), random.choice(Ns), K1=random.choice([0, 0, 0, 320, 64]), **kw)
    if "ld_res" in r: r["ld_res"] += r["N"]
    print(plan(r)[1].line.decode())
