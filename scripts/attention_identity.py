#!/usr/bin/env python3
"""Output identity of the 32x32x16 attention kernels (attention_x32.hip) between two builds of the library (GPU only).

One process, one library (DFH_LIB / DFH_STORAGE choose it): a fixed list of seeded cases goes through dfh_attention /
dfh_attention_lse / dfh_attention_fp8out, and one line per case carries the SHA-256 of O (and of the LSE where there is one).
Run it with each build and compare the two outputs line for line:

  DFH_LIB=<other build> python scripts/attention_identity.py > a.txt;  python scripts/attention_identity.py > b.txt;  cmp a.txt b.txt
  python scripts/attention_identity.py --only "gain 4"        # the cases whose name contains the text

Every case has two heads.  V^T is padded with NaN beyond Nk.  The "wide V^T" cases hand in a column slice of a wider V^T (ldvt larger
than the key range, NaN around it); AttnArgs::vt_bstride itself is not reachable through these entry points (the U-Net walk sets it).
A case the library refuses (the e4m3 output under fp16 storage) prints "refused"."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from difashion_amd import _lib

DEV, HEADS = "cuda", 2

# name, d, B, Nq, Nk, gain, planted keys [(key, query, factor)], mode ("o" | "lse" | "e4m3"), wide V^T
CASES = [
    # the streaming kernel
    ("x32 d40 256x192 three full tiles", 40, 1, 256, 192, 1.0, [], "o", False),
    ("x32 d40 B=2 300x200 ragged queries, ragged tile in buffer 1", 40, 2, 300, 200, 1.0, [], "o", False),
    ("x32 d40 256x129 third tile of one key", 40, 1, 256, 129, 1.0, [], "o", False),
    ("x32 d80 512x640 QB=1", 80, 1, 512, 640, 1.0, [], "o", False),
    ("x32 d64 1030x1100 LSUM, ragged", 64, 1, 1030, 1100, 1.0, [], "o", False),
    ("x32 d40 512x512 gain 4, two planted keys", 40, 1, 512, 512, 4.0, [(300, 7, 3.0), (450, 260, 5.0)], "o", False),
    ("x32 d40 512x512 poison re-run", 40, 1, 512, 512, 1.0, [(300, 7, 16.0)], "o", False),
    ("x32 d80 512x512 poison re-run", 80, 1, 512, 512, 1.0, [(300, 7, 16.0)], "o", False),
    ("x32 d40 512x512 with LSE", 40, 1, 512, 512, 1.0, [], "lse", False),
    ("x32 d40 256x64 with LSE (short keys, streaming kernel)", 40, 1, 256, 64, 1.0, [], "lse", False),
    ("x32 d40 1024x1024 e4m3 output", 40, 1, 1024, 1024, 1.0, [], "e4m3", False),
    ("x32 d40 B=2 256x200 wide V^T", 40, 2, 256, 200, 1.0, [], "o", True),
    # the short-key kernel
    ("xs d40 B=8 4096x77 qrep > 1, key block 1 skipped", 40, 8, 4096, 77, 1.0, [], "o", False),
    ("xs d40 B=2 512x65 gain 4, offset raised in tile 1", 40, 2, 512, 65, 4.0, [(64, 5, 3.0)], "o", False),
    ("xs d80 B=3 1024x128 two full tiles, QB=1", 80, 3, 1024, 128, 1.0, [], "o", False),
    ("xs d80 300x64 ragged queries, one tile", 80, 1, 300, 64, 1.0, [], "o", False),
    ("xs d40 1024x77 e4m3 output", 40, 1, 1024, 77, 1.0, [], "e4m3", False),
    ("xs d40 B=2 512x77 wide V^T", 40, 2, 512, 77, 1.0, [], "o", True),
]


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def run(i, name, d, B, Nq, Nk, gain, plants, mode, wide):
    dt, C_ = _lib.storage_dtype(), d * HEADS
    q, k, v = ((rnd(B, n, C_, seed=1000 + 3 * i + j) * g).to(dt).to(DEV) for j, (n, g) in enumerate(((Nq, gain), (Nk, gain), (Nk, 1.0))))
    for key, query, f in plants:
        k[:, key] = q[:, query] * f
    ld = (Nk + 7) // 8 * 8 + (24 if wide else 0)
    col0 = 8 if wide else 0
    # a slice that starts at column col0 moves the kernel's view of the last head's rows col0 elements past the tensor: keep a tail
    vt = torch.full((B * C_ * ld + 64,), float("nan"), dtype=dt, device=DEV)[:B * C_ * ld].view(B, C_, ld)
    vt[:, :, col0:col0 + Nk] = v.transpose(1, 2)
    vt_ptr = _lib.ptr(vt[:, :, col0:])
    s, scale = _lib.stream_ptr(), d ** -0.5
    if mode == "e4m3":
        o = torch.zeros((B, Nq, C_), dtype=torch.uint8, device=DEV)
        amax = v.float().abs().amax(dim=(1, 2)).contiguous()
        _lib.call("dfh_attention_fp8out", _lib.ptr(q), C_, _lib.ptr(k), C_, vt_ptr, ld, _lib.ptr(o), C_, _lib.ptr(amax),
                  B, HEADS, d, Nq, Nk, scale, s)
    elif mode == "lse":
        o = torch.zeros_like(q)
        lse = torch.zeros((B, HEADS, Nq), device=DEV)
        _lib.call("dfh_attention_lse", _lib.ptr(q), C_, _lib.ptr(k), C_, vt_ptr, ld, _lib.ptr(o), C_, B, HEADS, d, Nq, Nk, scale, _lib.ptr(lse), s)
    else:
        o = torch.zeros_like(q)
        _lib.call("dfh_attention", _lib.ptr(q), C_, _lib.ptr(k), C_, vt_ptr, ld, _lib.ptr(o), C_, B, HEADS, d, Nq, Nk, scale, s)
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(o.float()).all()) if mode != "e4m3" else True
    return f"O {sha(o)}" + (f" LSE {sha(lse)}" if mode == "lse" else "") + ("" if finite else " NOT-FINITE")


if __name__ == "__main__":
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    print(f"# storage={_lib.storage()} DFH_ATTN_VARIANT={os.environ.get('DFH_ATTN_VARIANT', '0')}", flush=True)
    for i, case in enumerate(CASES):
        if only not in case[0]:
            continue
        _lib.census_reset()
        try:
            line = run(i, *case)
        except _lib.DfhError as e:
            if "refused" not in str(e):      # anything else (a failed launch) is an error, not a refusal
                raise
            line = "refused"
        print(f"{case[0]:62s} x32={_lib.census()['attention_x32']} {line}", flush=True)
