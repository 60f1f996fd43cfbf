"""Shared by tests/test_jpeg_cpu.py, tests/test_gpu_jpeg.py, tests/jpeg_fp16_child.py and tests/golden/make_golden_jpeg.py: the numpy
restatement of the JPEG save / open round trip, the seeded case images and the case list.

``roundtrip`` is written from the arithmetic contract of the row -- libjpeg's "islow" path, which PIL takes in both directions -- and
not from the kernel: integer numpy throughout, ``>>`` arithmetic.  ``dtype=np.int32`` runs the same expressions in wrapping 32-bit
integers, which is what licenses int32 in the kernel.  It returns the pixels and the quantised coefficients in the kernel's layout."""
import functools
import hashlib
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_roundtrip.npz")

SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (31, 33), (30, 46), (64, 64), (100, 75), (512, 512)]
KINDS = ("noise", "smooth", "white", "checker")
SETTINGS = [(75, "4:2:0"), (75, "4:4:4"), (95, "4:2:0"), (30, "4:2:0"), (90, "4:4:4"), (1, "4:2:0"), (100, "4:4:4")]
EXTRA_SIZES = [(9, 12)]                                    # beside the row's list: an odd height at a width the four-pixel kernel takes
GOLDEN_SIZES = SIZES[:-1]                                 # up to 100 x 75: the fixture stays small
GOLDEN_FEW_KINDS = {(64, 64): ("smooth", "checker"), (100, 75): ("smooth", "checker")}

LUMA_BASE = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                      72, 92, 95, 98, 112, 100, 103, 99]).reshape(8, 8)
CHROMA_BASE = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32).reshape(8, 8)
# the twelve 13-bit constants of the butterfly
C298, C390, C541, C765, C899, C1175, C1501, C1847, C1961, C2053, C2562, C3072 = (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819,
                                                                                 20995, 25172)


def setting_id(setting) -> str:
    return f"q{setting[0]}_{setting[1].replace(':', '')}"


def case_image(kind: str, h: int, w: int) -> np.ndarray:
    """The seeded uint8 [h, w, 3] image of a case: integers only, so every platform regenerates the same bytes."""
    rng = np.random.default_rng([KINDS.index(kind), h, w])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "checker":                                   # one-pixel 0 / 255: the wrap of the range limit, the widest coefficients
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    tri = lambda v: np.abs(v % 510 - 255)                   # smooth + noise: triangle waves of different slopes per channel
    base = np.stack([tri(3 * x + 2 * (c + 1) * y + 60 * c) for c in range(3)], -1)
    return np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def checksum(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def quant_tables(quality: int):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA_BASE, CHROMA_BASE))


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_1d(d, first: bool):
    """Along the last axis.  first: the row pass (2 extra bits, descale by 11); else the column pass (2 for outputs 0 and 4, else 15)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
    z1 = (t12 + t13) * C541
    o[2], o[6] = descale(z1 + t13 * C765, n), descale(z1 - t12 * C1847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C1175
    t4, t5, t6, t7 = t4 * C298, t5 * C2053, t6 * C3072, t7 * C1501
    z1, z2, z3, z4 = -z1 * C899, -z2 * C2562, -z3 * C1961 + z5, -z4 * C390 + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def idct_1d(x, n: int):
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., i] for i in range(8))
    z1 = (i2 + i6) * C541
    t2, t3 = z1 - i6 * C1847, z1 + i2 * C765
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * C1175
    t0, t1, t2, t3 = t0 * C298, t1 * C2053, t2 * C3072, t3 * C1501
    z1, z2, z3, z4 = -z1 * C899, -z2 * C2562, -z3 * C1961 + z5, -z4 * C390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([descale(v, n) for v in (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)], -1)


def range_limit(v):
    """libjpeg's table as a function of v & 1023: a wrap, not a clamp."""
    i = v & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))


def to_blocks(p):
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def from_blocks(b):
    return b.transpose(0, 2, 1, 3).reshape(b.shape[0] * 8, b.shape[1] * 8)


def component_roundtrip(plane, q):
    """plane: padded to whole blocks.  -> (the decoded plane, the quantised coefficients [block rows, block cols, 8, 8])."""
    dt = plane.dtype.type
    q = q.astype(plane.dtype)
    c = fdct_1d(to_blocks(plane - dt(128)), True)                          # rows
    c = fdct_1d(c.swapaxes(-1, -2), False).swapaxes(-1, -2)                # columns; the output is scaled by 8
    q8 = q * dt(8)
    m = (np.abs(c) + (q8 >> 1)) // q8
    k = np.where(c < 0, -m, m)
    w = idct_1d((k * q).swapaxes(-1, -2), 11).swapaxes(-1, -2)             # columns first
    return from_blocks(range_limit(idct_1d(w, 18))), k


def edge_pad(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def roundtrip(rgb: np.ndarray, quality: int = 75, subsampling: str = "4:2:0", dtype=np.int64):
    """-> (uint8 [H, W, 3], int16 [blocks, 64]): the pixels after save / open, and the coefficients of the real blocks: Y row-major, Cb, Cr."""
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and subsampling in ("4:2:0", "4:4:4")
    H, W, _ = rgb.shape
    R, G, B = (rgb[..., i].astype(dtype) for i in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    ql, qc = quant_tables(quality)
    sub = subsampling == "4:2:0"
    m = 16 if sub else 8
    Hp, Wp = -(-H // m) * m, -(-W // m) * m
    Yd, Yk = component_roundtrip(edge_pad(Y, Hp, Wp), ql)
    ch, cw = ((H + 1) // 2, (W + 1) // 2) if sub else (H, W)
    if sub:
        def down(p):
            p = edge_pad(p, H + (H & 1), Wp)                              # columns to the MCU, rows to an even count only
            bias = np.tile(np.array([1, 2], dtype), Wp // 4)[None, :]
            d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
            return edge_pad(d, Hp // 2, Wp // 2)                           # the DOWNSAMPLED last row goes down to the block multiple

        def up(d):
            d = d[:ch, :cw]
            e = np.pad(d, ((1, 1), (0, 0)), mode="edge")
            rows = np.empty((2 * ch, cw), dtype)
            rows[0::2], rows[1::2] = 3 * e[1:-1] + e[:-2], 3 * e[1:-1] + e[2:]
            f = np.pad(rows, ((0, 0), (1, 1)), mode="edge")
            o = np.empty((2 * ch, 2 * cw), dtype)
            o[:, 0::2], o[:, 1::2] = (3 * f[:, 1:-1] + f[:, :-2] + 8) >> 4, (3 * f[:, 1:-1] + f[:, 2:] + 7) >> 4
            return o[:H, :W]
        (Cbd, Cbk), (Crd, Crk) = component_roundtrip(down(Cb), qc), component_roundtrip(down(Cr), qc)
        Cbd, Crd = up(Cbd), up(Crd)
    else:
        (Cbd, Cbk), (Crd, Crk) = component_roundtrip(edge_pad(Cb, Hp, Wp), qc), component_roundtrip(edge_pad(Cr, Hp, Wp), qc)
        Cbd, Crd = Cbd[:H, :W], Crd[:H, :W]
    Yd = Yd[:H, :W]
    cb, cr = Cbd - 128, Crd - 128
    r = Yd + ((91881 * cr + 32768) >> 16)
    g = Yd + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = Yd + ((116130 * cb + 32768) >> 16)
    pixels = np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
    real = lambda k, rows, cols: k[:-(-rows // 8), :-(-cols // 8)].reshape(-1, 64)
    coef = np.concatenate([real(Yk, H, W), real(Cbk, ch, cw), real(Crk, ch, cw)]).astype(np.int16)
    return pixels, coef


@functools.lru_cache(maxsize=None)
def expected(kind: str, h: int, w: int, quality: int, subsampling: str):
    """The restatement of one case, computed once a process and shared: do not write into it."""
    px, coef = roundtrip(case_image(kind, h, w), quality, subsampling)
    px.setflags(write=False)
    coef.setflags(write=False)
    return px, coef


def pil_roundtrip(a: np.ndarray, quality: int = 75, subsampling: str = "4:2:0") -> np.ndarray:
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", quality=quality, subsampling=subsampling)
    f.seek(0)
    return np.array(Image.open(f).convert("RGB"))


def pil_quant_tables(quality: int):
    """What a file saved at ``quality`` carries: ``Image.open(f).quantization``, which Pillow (since 8.3) hands out in natural order."""
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(f, "JPEG", quality=quality)
    f.seek(0)
    q = Image.open(f).quantization
    return [np.array(list(q[i]), np.int32).reshape(8, 8) for i in (0, 1)]


def golden_cases():
    for h, w in GOLDEN_SIZES:
        for kind in GOLDEN_FEW_KINDS.get((h, w), KINDS):
            for quality, subsampling in SETTINGS:
                yield kind, h, w, quality, subsampling


def golden_key(kind, h, w, quality, subsampling) -> str:
    return f"{kind}_{h}x{w}_{setting_id((quality, subsampling))}"
