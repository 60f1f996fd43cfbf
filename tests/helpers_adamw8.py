"""numpy / fp64 restatement of the block-wise 8-bit optimizer state and of one AdamW step on it, written from the format's
specification (DESIGN.md "8-bit optimizer states") and from Dettmers et al., "8-bit Optimizers via Block-wise Quantization" -- not
from the library's code.  tests/test_adamw8_cpu.py and tests/test_gpu_adamw8.py compare the library against it.

A block is 64 consecutive elements; it has one fp32 absmax per moment and each element one uint8 code per moment into a table of 256
ascending fp32 entries; x = table[code] * absmax (one fp32 multiply)."""
import numpy as np

BLOCK = 64
# the largest distance from a point of [-1, 1] / [0, 1] to the nearest entry of the signed / unsigned table
MAX_GAP = {True: 7.0313e-3, False: 3.5157e-3}
U = 2.0 ** -24          # fp32 unit roundoff


def table(signed: bool) -> np.ndarray:
    """Signed: {0, +1} and +-10^(i-6) (0.1 + 0.9 (2j+1) / 2^(i+1)), i = 0..6, j = 0..2^i - 1 (no -1; 0 is index 127).
    Unsigned: {0, 1} and 10^(i-6) (0.1 + 0.9 (2j+1) / 2^(i+2)), i = 0..6, j = 0..2^(i+1) - 1 (0 is index 0).
    Evaluated in double, rounded once to fp32, ascending."""
    vals = [0.0, 1.0]
    for i in range(7):
        slots = 2 ** i if signed else 2 ** (i + 1)
        for j in range(slots):
            x = 10.0 ** (i - 6) * (0.1 + 0.9 * (2 * j + 1) / (2.0 * slots))
            vals += [x, -x] if signed else [x]
    return np.sort(np.asarray(vals, dtype=np.float64)).astype(np.float32)


def zero_code(signed: bool) -> int:
    return 127 if signed else 0


def block_absmax(x) -> np.ndarray:
    """max |x| per block, exactly, in the dtype of x; a NaN in a block makes its absmax NaN (np.max propagates it)."""
    return np.abs(np.asarray(x)).reshape(-1, BLOCK).max(axis=1)


def nearest_gap(x, absmax, signed: bool):
    """(k, e): for every element the index of an entry whose dequantised value is nearest to x, and that distance
    e = min_k |x - table[k] * absmax|, both in fp64.  table[k] * absmax ascends in k, so the two entries around x decide."""
    t = table(signed).astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    am = np.repeat(np.asarray(absmax, dtype=np.float64), BLOCK)
    safe = np.where(am > 0, am, 1.0)
    pos = np.clip(np.searchsorted(t, x / safe), 1, 255)
    best_k, best_e = None, None
    for k in (pos - 2, pos - 1, pos, pos + 1):         # one entry of margin on each side for the rounding of x / absmax
        k = np.clip(k, 0, 255)
        e = np.abs(x - t[k] * am)
        if best_e is None:
            best_k, best_e = k, e
        else:
            take = e < best_e
            best_k, best_e = np.where(take, k, best_k), np.where(take, e, best_e)
    return best_k, best_e


def code_gap(x, codes, absmax, signed: bool) -> np.ndarray:
    """e(code) = |x - table[code] * absmax| in fp64 for the given codes."""
    t = table(signed).astype(np.float64)
    am = np.repeat(np.asarray(absmax, dtype=np.float64), BLOCK)
    return np.abs(np.asarray(x, dtype=np.float64) - t[np.asarray(codes).astype(np.int64)] * am)


def floor_applies(x, absmax, signed: bool) -> np.ndarray:
    """Elements of a second moment to which the floor rule applies: v > 0 whose nearest entry would be 0 (index 0)."""
    if signed:
        return np.zeros(np.asarray(x).shape, dtype=bool)
    k, _ = nearest_gap(x, absmax, signed)
    return (np.asarray(x, dtype=np.float64) > 0) & (k == 0)


def quantize(x, signed: bool):
    """-> (codes uint8, absmax float32).  Exact nearest entry in fp64; an all-zero block has absmax 0 and zero codes (no 0 / 0); a
    second moment v > 0 never takes code 0, it takes code 1."""
    x = np.asarray(x, dtype=np.float64)
    am = block_absmax(x)
    k, _ = nearest_gap(x, am, signed)
    if not signed:
        k = np.where((x > 0) & (k == 0), 1, k)
    k = np.where(np.repeat(am, BLOCK) == 0, zero_code(signed), k)
    return k.astype(np.uint8), am.astype(np.float32)


def dequantize(codes, absmax, signed: bool) -> np.ndarray:
    """table[code] * absmax: one fp32 multiply."""
    with np.errstate(invalid="ignore", over="ignore"):
        return table(signed)[np.asarray(codes).astype(np.int64)] * np.repeat(np.asarray(absmax, dtype=np.float32), BLOCK)


def clip_coef_f32(sumsq, max_norm) -> float:
    """min(1, max_norm / (sqrt(sumsq) + 1e-6)) in fp32 operations, as the update kernel derives this one scalar from *sumsq."""
    nrm = np.sqrt(np.float32(sumsq))
    return float(np.minimum(np.float32(1.0), np.float32(max_norm) / (nrm + np.float32(1e-6))))


def adamw_moments(g, m, v, *, beta1, beta2, clip=1.0):
    g = np.asarray(g, dtype=np.float64) * clip
    return g, beta1 * np.asarray(m, dtype=np.float64) + (1.0 - beta1) * g, beta2 * np.asarray(v, dtype=np.float64) + (1.0 - beta2) * g * g


def adamw_step(p, g, m, v, *, lr, beta1, beta2, eps, wd, step, clip=1.0, shadow=None, ema_decay=0.0):
    """One torch.optim.AdamW step in fp64 (decoupled weight decay, bias corrections, eps outside the corrected root), the gradient
    pre-scaled by ``clip``; with ``shadow``, diffusers' EMA folded in: shadow -= (1 - decay) (shadow - p_new).
    -> (p, m, v, shadow)."""
    _, m, v = adamw_moments(g, m, v, beta1=beta1, beta2=beta2, clip=clip)
    p = np.asarray(p, dtype=np.float64) * (1.0 - lr * wd)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    with np.errstate(invalid="ignore", divide="ignore"):
        p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    if shadow is not None:
        shadow = np.asarray(shadow, dtype=np.float64)
        shadow = shadow - (1.0 - ema_decay) * (shadow - p)
    return p, m, v, shadow


def adamw8_step(p, g, codes1, absmax1, codes2, absmax2, **kw):
    """One step on 8-bit states: dequantise, ``adamw_step``, quantise the new moments.  The parameter moves by the UNQUANTISED new
    moments.  -> (p, codes1, absmax1, codes2, absmax2, shadow)."""
    m = dequantize(codes1, absmax1, True).astype(np.float64)
    v = dequantize(codes2, absmax2, False).astype(np.float64)
    p, m, v, shadow = adamw_step(p, g, m, v, **kw)
    c1, a1 = quantize(m, True)
    c2, a2 = quantize(v, False)
    return p, c1, a1, c2, a2, shadow


def hard_blocks(n: int, seed: int, signed: bool) -> np.ndarray:
    """fp32 quantiser inputs of n elements (n % 64 == 0) whose first blocks, repeated cyclically, are: zeros; a block whose largest
    magnitude is negative (signed) and which holds exact +-absmax; values spread over 9 decades; subnormals; plain normal values."""
    rng = np.random.default_rng(seed)
    nb = n // BLOCK
    x = rng.standard_normal((nb, BLOCK))
    kinds = (np.arange(nb) + (1 if nb == 1 else 0)) % 5       # a lone block is the negative-largest one
    for b in range(min(nb, 10)):
        kind = kinds[b]
        if kind == 0 and b == 0:
            x[b] = 0.0
        elif kind == 1 or (kind == 0 and b > 0):
            x[b] = rng.uniform(-0.9, 0.9, BLOCK) * 3.0
            x[b, 5], x[b, 40], x[b, 41] = -3.0, 3.0 if b > 1 else -3.0, -3.0       # exact +-absmax; in block 1 the largest is negative only
            x[b, 7] = 2.999
        elif kind == 2:
            x[b] = rng.standard_normal(BLOCK) * 10.0 ** rng.uniform(-9, 0, BLOCK)
            x[b, 0] = 1.0
        elif kind == 3:
            x[b] = rng.standard_normal(BLOCK) * 2.0 ** -140
            x[b, 3] = 2.0 ** -149
    if nb > 10:      # the bulk: per-block scales over a few decades, a share of exact zeros
        x[10:] *= 10.0 ** rng.uniform(-4, 2, (nb - 10, 1))
        x[10:][rng.random((nb - 10, BLOCK)) < 0.02] = 0.0
    if not signed:
        x = np.abs(x)
    return x.astype(np.float32).reshape(-1)


def drift_gradients(n: int, steps: int, seed: int):
    """The open-loop gradient sequence of the drift test: g_t = (mu + xi_t) * s, mu ~ 0.3 N(0,1), xi_t ~ N(0,1),
    s = exp(0.5 N(0,1)) per element times exp(3 N(0,1)) per block.  -> (p0 [n], g [steps][n]) as fp32."""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n)
    mu = 0.3 * rng.standard_normal(n)
    s = np.exp(0.5 * rng.standard_normal(n)) * np.repeat(np.exp(3.0 * rng.standard_normal(n // BLOCK)), BLOCK)
    g = (mu[None, :] + rng.standard_normal((steps, n))) * s[None, :]
    return p0.astype(np.float32), g.astype(np.float32)


def drift(p, p_true, p0) -> float:
    p, p_true, p0 = (np.asarray(a, dtype=np.float64) for a in (p, p_true, p0))
    return float(np.linalg.norm(p - p_true) / np.linalg.norm(p_true - p0))
