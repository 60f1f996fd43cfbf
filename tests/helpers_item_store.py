"""Shared by tests/test_item_store_cpu.py, tests/test_gpu_item_store.py and tests/item_store_fp16_child.py: seeded inputs of the two
item-store kernels, a pure-torch emulation of their contracts -- the operations of include/difashion_hip.h, one
rounding each, in the stated order -- the fp64 reference with its derived bound, the exact-data condition, and a stand-in VAE with a
real posterior.  The CPU test holds the emulation to fp64, so the GPU tests compare against something that was itself checked."""
import types

import torch

import difashion_amd as da

ROW_ELEMS = (16, 256, 16384)                 # 4 x 2 x 2 (a quarter-filled wave), one full slab, the real 4 x 64 x 64 row
ROWS = (1, 5, 33)
SEG_LENS = (1, 2, 3, 4, 5, 67, 0)            # every remainder of the 4-wide unroll, a long list, an empty segment (index 6)
ITEMS = 40
SCALE = 0.18215
U = 2.0 ** -24


def f32(x: float) -> float:
    """The fp32 value a C float argument carries."""
    return float(torch.tensor(x, dtype=torch.float32))


def make_table(items, row_elems, seed, exact=False, with_std=True):
    """[items][2 * row_elems] (or [items][row_elems]) fp32: means ~ N(0, 1), std in (0.05, 1.05).  exact: integer means in [-8, 8]."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randint(-8, 9, (items, row_elems), generator=g).float() if exact else torch.randn(items, row_elems, generator=g)
    if not with_std:
        return mean.contiguous()
    return torch.cat([mean, torch.rand(items, row_elems, generator=g) + 0.05], dim=1).contiguous()


def make_segments(items, seed):
    """One id list per entry of SEG_LENS: id 0, id items - 1 and repeated ids are all present."""
    g = torch.Generator().manual_seed(seed)
    segs = [torch.randint(0, items, (n,), generator=g).tolist() for n in SEG_LENS]
    segs[0] = [items - 1]
    segs[1] = [0, 0]                                          # a repeated id, and id 0
    segs[4] = [items - 1, 3, 3, 0, items - 1]
    segs[5][:3] = [0, items - 1, segs[5][3]]
    return segs


def row_segments(rows):
    """Null rows first, last and alone; an empty segment; every segment length."""
    if rows == 1:
        return [5]
    seq = [-1] + [(i * 3) % len(SEG_LENS) for i in range(rows - 2)] + [-1]
    if rows >= 5:
        seq[3] = 6                                            # the empty segment
    return seq


def csr(segs):
    items, offsets = [], [0]
    for s in segs:
        items += list(s)
        offsets.append(len(items))
    return items, offsets


def gather_ids(rows, items, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, items, (rows,), generator=g)
    ids[0] = items - 1
    if rows >= 5:
        ids[1], ids[2], ids[3] = 0, 7, 7                      # id 0, a repeated id
    return ids


# ---------------------------------------------------------------------- the emulation: torch CPU ops, one rounding each
def emulate_gather(table, row_elems, iids, eps, scale):
    """(table[iid][:E] + table[iid][E:2E] * eps) * scale, or table[iid][:E] * scale; a bad id gives a row of NaN."""
    iids = torch.as_tensor(iids, dtype=torch.int64)
    ok = (iids >= 0) & (iids < table.shape[0])
    safe = torch.where(ok, iids, torch.zeros_like(iids))
    v = table[safe, :row_elems]
    if eps is not None:
        v = v + table[safe, row_elems:2 * row_elems] * eps.reshape(len(iids), row_elems)
    v = v * torch.tensor(scale, dtype=torch.float32)
    v[~ok] = float("nan")
    return v


def emulate_history(table, row_elems, segs, row_seg, null_row, scale):
    """Per row: acc = 0; acc = acc + table[item] * scale in list order; acc / float(count).  -1 or an empty segment: null_row."""
    s = torch.tensor(scale, dtype=torch.float32)
    out = torch.empty(len(row_seg), row_elems)
    for r, seg in enumerate(row_seg):
        ids = segs[seg] if seg >= 0 else []
        if not ids:
            out[r] = null_row.reshape(-1)
            continue
        acc = torch.zeros(row_elems)
        for i in ids:
            acc = acc + table[i, :row_elems] * s
        out[r] = acc / torch.tensor(float(len(ids)), dtype=torch.float32)
    return out


def history_ref64(table, row_elems, segs, row_seg, null_row, scale):
    """fp64 mean of scale * x_k (scale = the fp32 value the kernel is handed), and the bound of the issue per element:
    (L + 1) * 2^-24 * mean_k |scale * x_k| -- L - 1 roundings of the running sum and one of each product, each below 2^-24 of the sum
    of magnitudes, divided by L; plus the division's own rounding."""
    s = f32(scale)
    ref = torch.empty(len(row_seg), row_elems, dtype=torch.float64)
    bound = torch.zeros(len(row_seg), row_elems, dtype=torch.float64)
    for r, seg in enumerate(row_seg):
        ids = segs[seg] if seg >= 0 else []
        if not ids:
            ref[r] = null_row.reshape(-1).double()
            continue
        t = table[ids, :row_elems].double() * s
        ref[r] = t.mean(dim=0)
        bound[r] = (len(ids) + 1) * U * t.abs().mean(dim=0)
    return ref, bound


def exact_condition(table, row_elems, segs, scale):
    """True when every product and every partial sum of every segment is an integer below 2^24 in magnitude: integer means, scale 1.
    Then any order of summation is exact, and the kernel must equal torch.mean of the gathered rows bit for bit."""
    m = table[:, :row_elems]
    if f32(scale) != 1.0 or not bool((m == m.round()).all()):
        return False
    worst = max((len(s) for s in segs), default=0) * float(m.abs().max())
    return worst < 2.0 ** 24


def torch_mean_history(table, row_elems, segs, row_seg, null_row):
    return torch.stack([table[segs[s], :row_elems].mean(dim=0) if s >= 0 and segs[s] else null_row.reshape(-1) for s in row_seg])


# ---------------------------------------------------------------------- raw-pointer drivers over the C ABI (device tensors)
def run_gather(table, row_elems, iids, eps, scale, out=None):
    from difashion_amd import _lib
    rows = iids.numel()
    out = torch.empty(rows, row_elems, dtype=torch.float32, device=table.device) if out is None else out
    _lib.call("dfh_item_gather", _lib.ptr(table), table.shape[0], table.shape[1], row_elems, _lib.ptr(iids), rows, _lib.ptr(eps), scale,
              _lib.ptr(out), _lib.stream_ptr())
    return out


def run_history(table, row_elems, seg_items, seg_offsets, row_seg, null_row, scale):
    from difashion_amd import _lib
    rows = row_seg.numel()
    out = torch.empty(rows, row_elems, dtype=torch.float32, device=table.device)
    _lib.call("dfh_history_rows", _lib.ptr(table), table.shape[0], table.shape[1], row_elems, _lib.ptr(seg_items), _lib.ptr(seg_offsets),
              _lib.ptr(row_seg), rows, _lib.ptr(null_row), scale, _lib.ptr(out), _lib.stream_ptr())
    return out


def history_device_inputs(segs, row_seg, device):
    items, offsets = csr(segs)
    return (torch.tensor(items, dtype=torch.int64, device=device), torch.tensor(offsets, dtype=torch.int64, device=device),
            torch.tensor(row_seg, dtype=torch.int32, device=device))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------- a stand-in VAE with a real posterior
class Cfg(dict):
    __getattr__ = dict.__getitem__


class PosteriorVAE:
    """"Images" are latent-shaped: mean = the image, logvar = a fixed non-constant tensor; the distribution is the package's own
    DiagonalGaussianDistribution, so std and sample() are the torch expressions of the real path."""

    def __init__(self, size, device, scaling_factor=SCALE):
        self.config = Cfg(scaling_factor=scaling_factor, latent_channels=4, block_out_channels=(1, 1, 1, 1))
        g = torch.Generator().manual_seed(91)
        self.logvar = (torch.randn(1, 4, size, size, generator=g) * 0.7 - 1.0).to(device)

    def encode(self, x):
        params = torch.cat([x, self.logvar.expand(x.shape[0], -1, -1, -1)], dim=1)
        return types.SimpleNamespace(latent_dist=da.vae.DiagonalGaussianDistribution(params))

    def decode(self, z, return_dict=False):
        return (z,)
