"""Seeded inputs of the grounding-retrieval row (csrc/eval_rank.hip, ``rank_candidates``), shared by
tests/golden/make_golden_grounding.py, tests/test_grounding_cpu.py and tests/test_gpu_grounding.py.  Everything is regenerated from the
seeds on every box (CPU generator, elementwise arithmetic only: the same tensors everywhere); the fixtures ``tests/golden/grounding_*.npz``
hold what the REFERENCE's ``clip_og_retrieval_given_data`` made of them in fp64, and a checksum of the inputs.

So that ranks are exact in any correct fp32 arithmetic every row gets a PLANTED LADDER: the first min(len, 112) candidates of its list are
rebuilt as ``(a_j u + sqrt(1 - a_j^2) z_j) * length`` with ``u`` the row's direction, ``z_j`` orthogonal to it and ``a_j = 0.9 - 0.005 j``,
then the list is shuffled.  ``u`` is a sign pattern on the dimensions of index 0, 2 or 3 mod 4 (split between the two directions where two share a set) and
``z_j`` one on the dimensions 1 mod 4, so the orthogonality and the norms are exact without a reduction.  Consecutive similarities through
rank 101 stand 5e-3 apart and the rest of the list -- plain ``randn`` rows, other sets' ladders among them -- stays below 0.15, under the
ladder's foot at 0.345.  Ladders of different sets use disjoint id blocks, so none rewrites another's."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOPN = (10, 20, 50, 100)
LADDER, LADDER_TOP, LADDER_STEP = 112, 0.9, 0.005
CROWD_MAX = 0.15
# the rank at which a row's ground truth is planted, cycled over the rows: both sides of every cutoff, inside the list but past the top
# 100, and -1 = not in the list at all
GRD_RANKS = (0, 9, 10, 19, 20, 49, 50, 99, 100, 111, -1)

# name -> dim, table rows, seed, the lengths of the sets ranked by one row each, (length, rows) of the set shared by many rows.
# main: the 64-candidate tile edge (64, 65), the top-N edge (100, 101), more than one selection batch (1000, 2500), and a shared set of a
# full 64-row tile plus a partial one whose rows alternate between two directions; narrow: K a multiple of 4 and not of 32.
CASES = {
    "main": dict(dim=1024, table_rows=3000, seed=71, lens=(1, 7, 64, 65, 100, 101, 130, 1000, 2500), shared=(300, 70)),
    "narrow": dict(dim=20, table_rows=512, seed=72, lens=(7, 65, 100, 112), shared=None),
    "clip_l": dict(dim=768, table_rows=1500, seed=73, lens=(65, 130, 1000), shared=None),
}
SHARED_JITTER = 0.02


def load_fixture(name: str):
    return dict(np.load(fixture_path(name)))


def fixture_path(name: str) -> str:
    return os.path.join(GOLDEN, f"grounding_{name}.npz")


def rank_bound(dim: int) -> float:
    """Absolute error of one similarity of embed_rank_gemm_kernel at fp32, in units of 2^-24 on a value of at most 1.  The dot product:
    every 32-wide k-tile is two chains of 16 fused multiply-adds (16 roundings, each relative to no more than the tile's sum of
    |products|), one add of the two and the compensated add over k-tiles (2, independent of K): 19 units of sum |g_k t_k| <= |g| |t|.
    The two norms (embed_row_norms_kernel): per lane a run of dim / 64 fused multiply-adds and a 6-step wave tree, halved by the square
    root, plus its rounding: dim / 64 + 8 for the pair; their product, the divide and the fixture's own rounding to fp32: 3 more.
    (dim / 64 + 30) 2^-24: 2.7e-6 at dim 1024, three orders below the 5e-3 ladder step."""
    return (dim / 64 + 30) * 2.0 ** -24


def _signs(n, g):
    return (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()


def _direction(dim, residues, g):
    """A unit vector: random signs on the dimensions whose index mod 4 is in ``residues``."""
    idx = torch.tensor([k for k in range(dim) if k % 4 in residues])
    u = torch.zeros(dim, dtype=torch.float64)
    u[idx] = _signs(len(idx), g) / math.sqrt(len(idx))
    return u


def _ladder(u, n, g):
    """[n, dim] fp64: rung j = (a_j u + sqrt(1 - a_j^2) z_j) * length_j, z_j a unit sign pattern on the dimensions 1 mod 4."""
    dim = u.numel()
    zdims = torch.arange(1, dim, 4)
    out = torch.zeros((n, dim), dtype=torch.float64)
    for j in range(n):
        a = LADDER_TOP - LADDER_STEP * j
        z = torch.zeros(dim, dtype=torch.float64)
        z[zdims] = _signs(len(zdims), g) / math.sqrt(len(zdims))
        out[j] = (a * u + math.sqrt(1.0 - a * a) * z) * float(0.5 + 2.0 * torch.rand((), generator=g))
    return out


def _plant_grd(rank, ladder_ids, cand, table_rows):
    if 0 <= rank < len(ladder_ids):
        return int(ladder_ids[rank])
    held = set(cand.tolist())
    return next(i for i in range(table_rows - 1, -1, -1) if i not in held)


def case_inputs(name):
    """-> dict(gen [rows, dim], table [table_rows, dim], candidates: one int64 tensor per row -- the rows of the shared set hold the SAME
    tensor object --, grds [rows], set_len [rows], shared_rows: the caller rows of the shared set).  Rows come in a shuffled order."""
    c = CASES[name]
    dim, T = c["dim"], c["table_rows"]
    g = torch.Generator().manual_seed(c["seed"])
    table = torch.randn((T, dim), generator=g).double()
    block = [0]

    def new_block(n):
        ids = torch.arange(block[0] * LADDER, block[0] * LADDER + n)
        block[0] += 1
        assert block[0] * LADDER <= T
        return ids

    def crowd(own_blocks, n):
        own = set(i for b in own_blocks for i in range(b * LADDER, (b + 1) * LADDER))
        rest = torch.tensor([i for i in range(T) if i not in own])
        return rest[torch.randperm(len(rest), generator=g)[:n]]

    gens, cands, ladders = [], [], []
    for n in c["lens"]:
        u = _direction(dim, (0, 2, 3), g)
        nl = min(n, LADDER)
        b0 = block[0]
        ids = new_block(nl)
        table[ids] = _ladder(u, nl, g)
        cand = torch.cat([ids, crowd([b0], n - nl)])
        cands.append(cand[torch.randperm(n, generator=g)])
        gens.append(u * float(0.5 + 2.0 * torch.rand((), generator=g)))
        ladders.append(ids)
    shared_first = len(gens)
    if c["shared"]:
        n, rows = c["shared"]
        u, v = _direction(dim, (0, 3), g), _direction(dim, (2,), g)
        b0 = block[0]
        ids_u, ids_v = new_block(LADDER), new_block(LADDER)
        table[ids_u], table[ids_v] = _ladder(u, LADDER, g), _ladder(v, LADDER, g)
        cand = torch.cat([ids_u, ids_v, crowd([b0, b0 + 1], n - 2 * LADDER)])
        cand = cand[torch.randperm(n, generator=g)]
        for r in range(rows):
            d = (u, v)[r % 2] + SHARED_JITTER / math.sqrt(dim) * torch.randn((dim,), generator=g).double()
            gens.append(d * float(0.5 + 2.0 * torch.rand((), generator=g)))
            cands.append(cand)                             # one object for all rows of the set
            ladders.append((ids_u, ids_v)[r % 2])
    grds = [_plant_grd(GRD_RANKS[i % len(GRD_RANKS)], ladders[i], cands[i], T) for i in range(len(gens))]
    perm = torch.randperm(len(gens), generator=g).tolist()
    return dict(gen=torch.stack([gens[i] for i in perm]).float(), table=table.float(), candidates=[cands[i] for i in perm],
                grds=torch.tensor([grds[i] for i in perm]), set_len=[len(cands[i]) for i in perm],
                shared_rows=[r for r, i in enumerate(perm) if i >= shared_first])


# ------------------------------------------------------------------ rows the reference defines no order for
SPECIAL_DIM, SPECIAL_TABLE_ROWS, SPECIAL_SEED = 64, 400, 74
SPECIAL_ROWS = ("dup", "twins", "nan", "zero")


def special_inputs():
    """Four rows over a small table, each with a set of its own shorter than the top-N list (so the padding shows too):
      dup    one id twice in the list: a planted tie at rank 3;
      twins  two bit-equal table rows under different ids;
      nan    two candidates whose table rows are zero: NaN similarities, which rank first;
      zero   a candidate orthogonal to the row with a dot product of exactly zero (disjoint supports) and its negation: a -0.0 / +0.0
             pair in IEEE arithmetic, ranked below ten positive and above five negative similarities.
    Among equals the lower POSITION comes first: the expected order is ``expected_ranking``'s fp64 stable sort, not the reference's."""
    dim, T = SPECIAL_DIM, SPECIAL_TABLE_ROWS
    g = torch.Generator().manual_seed(SPECIAL_SEED)
    table = torch.randn((T, dim), generator=g).double()
    shuffle = lambda t: t[torch.randperm(len(t), generator=g)]
    gens, cands = [], []
    # dup
    u = _direction(dim, (0, 2), g)
    table[0:20] = _ladder(u, 20, g)
    cand = shuffle(torch.arange(0, 20)).tolist()
    cand.insert(len(cand) - 2, 3)
    gens.append(u * 1.7); cands.append(torch.tensor(cand))
    # twins
    u = _direction(dim, (0, 2), g)
    table[20:40] = _ladder(u, 20, g)
    table[40] = table[23]
    gens.append(u * 0.6); cands.append(shuffle(torch.arange(20, 41)))
    # nan
    u = _direction(dim, (0, 2), g)
    table[41:61] = _ladder(u, 20, g)
    table[61:63] = 0.0
    gens.append(u * 2.2); cands.append(shuffle(torch.arange(41, 63)))
    # zero: the row lives on the first half of the dimensions, w on the second half
    u = torch.zeros(dim, dtype=torch.float64)
    u[0:dim // 2:2] = _signs(dim // 4, g) / math.sqrt(dim // 4)
    lad = _ladder(u, 10, g)
    table[63:73] = lad
    table[73:78] = _ladder(u, 5, g) * torch.where(u != 0, -1.0, 1.0)[None, :]       # the u component mirrored: similarities -a_j
    w = torch.zeros(dim, dtype=torch.float64)
    w[dim // 2::2] = _signs(dim // 4, g)
    table[78], table[79] = w, -w
    rest = shuffle(torch.arange(63, 78)).tolist()
    rest.insert(2, 79)                                    # -w at the lower position, w later
    rest.insert(9, 78)
    gens.append(u * 1.3); cands.append(torch.tensor(rest))
    return dict(gen=torch.stack(gens).float(), table=table.float(), candidates=cands)


def cosine64(gen_row, table, cand):
    """The row's similarities in fp64 from the fp32 inputs: <g, t> / (|g| |t|); a zero row gives NaN."""
    gd, t = gen_row.double(), table.double()[cand]
    with np.errstate(all="ignore"):
        return ((t @ gd) / (gd.norm() * t.norm(dim=1))).numpy()


def expected_ranking(sims, top_n):
    """Positions of the best ``top_n`` of ``sims`` under the row's rule: descending, a NaN above everything, among equal values
    (-0.0 == +0.0, NaN == NaN) the lower position first -- a stable sort."""
    s = np.asarray(sims, dtype=np.float64)
    key = np.where(np.isnan(s), np.inf, s) + 0.0
    order = sorted(range(len(s)), key=lambda j: (not np.isnan(s[j]), -key[j], j))
    return order[:top_n]


def ladder_gaps(sims, through):
    """Gaps between consecutive sorted similarities down to rank ``through`` (0-based, inclusive)."""
    top = np.sort(np.asarray(sims, dtype=np.float64))[::-1][:through + 1]
    return top[:-1] - top[1:]


def recall_from_hit_positions(hit_pos, cutoffs):
    """``[#{r : 0 <= hit_pos[r] < N} / rows for N in cutoffs]``: the reference's ``grd in topN_iids[:N]`` count (eval_utils.py:754-762)
    from the first rank at which each row's list holds its ground truth (-1: nowhere)."""
    hp = [int(h) for h in hit_pos]
    return [sum(1 for h in hp if 0 <= h < int(c)) / len(hp) for c in cutoffs]


def checksum(inp) -> np.ndarray:
    ts = [inp["gen"], inp["table"]]
    ids = torch.cat([c for c in inp["candidates"]]).double()
    return np.array([float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts] + [float(ids.sum()), float((ids * ids).sum())])
