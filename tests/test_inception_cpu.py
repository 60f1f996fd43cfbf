"""CPU tier (-m "not gpu"): the host-only half of the FID / Inception Score row -- the C ABI of the ``dfh_incep_*``
family in all three places (header, both libraries, ctypes), the parameter tables of both variants, the launch plan against the shape
table (geometry, concatenation slices, workspace bounds), the Python classes' refusals and weight routes, the plain-torch restatement
against the fixtures, ``frechet_distance`` against closed forms, and a sanitizer run of the table, plan and guards as a stand-alone
program.  No compute call is made here; the kernels are held to the same fixtures on the GPU (tests/test_gpu_inception.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from difashion_amd import inception as I
from tests import helpers_inception as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ["dfh_incep_" + n for n in ("create", "destroy", "num_params", "param_name", "param_ndim", "param_dim", "packed_bytes", "pack", "plan_count",
                                     "plan_entry", "workspace_bytes", "forward", "prep", "conv_bn_relu", "pool", "global_mean", "fc_softmax", "is_rows",
                                     "is_splits", "stats")]
K_PREP, K_CONV, K_POOL, K_GMEAN, K_FC, K_SOFTMAX = range(6)
POOL_MAX_S2, POOL_MAX_S1, POOL_AVG_INCL, POOL_AVG_EXCL = range(4)


def make_ctx(variant, mask, classes=50, resize=1, normalize=1):
    h = C.c_void_p()
    _lib.call("dfh_incep_create", C.byref(_lib.IncepConfigC({"tv": 0, "fid": 1}[variant], classes, resize, normalize, mask)), C.byref(h))
    return h


def test_every_incep_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "difashion_hip.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(dfh_incep_[a-z0-9_]+)\s*\(", src)) == set(FAMILY)
    for lib_name in _lib._LIB_NAMES.values():                                   # both storage builds export the row
        lib = C.CDLL(os.path.join(_lib.CSRC, lib_name))
        for n in FAMILY:
            assert hasattr(lib, n), f"{n} not exported by {lib_name}"
    for n in FAMILY:
        assert n in _lib.SIGNATURES, n
    assert C.sizeof(_lib.IncepLaunchC) == 19 * 4 + 4 + 4 * 8 + 48                 # 19 ints, padding, 4 size_t, the name
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "inception.hip" in mk and re.search(r"inception\.o:.*\n\t.*-ffp-contract=off", mk)
    text = open(os.path.join(_lib.CSRC, "inception.hip")).read()
    # one source for both builds, fp32 / fp64 only, no atomics, nothing allocated, one conv kernel
    assert not re.search(r"\b(bf16_t|h16x8_t|DFH_F16|pack2bf|f2bf|atomic[A-Z]\w*|__hip_atomic\w*|getenv|hipMalloc\w*)\b", text)
    assert len(re.findall(r"__global__[^;{]*?void incep_conv\w*kernel", text)) == 1
    assert "mfma_f64_16x16x4f64" in text and "TileKahanSum" in text


@pytest.mark.parametrize("variant", ["fid", "tv"])
def test_parameter_table_is_the_restatements_state_dict(variant):
    m = da.FIDInceptionV3(init_seed=None) if variant == "fid" else da.InceptionV3(init_seed=None)
    table = m.param_table()
    want = H.param_shapes(variant)
    assert len(table) == (470 if variant == "fid" else 472) == len(want)
    assert table == [(k, tuple(v)) for k, v in want.items()]
    sd = m.state_dict()
    assert list(sd) == [n for n, _ in table] and all(tuple(sd[n].shape) == s for n, s in table)
    assert table[0] == ("Conv2d_1a_3x3.conv.weight", (32, 3, 3, 3)) and table[4] == ("Conv2d_1a_3x3.bn.running_var", (32,))
    assert ("Mixed_6c.branch7x7dbl_2.conv.weight", (160, 160, 7, 1)) in table and ("Mixed_7c.branch3x3dbl_2.conv.weight", (384, 448, 3, 3)) in table
    ctx = make_ctx(variant, 8)
    lib = _lib.raw()
    try:
        for i in (-1, len(table), 10_000_000):
            assert lib.dfh_incep_param_name(ctx, i) == b"" and lib.dfh_incep_param_ndim(ctx, i) == 0 and lib.dfh_incep_param_dim(ctx, i, 0) == 0
        packed = 4 * sum(s[0] * (s[2] * s[3] * ((s[1] + 3) // 4 * 4) + 2) for n, s in want.items() if n.endswith(".conv.weight"))
        assert lib.dfh_incep_packed_bytes(ctx) == packed
    finally:
        lib.dfh_incep_destroy(ctx)


def test_foreign_keys_are_dropped_and_the_weight_routes_agree(tmp_path):
    for variant, cls in (("fid", da.FIDInceptionV3), ("tv", da.InceptionV3)):
        params = H.make_params(variant)
        foreign = H.foreign_state_dict(params, variant)
        assert any(k.startswith("AuxLogits.") for k in foreign) and any(k.endswith("num_batches_tracked") for k in foreign)
        a = cls(init_seed=None)
        a.load_state_dict(foreign)                                               # strict: what is left is exactly the table
        b = cls(init_seed=None).load_reference_weights(foreign)
        assert list(a.state_dict()) == list(params)
        assert all(torch.equal(a.state_dict()[k], params[k]) and torch.equal(b.state_dict()[k], params[k]) for k in params)
        with pytest.raises(RuntimeError, match="Unexpected key"):
            cls(init_seed=None).load_state_dict(dict(foreign, **{"Mixed_8a.conv.weight": torch.zeros(1)}))
        with pytest.raises(KeyError, match="Mixed_7c.branch_pool.bn.bias"):
            cls(init_seed=None).load_reference_weights({k: v for k, v in foreign.items() if k != "Mixed_7c.branch_pool.bn.bias"})
        a.save_pretrained(str(tmp_path / variant))
        assert sorted(os.listdir(tmp_path / variant)) == ["config.json", "model.safetensors"]
        d = cls.from_pretrained(str(tmp_path), subfolder=variant, max_workspace_bytes=1 << 30)
        assert d.max_workspace_bytes == 1 << 30 and dict(d.config) == dict(a.config)
        assert all(torch.equal(d.state_dict()[k], params[k]) for k in params)
    torch.save(H.foreign_state_dict(H.make_params("tv", 7), "tv") | {"AuxLogits.fc.weight": torch.zeros(7, 768)}, str(tmp_path / "cls.pth"))
    c = da.InceptionV3(model_path=str(tmp_path / "cls.pth"), num_classes=7, init_seed=None)
    assert c.state_dict()["fc.weight"].shape == (7, 2048) and torch.equal(c.state_dict()["fc.bias"], H.make_params("tv", 7)["fc.bias"])
    # the seeded stand-ins: unit running variance, something to compute with
    s = da.FIDInceptionV3().state_dict()
    assert float(s["Mixed_5b.branch1x1.bn.running_var"].min()) == 1.0 and float(s["Conv2d_1a_3x3.conv.weight"].abs().max()) > 0


def conv_out(v, k, s, p):
    return (v + 2 * p - k) // s + 1


def expected_walk(variant, last_block, side_h, side_w):
    """(name, kind, Hin, Win, Cin, Hout, Wout, Cout, ldc, offset, pool mode) of every launch that touches an activation, from the shape
    table and torchvision's block definitions alone."""
    avg = POOL_AVG_INCL if variant == "tv" else POOL_AVG_EXCL
    out = []

    def conv(name, h, w, cin, ldc=None, offset=0):
        _, tcin, cout, k, s, p = H.LAYERS[name]
        assert (tcin + 3) // 4 * 4 == cin, name
        oh, ow = conv_out(h, k[0], s, p[0]), conv_out(w, k[1], s, p[1])
        out.append((name, K_CONV, h, w, cin, oh, ow, cout, ldc or cout, offset, -1, k, s, p))
        return oh, ow, cout

    def pool(name, mode, h, w, c, ldc=None, offset=0):
        oh, ow = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == POOL_MAX_S2 else (h, w)
        out.append((name, K_POOL, h, w, c, oh, ow, c, ldc or c, offset, mode, (3, 3), 2 if mode == POOL_MAX_S2 else 1, (0, 0) if mode == POOL_MAX_S2 else (1, 1)))
        return oh, ow, c

    h, w, c = side_h, side_w, 4
    for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        h, w, c = conv(n, h, w, c)
    h, w, c = pool("maxpool1", POOL_MAX_S2, h, w, c)
    if last_block >= 1:
        for n in ("Conv2d_3b_1x1", "Conv2d_4a_3x3"):
            h, w, c = conv(n, h, w, c)
        h, w, c = pool("maxpool2", POOL_MAX_S2, h, w, c)
    blocks = []
    if last_block >= 2:
        blocks += ["Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"]
    if last_block >= 3:
        blocks += ["Mixed_7a", "Mixed_7b", "Mixed_7c"]
    chains = {"A": [["branch1x1"], ["branch5x5_1", "branch5x5_2"], ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], ["POOL", "branch_pool"]],
              "B": [["branch3x3"], ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], ["POOL"]],
              "C": [["branch1x1"], ["branch7x7_1", "branch7x7_2", "branch7x7_3"],
                    ["branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"], ["POOL", "branch_pool"]],
              "D": [["branch3x3_1", "branch3x3_2"], ["branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"], ["POOL"]]}
    for b in blocks:
        kind = H.BLOCK_KIND[b]
        reduce = kind in "BD"
        oh, ow = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if reduce else (h, w)
        if kind == "E":
            widths = [320, 384, 384, 384, 384, 192]
        else:
            widths = [c if ch == ["POOL"] else H.LAYERS[f"{b}.{ch[-1]}"][2] for ch in chains[kind]]
        ldc = sum(widths)
        offs = np.concatenate([[0], np.cumsum(widths)]).tolist()
        if kind == "E":
            conv(f"{b}.branch1x1", h, w, c, ldc, offs[0])
            conv(f"{b}.branch3x3_1", h, w, c)
            conv(f"{b}.branch3x3_2a", h, w, 384, ldc, offs[1])
            conv(f"{b}.branch3x3_2b", h, w, 384, ldc, offs[2])
            conv(f"{b}.branch3x3dbl_1", h, w, c)
            conv(f"{b}.branch3x3dbl_2", h, w, 448)
            conv(f"{b}.branch3x3dbl_3a", h, w, 384, ldc, offs[3])
            conv(f"{b}.branch3x3dbl_3b", h, w, 384, ldc, offs[4])
            mode = POOL_MAX_S1 if (variant == "fid" and b == "Mixed_7c") else avg
            pool("branch_pool.max" if mode == POOL_MAX_S1 else "branch_pool.avg", mode, h, w, c)
            conv(f"{b}.branch_pool", h, w, c, ldc, offs[5])
        else:
            for ch, off in zip(chains[kind], offs):
                th, tw, tc = h, w, c
                for i, step in enumerate(ch):
                    last = i == len(ch) - 1
                    if step == "POOL":
                        if reduce:
                            pool(f"{b}.max", POOL_MAX_S2, th, tw, tc, ldc, off)
                        else:
                            th, tw, tc = pool("branch_pool.avg", avg, th, tw, tc)
                    else:
                        th, tw, tc = conv(f"{b}.{step}", th, tw, tc, ldc if last else None, off if last else 0)
        h, w, c = oh, ow, ldc
    return out


@pytest.mark.parametrize("variant,blocks", [("fid", (0,)), ("fid", (2,)), ("fid", (3,)), ("fid", (0, 1, 2, 3)), ("tv", (3,)), ("tv", (0, 1, 2, 3))])
def test_the_plan_matches_the_shape_table(variant, blocks):
    mask = sum(1 << b for b in blocks)
    ctx = make_ctx(variant, mask)
    try:
        for n, Hh, Ww in [(1, 299, 299), (3, 75, 91)]:
            plan = I.plan(ctx, n, Hh, Ww)
            ws = _lib.raw().dfh_incep_workspace_bytes(ctx, n, Hh, Ww)
            assert ws > 0
            assert plan[0].kind == K_PREP and (plan[0].Hin, plan[0].Win, plan[0].Cin, plan[0].Hout, plan[0].Wout, plan[0].Cout) == (Hh, Ww, 3, 299, 299, 4)
            assert plan[0].src_region == -1 and plan[0].src_floats == n * 3 * Hh * Ww
            # every launch's geometry equals the shape table, in the order of the walk
            body = [e for e in plan if e.kind in (K_CONV, K_POOL)]
            want = expected_walk(variant, max(blocks), 299, 299)
            assert len(body) == len(want)
            for e, w in zip(body, want):
                got = (e.name.decode(), e.kind, e.Hin, e.Win, e.Cin, e.Hout, e.Wout, e.Cout, e.ldc, e.offset, e.pool_mode, (e.KH, e.KW), e.stride, (e.padH, e.padW))
                assert got == w
                if e.kind == K_CONV:
                    assert H.layer_table()[e.conv][0] == w[0]
            assert [e.conv for e in body if e.kind == K_CONV] == list(range(sum(e.kind == K_CONV for e in body)))
            # the taps: one global mean per requested block, of the right width
            gm = [e for e in plan if e.kind == K_GMEAN]
            assert [(e.block, e.Cin, e.dst_region, e.dst_floats) for e in gm] == [(b, H.BLOCK_DIMS[b], -2, n * H.BLOCK_DIMS[b]) for b in blocks]
            head = [e.kind for e in plan if e.kind in (K_FC, K_SOFTMAX)]
            assert head == ([K_FC, K_SOFTMAX] if variant == "tv" else [])
            if variant == "tv":
                assert plan[-1].dst_region == -3 and plan[-1].dst_floats == n * 50 and plan[-2].Cin == 2048 and plan[-2].Cout == 50
            # the slices of each concatenation tile [0, ldc) exactly once, and nothing reads a tensor before it is complete
            live = {}                                                            # region -> (H, W, ldc, covered channels)
            for e in plan:
                if e.src_region >= 0 and e.kind in (K_CONV, K_POOL, K_GMEAN):
                    hh, ww, ldc, cov = live[e.src_region]
                    assert (hh, ww, ldc) == (e.Hin, e.Win, e.Cin) and cov.all(), (e.name, "reads an incomplete or mismatched tensor")
                    assert e.src_floats == n * hh * ww * ldc
                if e.dst_region >= 0 and e.kind in (K_PREP, K_CONV, K_POOL):
                    assert e.dst_region != e.src_region
                    key = (e.Hout, e.Wout, e.ldc)
                    if e.dst_region not in live or live[e.dst_region][:3] != key or live[e.dst_region][3].all():
                        live[e.dst_region] = key + (np.zeros(e.ldc, dtype=bool),)
                    cov = live[e.dst_region][3]
                    assert not cov[e.offset:e.offset + e.Cout].any(), (e.name, "writes a slice twice")
                    cov[e.offset:e.offset + e.Cout] = True
                    assert e.dst_floats == n * e.Hout * e.Wout * e.ldc
                # every read and write lies inside workspace_bytes (the last 256 bytes are the caller's alignment slack)
                for region, off, fl in ((e.src_region, e.src_off, e.src_floats), (e.dst_region, e.dst_off, e.dst_floats)):
                    if region >= 0:
                        assert off % 64 == 0 and 4 * (off + fl) + 256 <= ws, e.name
            assert all(cov.all() for _, _, _, cov in live.values())
            # regions do not overlap: a launch's source and destination ranges are disjoint
            for e in plan:
                if e.src_region >= 0 and e.dst_region >= 0:
                    assert e.src_off + e.src_floats <= e.dst_off or e.dst_off + e.dst_floats <= e.src_off, e.name
    finally:
        _lib.raw().dfh_incep_destroy(ctx)


def test_plan_without_resize_and_shape_refusals():
    ctx = make_ctx("fid", 8, resize=0)
    try:
        plan = I.plan(ctx, 2, 75, 91)
        assert (plan[0].Hout, plan[0].Wout) == (75, 91)
        last = [e for e in plan if e.kind == K_CONV][-1]
        assert (last.Hout, last.Wout, last.ldc) == (1, 1, 2048)
        assert _lib.raw().dfh_incep_workspace_bytes(ctx, 1, 74, 91) == 0
        with pytest.raises(_lib.DfhError, match="at least 75"):
            I.plan(ctx, 1, 91, 74)
        with pytest.raises(_lib.DfhError, match=r"n must be in \[1, 65535\]"):
            I.plan(ctx, 0, 91, 91)
        with pytest.raises(_lib.DfhError, match="out of range"):
            _lib.call("dfh_incep_plan_entry", ctx, 1, 91, 91, len(I.plan(ctx, 1, 91, 91)), C.byref(_lib.IncepLaunchC()))
    finally:
        _lib.raw().dfh_incep_destroy(ctx)
    h = C.c_void_p()
    for cfg, match in [((2, 50, 1, 1, 8), "unsupported variant"), ((1, 0, 1, 1, 0), "block_mask"), ((1, 0, 1, 1, 16), "block_mask"),
                       ((0, 50, 1, 1, 7), "block_mask must include block 3"), ((0, 0, 1, 1, 8), "num_classes"), ((0, 5000, 1, 1, 8), "num_classes")]:
        with pytest.raises(_lib.DfhError, match=match):
            _lib.call("dfh_incep_create", C.byref(_lib.IncepConfigC(*cfg)), C.byref(h))


def test_constructor_and_tensor_refusals():
    with pytest.raises(NotImplementedError, match="requires_grad=True"):
        da.FIDInceptionV3(requires_grad=True, init_seed=None)
    with pytest.raises(NotImplementedError, match="use_fid_inception=False"):
        da.FIDInceptionV3(use_fid_inception=False, init_seed=None)
    for blocks in [(), (4,), (-1,), (1, 1)]:
        with pytest.raises(ValueError, match="output_blocks"):
            da.FIDInceptionV3(blocks, init_seed=None)
    with pytest.raises(ValueError, match="num_classes"):
        da.InceptionV3(num_classes=0, init_seed=None)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        da.FIDInceptionV3(max_workspace_bytes=0, init_seed=None)
    m = da.FIDInceptionV3((3, 0), init_seed=None)
    assert m.output_blocks == [0, 3] and m.last_needed_block == 3 and not m.training and not any(p.requires_grad for p in m.parameters())
    assert da.FIDInceptionV3.BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3}
    with pytest.raises(NotImplementedError, match="inference only"):
        m.train()
    assert m.eval() is m
    x = torch.zeros(2, 3, 32, 32)
    c = da.InceptionV3(init_seed=None)
    for call in (lambda: m(x), lambda: c(torch.zeros(2, 3, 299, 299)), lambda: c.feature_extract(torch.zeros(2, 3, 299, 299)),
                 lambda: da.activation_statistics(m, x), lambda: da.fid_given_data(x, x, model=m),
                 lambda: da.inception_score_given_data(c, x, torch.zeros(2, dtype=torch.long)), lambda: da.inception_rows(torch.zeros(2, 50))):
        with pytest.raises(da.DfhError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="299 x 299"):
        da.InceptionV3(init_seed=None)(x)
    with pytest.raises(ValueError, match="dims must be one of"):
        da.fid_given_data(x, x, dims=100, model=m)
    with pytest.raises(_lib.DfhError, match="max_workspace_bytes"):
        da.FIDInceptionV3(init_seed=None, max_workspace_bytes=1000).images_per_call(299, 299)
    big = da.FIDInceptionV3((0,), init_seed=None)
    need = lambda n: _lib.raw().dfh_incep_workspace_bytes(big._context(), n, 64, 64)
    assert da.FIDInceptionV3((0,), init_seed=None, max_workspace_bytes=need(3)).images_per_call(64, 64) == 3
    assert da.FIDInceptionV3((0,), init_seed=None, max_workspace_bytes=need(3) - 1).images_per_call(64, 64) == 2


@pytest.mark.parametrize("name", list(H.CASES))
def test_restatement_reproduces_the_fixtures(name):
    assert os.path.getsize(H.fixture_path("inception_" + name)) < 1 << 20
    variant, params, x, fx = H.load_case(name)
    np.testing.assert_allclose(fx["checksum"], H.checksum(params, x), rtol=1e-12)
    assert x.shape == (H.IMAGES, 3) + H.CASES[name][1:3] and all(0.2 < v < 0.8 for v in fx["live"])
    with torch.no_grad():
        r = H.Net(params, variant, torch.float32).forward(x)
    for b in range(4):
        t32, t64 = fx[f"tap{b}_32"], fx[f"tap{b}_64"]
        assert t64.dtype == np.float64 and t64.shape == (H.IMAGES, H.BLOCK_DIMS[b]) and np.isfinite(t64).all()
        # the same torch build reproduces its own fp32 run; another build may sum in another order: hold it to the run's own distance
        d = H.rel(t32, t64)
        assert 0 < d < 1e-2
        assert H.rel(r["taps"][b], t64) < 3 * d
    if variant == "tv":
        assert fx["labels"].tolist() == np.argmax(fx["probs_64"], 1).tolist() == torch.argmax(r["probs"], 1).tolist()
        assert H.rel(r["probs"], fx["probs_64"]) < 3 * H.rel(fx["probs_32"], fx["probs_64"])
        np.testing.assert_allclose(fx["probs_64"].sum(1), 1.0, rtol=1e-12)


def test_restatement_of_the_score_arithmetic():
    g = torch.Generator().manual_seed(1)
    p = torch.softmax(2.0 * torch.randn((10, 50), generator=g), dim=1)
    cate = torch.argmax(p, 1)
    acc, me, se, ms, ss = H.inception_score(p, cate, 1)
    assert acc == 1.0 and np.isnan(se) and np.isnan(ss) and 0 < me < np.log(50) and 1 < ms < 50
    u = torch.full((4, 50), 1 / 50)
    _, me, _, ms, _ = H.inception_score(u, torch.zeros(4, dtype=torch.long), 2)
    assert abs(me - np.log(50)) < 1e-5 and abs(ms - 1) < 1e-5


def spd(rng, d, scale=1.0):
    a = rng.standard_normal((d, d))
    return scale * (a @ a.T / d + 0.1 * np.eye(d))


def test_frechet_distance_against_closed_forms():
    rng = np.random.default_rng(0)
    d = 64
    mu, s = rng.standard_normal(d), spd(rng, d)
    traces = 2 * np.trace(s)
    assert abs(da.frechet_distance(mu, s, mu, s)) <= 1e-9 * traces
    # commuting (diagonal) covariances: sum (sqrt a - sqrt b)^2 + |mu1 - mu2|^2
    a, b = rng.uniform(0.5, 2.0, d), rng.uniform(0.5, 2.0, d)
    mu2 = rng.standard_normal(d)
    want = float(((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((mu - mu2) ** 2).sum())
    got = da.frechet_distance(mu, np.diag(a), mu2, np.diag(b))
    scale = float(a.sum() + b.sum() + ((mu - mu2) ** 2).sum())
    assert abs(got - want) <= 1e-10 * scale
    # symmetric in its arguments
    s2 = spd(rng, d, 1.5)
    f12, f21 = da.frechet_distance(mu, s, mu2, s2), da.frechet_distance(mu2, s2, mu, s)
    assert f12 > 0 and abs(f12 - f21) <= 1e-10 * (np.trace(s) + np.trace(s2) + ((mu - mu2) ** 2).sum())
    # tensors are accepted as numpy arrays are
    assert da.frechet_distance(torch.from_numpy(mu), torch.from_numpy(s), torch.from_numpy(mu2), torch.from_numpy(s2)) == f12
    # a rank-deficient pair (fewer samples than dimensions): no exception, a finite value, whether or not this scipy's root of the
    # singular product is finite (the eps branch itself is driven in the next test)
    x, y = rng.standard_normal((5, d)), rng.standard_normal((5, d)) + 0.5
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = da.frechet_distance(x.mean(0), np.cov(x, rowvar=False), y.mean(0), np.cov(y, rowvar=False))
    assert np.isfinite(f) and f > 0
    with pytest.raises(ValueError, match="different lengths"):
        da.frechet_distance(mu, s, mu[:3], s)
    with pytest.raises(ValueError, match="different dimensions"):
        da.frechet_distance(mu, s, mu, s[:3, :3])


def test_frechet_distance_eps_branch(monkeypatch):
    """This scipy's sqrtm stays finite on the rank-deficient pair above, so the branch is driven here: a root that comes back
    non-finite is taken again of (s1 + eps I)(s2 + eps I), and a complex root passes only with an imaginary diagonal below 1e-3."""
    from scipy import linalg
    rng = np.random.default_rng(1)
    d = 8
    mu, s1, s2 = rng.standard_normal(d), spd(rng, d), spd(rng, d, 2.0)
    real, seen = linalg.sqrtm, []

    def first_root_fails(a, *args, **kw):
        seen.append(np.array(a))
        return np.full_like(a, np.nan) if len(seen) == 1 else real(a, *args, **kw)

    monkeypatch.setattr(linalg, "sqrtm", first_root_fails)
    got = da.frechet_distance(mu, s1, mu, s2, eps=1e-6)
    assert len(seen) == 2 and np.array_equal(seen[0], s1.dot(s2)) and np.array_equal(seen[1], (s1 + 1e-6 * np.eye(d)).dot(s2 + 1e-6 * np.eye(d)))
    monkeypatch.setattr(linalg, "sqrtm", real)
    assert abs(got - da.frechet_distance(mu, s1, mu, s2)) <= 1e-4 * (np.trace(s1) + np.trace(s2))     # the offset moves the traces by d eps
    monkeypatch.setattr(linalg, "sqrtm", lambda a, *args, **kw: real(a, *args, **kw) + 1e-4j * np.eye(d))
    assert abs(da.frechet_distance(mu, s1, mu, s2) - got) <= 1e-4 * (np.trace(s1) + np.trace(s2))
    monkeypatch.setattr(linalg, "sqrtm", lambda a, *args, **kw: real(a, *args, **kw) + 1e-2j * np.eye(d))
    with pytest.raises(ValueError, match="Imaginary component"):
        da.frechet_distance(mu, s1, mu, s2)


def test_table_plan_and_guards_under_the_host_sanitizers(tmp_path):
    """csrc/inception.hip's host side, built with tests/native/inception_host_check.hip into a program of its own under
    -fsanitize=address,undefined: the tables, the sizes and the plan equal the library's, every guard refuses, nothing is launched, no report."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the sanitizer build needs the compiler the library is built with")
    exe = str(tmp_path / "inception_host_check")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(_lib.CSRC, "inception.hip"),
           os.path.join(ROOT, "tests", "native", "inception_host_check.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    shapes = [(1, 299, 299), (3, 75, 91)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")                      # the HIP runtime's start-up allocations are not ours to free
    r = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    lib = _lib.raw()
    for variant, mask in (("fid", 15), ("tv", 8)):
        table = [l.split()[3:] for l in lines if l.startswith(f"param {variant} ")]
        want = H.param_shapes(variant)
        assert [(t[0], tuple(map(int, t[1:]))) for t in table] == [(k, tuple(v)) for k, v in want.items()]
        ctx = make_ctx(variant, mask)
        try:
            assert f"params {variant} {len(want)} floats {sum(int(np.prod(s)) for s in want.values())} packed {lib.dfh_incep_packed_bytes(ctx)}" in lines
            for s in shapes:
                plan = I.plan(ctx, *s)
                assert f"workspace {variant} {s[0]} {s[1]} {s[2]} -> {lib.dfh_incep_workspace_bytes(ctx, *s)} launches {len(plan)}" in lines
            launches = [l for l in lines if l.startswith(f"launch {variant} ")]
            assert len(launches) == sum(len(I.plan(ctx, *s)) for s in shapes)
        finally:
            lib.dfh_incep_destroy(ctx)
    guards = [l for l in lines if l.startswith("guard ")]
    assert len(guards) == 5 + (17 + 2) + (18 + 2) + 1 + 17 and all(": refused (" in l for l in guards), guards
    assert lines[-1] == "launches 0 failures 0"
